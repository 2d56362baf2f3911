"""The float64 references and arithmetic bounds of tests/helpers.py (used at arena size by tests/test_gpu_update_production.py) are shown to
bite, on the CPU: fp32 torch emulations of the kernels of csrc/multi_tensor.hip (the same operations in the same order, one rounding each) pass
them, and every planted error below fails them:
  * one element off by twice its own bound at the last index (per kernel: the bound of a 98-chunk mean is ~100 u |a|, of a momentum 4 u S);
  * the scalar tail (the last n % 4 elements) left unprocessed;
  * rows j and j+1 swapped (per-row norms, per-row eps_n of the recombination: the plain mean is symmetric in its rows and cannot see it);
  * 1/(c+j) instead of 1/(c+j+1);
  * one grid-stride pass skipped (elements [grid*256, 2*grid*256) untouched);
and the scalar rule: a float64 reference with the unrounded 0.9 fails an honest fp32 momentum update, with float32(0.9) it passes.
1 M elements (n % 4 == 2), 98 chunks, counters 0 and 292, the magnitude bands of the GPU cases."""
import numpy as np
import pytest
import torch

from tests.helpers import (U32, clip_coef_ref, distinct_rows, f32r, fd_combine_ref, fd_perturb_ref, norm_bias_ref, reduction_bound,
                           running_mean_ref, sam_ref, sgd_ref, within_bound)

N, G = 1_000_002, 98
GRID = 1024                     # emulated launch: GRID workgroups of 256 threads -> four grid-stride passes over N
F = torch.float32


def _f(x):
    return torch.tensor(x, dtype=F)


def _mean_f32(a0, rows, c0, inv_of=lambda c0, j: 1.0 / (c0 + j + 1)):
    """mt_accumulate_kernel in fp32 torch: a += (v - a) * (float)(1.0 / (double)(c0 + j + 1))."""
    a = a0.clone()
    for j, v in enumerate(rows):
        a = a + (v - a) * _f(inv_of(c0, j))
    return a


@pytest.fixture(scope="module")
def rows():
    torch.manual_seed(0)
    return distinct_rows(G, N, N, 1e-2, 11, "cpu")


@pytest.fixture(scope="module")
def a0():
    return torch.randn(N, generator=torch.Generator().manual_seed(5)) * 1e-2


@pytest.fixture(scope="module", params=[0, 292])
def mean_case(request, rows, a0):
    c0 = request.param
    ref, B, total = running_mean_ref(a0, rows, c0)
    return c0, _mean_f32(a0, rows, c0), ref, B, total


def test_within_bound_reports_the_worst_element():
    ref = torch.zeros(5, dtype=torch.float64)
    got = torch.tensor([0.0, 1.0, -3.0, 0.5, 0.0])
    assert within_bound(got, ref, torch.full((5,), 2.0, dtype=torch.float64)) == (1.5, 2)
    assert within_bound(got, ref, 4.0) == (0.75, 2)
    assert within_bound(torch.zeros(3), torch.zeros(3, dtype=torch.float64), 0.0) == (0.0, 0)               # bound 0: equality
    assert within_bound(torch.tensor([0.0, 1e-30]), torch.zeros(2, dtype=torch.float64), 0.0) == (float("inf"), 1)
    assert within_bound(torch.tensor([0.0, float("nan")]), torch.zeros(2, dtype=torch.float64), 1.0) == (float("inf"), 1)
    assert within_bound(torch.zeros(0), torch.zeros(0, dtype=torch.float64), 1.0) == (0.0, -1)


def test_reduction_bound_values():
    # ResNet-18's arena: 11 float4 per thread in the float4 kernels, 43 elements per thread in the scalar ones -- both inside the 1e-5 the project uses
    assert reduction_bound(11_173_962 // 4, 1024, 8) == (8 * 11 + 16) * U32 < 1e-5
    assert reduction_bound(11_173_962, 1024, 2) == (2 * 43 + 16) * U32 < 1e-5
    assert reduction_bound(60_192_808, 1024, 2) == (2 * 230 + 16) * U32
    assert reduction_bound(10, 1024, 2, extra=4 * U32) == 22 * U32


def test_running_mean_honest_fp32_passes_and_recurrence_equals_closed_form(mean_case, a0):
    c0, got, ref, B, total = mean_case
    closed = (c0 * a0.double() + total) / (c0 + G)
    assert float((ref - closed).abs().max()) <= 1e-13 * max(1.0, float(closed.abs().max()))
    ratio, i = within_bound(got, ref, B)
    print(f"running mean, c0={c0}: honest fp32 worst error/bound {ratio:.3f} at {i}; B/(u|a|) median {float((B / (U32 * ref.abs())).median()):.0f}")
    assert ratio <= 1.0


def test_running_mean_planted_errors_fail(mean_case, rows, a0):
    c0, got, ref, B, _ = mean_case
    bad = got.clone()                                     # one element, twice its own bound, at the last index
    bad[-1] = (ref[-1] + 2.0 * B[-1]).float()
    assert abs(float(bad[-1]) - float(ref[-1])) > float(B[-1])
    ratio, i = within_bound(bad, ref, B)
    assert ratio > 1.0 and i == N - 1
    bad = got.clone()                                     # the scalar tail left unprocessed
    bad[N - N % 4:] = a0[N - N % 4:]
    ratio, i = within_bound(bad, ref, B)
    assert ratio > 1.0 and i >= N - N % 4
    bad = got.clone()                                     # the second grid-stride pass skipped
    bad[GRID * 256:2 * GRID * 256] = a0[GRID * 256:2 * GRID * 256]
    ratio, i = within_bound(bad, ref, B)
    assert ratio > 1.0 and GRID * 256 <= i < 2 * GRID * 256
    if c0:                                                # 1/(c+j) instead of 1/(c+j+1)
        ratio, _ = within_bound(_mean_f32(a0, rows, c0, lambda c, j: 1.0 / (c + j)), ref, B)
        assert ratio > 1.0
    # a fixed 16u |a| would NOT do as the bound of a 98-chunk mean: the honest result exceeds it
    assert within_bound(got, ref, 16 * U32 * ref.abs())[0] > 1.0


def test_row_norms_see_swapped_rows(rows):
    """The mean is symmetric in its rows; the per-row outputs (fused squared norms) are not: the reduction bound tells rows j, j+1 apart."""
    sq64 = rows.double().pow(2).sum(1)
    sq32 = (rows * rows).sum(1)                           # an honest fp32 reduction (torch's pairwise order)
    bound = reduction_bound(N // 4, min(-(-(N // 4) // 256), 1024), 8)
    assert float(((sq32.double() - sq64).abs() / sq64).max()) <= bound
    swapped = sq32.clone()
    swapped[[40, 41]] = sq32[[41, 40]]
    assert float(((swapped.double() - sq64).abs() / sq64).max()) > 1e-5 > bound


@pytest.mark.parametrize("c0", [0, 292])
def test_fd_recombination_bound_and_planted_errors(rows, a0, c0):
    """vhp = (ga - gb) / eps_n[j]; gt = g + cf vhp; running mean -- mt_fd_combine_kernel in fp32 torch."""
    cf = 0.1 / 4
    eps = torch.linspace(1e-3, 1.1e-2, G, dtype=F)
    gen = torch.Generator().manual_seed(3)
    ga = rows + 1e-4 * torch.randn(G, N, generator=gen)

    def kernel(eps_rows, first_only=False):
        a, gts = a0.clone(), []
        for j in range(G):
            vhp = (ga[j] - rows[j]) / eps_rows[j]
            gt = rows[j] + _f(cf) * vhp
            if first_only:
                gts.append(gt)
            a = a + (gt - a) * _f(1.0 / (c0 + j + 1))
            if first_only and j == 1:
                break
        return a, gts

    def refs():
        for j in range(G):
            yield fd_combine_ref(rows[j], ga[j], rows[j], float(eps[j]), cf)

    ref, B, _ = running_mean_ref(a0, refs(), c0)
    got, _ = kernel(eps)
    ratio, i = within_bound(got, ref, B)
    print(f"fd recombination + mean, c0={c0}: honest fp32 worst error/bound {ratio:.3f} at {i}")
    assert ratio <= 1.0
    # per element (fb_mt_fd_combine): honest passes, twice the bound at the last index fails
    _, gts = kernel(eps, first_only=True)
    gt_ref, gt_b = fd_combine_ref(rows[1], ga[1], rows[1], float(eps[1]), cf)
    assert within_bound(gts[1], gt_ref, gt_b)[0] <= 1.0
    bad = gts[1].clone()
    bad[-1] = (gt_ref[-1] + 2.0 * gt_b[-1]).float()
    assert within_bound(bad, gt_ref, gt_b) == (pytest.approx(2.0, rel=0.3), N - 1)
    # eps_n of rows 40 and 41 swapped: the recombination is not symmetric in its rows
    sw = eps.clone()
    sw[[40, 41]] = eps[[41, 40]]
    assert within_bound(kernel(sw)[0], ref, B)[0] > 1.0
    # the fused mean, one element off by twice its own bound at the last index
    bad = got.clone()
    bad[-1] = (ref[-1] + 2.0 * B[-1]).float()
    assert within_bound(bad, ref, B)[0] > 1.0


def _sgd_f32(p, g, m, coef, lr, wd, mu, damp, nesterov, first):
    """mt_clip_sgd_kernel in fp32 torch."""
    gr = g * _f(coef) if coef != 1.0 else g
    d = gr + _f(wd) * p
    buf = None
    if mu != 0.0:
        buf = d if first else _f(mu) * m + (_f(1.0) - _f(damp)) * d
        d = d + _f(mu) * buf if nesterov else buf
    return gr, buf, p - _f(lr) * d


@pytest.fixture(scope="module")
def sgd_inputs(rows):
    gen = torch.Generator().manual_seed(9)
    p = distinct_rows(1, N, N, 1.0, 21, "cpu")[0]
    m = distinct_rows(1, N, N, 1e-2, 22, "cpu")[0]
    return p, rows[3].clone(), m, gen


@pytest.mark.parametrize("first,nesterov,damp,mu,clip", [(1, 1, 0.0, 0.9, None), (0, 1, 0.0, 0.9, None), (0, 0, 0.1, 0.9, None), (0, 1, 0.1, 0.9, "hit"),
                                                          (0, 1, 0.0, 0.9, "miss"), (0, 1, 0.0, 0.0, "hit")])
def test_sgd_bounds_and_planted_errors(sgd_inputs, first, nesterov, damp, mu, clip):
    p, g, m, _ = sgd_inputs
    lr, wd = 0.1, 5e-4
    norm2 = float(np.float32(float(g.double().pow(2).sum())))
    norm = norm2 ** 0.5
    clipv = None if clip is None else (0.5 * norm if clip == "hit" else 2.0 * norm)
    coef, hit = clip_coef_ref(norm2, clipv)
    assert hit == (clip == "hit")
    coef32 = float(_f(clipv) / (_f(norm2).sqrt() + _f(1e-6))) if hit else 1.0
    gr, buf, pn = _sgd_f32(p, g, m, coef32, lr, wd, mu, damp, nesterov, first)
    ref = sgd_ref(p, g, m if mu else None, coef, hit, lr, wd, mu, damp, nesterov, first)
    got = {"grad": gr, "param": pn, **({"mom": buf} if mu else {})}
    assert set(got) == set(ref)
    for k in got:
        ratio, i = within_bound(got[k], *ref[k])
        print(f"sgd first={first} nesterov={nesterov} damp={damp} mu={mu} clip={clip}: {k} worst error/bound {ratio:.3f}")
        assert ratio <= 1.0, (k, ratio, i)
    for k in ("param",) + (("mom",) if mu else ()):
        r, b = ref[k]
        bad = got[k].clone()
        bad[-1] = (r[-1] + 2.0 * b[-1]).float()
        ratio, i = within_bound(bad, r, b)
        assert ratio > 1.0 and i == N - 1, k
        bad = got[k].clone()                               # the second grid-stride pass skipped
        src = p if k == "param" else m
        bad[GRID * 256:2 * GRID * 256] = src[GRID * 256:2 * GRID * 256]
        assert within_bound(bad, r, b)[0] > 1.0, k


def test_scalar_rule_references_use_fp32_rounded_scalars(sgd_inputs):
    """Host scalars reach the kernels as float: the reference must use float32(0.9), not 0.9 (2.6e-8 = 0.44 u relative).
    Where a bound is one rounding wide the unrounded scalar alone breaks it: x * 0.9f (fb_mt_scale, bound u |a x|: a single correctly
    rounded product) FAILS against 0.9 x and passes against float32(0.9) x.  For the momentum update the unrounded reference is measurably
    worse, but it cannot leave the bound 4 u S by itself: every scalar is within u of its fp32 value, so the reference moves by at most u S = a quarter
    of the bound (measured here: 0.20; the worst error/bound goes from 0.49 to 0.61) -- that case asserts the shift, not a failure."""
    import tests.helpers as H

    p, g, m, _ = sgd_inputs
    got = g * _f(0.9)
    assert within_bound(got, *H.scale_ref(g, 0.9))[0] <= 1.0
    ratio = within_bound(got, 0.9 * g.double(), U32 * (0.9 * g.double()).abs())[0]
    print(f"x * 0.9f vs a float64 reference with the unrounded 0.9: worst error/bound {ratio:.2f}")
    assert ratio > 1.0
    assert f32r(0.9) != 0.9 and abs(f32r(0.9) - 0.9) / 0.9 > 2e-8
    _, buf, pn = _sgd_f32(p, g, m, 1.0, 0.1, 5e-4, 0.9, 0.0, 1, 0)
    good = sgd_ref(p, g, m, 1.0, False, 0.1, 5e-4, 0.9, 0.0, 1, 0)
    r_good = within_bound(buf, *good["mom"])[0]
    assert r_good <= 1.0 and within_bound(pn, *good["param"])[0] <= 1.0
    keep = H.f32r
    H.f32r = float                                        # the same reference with the scalars left in double precision
    try:
        bad = H.sgd_ref(p, g, m, 1.0, False, 0.1, 5e-4, 0.9, 0.0, 1, 0)
    finally:
        H.f32r = keep
    r_bad = within_bound(buf, *bad["mom"])[0]
    shift = float(((bad["mom"][0] - good["mom"][0]).abs() / good["mom"][1]).max())
    print(f"momentum: worst error/bound {r_good:.2f} with float32 scalars, {r_bad:.2f} with unrounded ones (reference moved by up to {shift:.2f} of the bound)")
    assert r_bad > r_good and 0.05 < shift <= 0.25


def test_remaining_elementwise_references_accept_honest_fp32(sgd_inputs):
    p, g, m, _ = sgd_inputs
    # fb_mt_fd_perturb
    s, acc, eps = 0.5, 0.3, 1e-2
    v2 = float(np.float32(float((f32r(s) * g.double() + f32r(acc) * m.double()).pow(2).sum())))
    eps_n32 = _f(eps) / _f(v2).sqrt()
    eps_n64 = f32r(eps) / v2 ** 0.5
    assert abs(float(eps_n32) - eps_n64) <= 4 * U32 * eps_n64
    alpha = _f(-0.5) * eps_n32
    out = p + alpha * (_f(s) * g + _f(acc) * m)
    assert within_bound(out, *fd_perturb_ref(p, g, s, -0.5 * eps_n64, m, acc))[0] <= 1.0
    bad = out.clone()
    bad[N - N % 4:] = p[N - N % 4:]
    assert within_bound(bad, *fd_perturb_ref(p, g, s, -0.5 * eps_n64, m, acc))[0] > 1.0
    # fb_mt_sam_ascent (clip hit and not)
    norm2 = float(np.float32(float(g.double().pow(2).sum())))
    for clip in (None, 0.5 * norm2 ** 0.5):
        ref = sam_ref(p, g, norm2, clip, 0.05)
        norm = _f(norm2).sqrt()
        coef = _f(clip) / (norm + _f(1e-6)) if clip is not None else _f(1.0)
        e = (g * coef) * (_f(0.05) / (norm * coef + _f(1e-12)))
        assert ref["hit"] == (clip is not None)
        assert abs(float(norm * coef) - ref["norm_c"]) <= (2 + 4) * U32 * ref["norm_c"]
        assert within_bound(e, *ref["e"])[0] <= 1.0 and within_bound(p + e, *ref["theta"])[0] <= 1.0
        assert within_bound(e * _f(1.0 + 2e-6), *ref["e"])[0] > 1.0
    # fb_mt_norm_bias
    pn2 = float(np.float32(float(p.double().pow(2).sum())))
    for nt, bias in ((1, 0.9 * pn2 ** 0.5), (1, 1.1 * pn2 ** 0.5), (2, 0.9 * pn2 ** 0.5)):
        diff = _f(pn2) - _f(bias) * _f(bias)
        got = g + (_f(0.01) * torch.sign(diff) if nt == 1 else (_f(0.01) * (_f(2.0) * diff)) * p)
        r, b = norm_bias_ref(g, p, pn2, 0.01, bias, nt)
        assert within_bound(got, r, b)[0] <= 1.0, (nt, bias)
        assert within_bound(g - (got - g), r, b)[0] > 1.0, (nt, bias)              # the wrong sign


# ----------------------------------------------------------------------------------------------------------------------------------
# BatchNorm running statistics (helpers.bn_running_ref, used by tests/test_gpu_running_stats.py) and the evaluation coefficients (helpers.
# bn_eval_coeffs_ref + the walk's tensor bounds, used by tests/test_gpu_eval.py): an fp32 torch emulation of bn_running_update_kernel /
# bn_eval_coeffs_kernel passes, every planted error fails.
RS_CH, RS_CHUNKS, RS_CHUNK, RS_VALID, RS_HW = 200, 5, 32, 30, 16


def _running_f32(rm0, rv0, mean_tab, var_tab, unbias, n_chunks, n_passes, order="chunk-major", momentum=0.1, drop=None, biased=False, decay_new=False):
    """bn_running_update_kernel in fp32 torch: for g: for p: m = keep m + mom mean[p, g]; v = keep v + mom (var[p, g] ub).  The switches plant the errors."""
    mom = _f(momentum)
    keep = _f(1.0) - mom
    m, v = rm0.clone(), rv0.clone()
    steps = [(p, g) for g in range(n_chunks) for p in range(n_passes)] if order == "chunk-major" else [(p, g) for p in range(n_passes) for g in range(n_chunks)]
    for i, (p, g) in enumerate(steps):
        if drop == i:
            continue
        var = var_tab[p, g] if biased else var_tab[p, g] * unbias
        if decay_new:                                    # momentum applied to the OLD value: r = mom r + keep x
            m, v = mom * m + keep * mean_tab[p, g], mom * v + keep * var
        else:
            m, v = keep * m + mom * mean_tab[p, g], keep * v + mom * var
    return m, v


@pytest.fixture(scope="module")
def running_case():
    from tests.helpers import bessel, bn_running_ref
    gen = torch.Generator().manual_seed(3)
    rm0, rv0 = torch.randn(RS_CH, generator=gen), 0.5 + torch.rand(RS_CH, generator=gen)
    mean_tab = torch.randn(3, RS_CHUNKS, RS_CH, generator=gen) * 0.5
    var_tab = 0.2 + torch.rand(3, RS_CHUNKS, RS_CH, generator=gen)
    ub = bessel(RS_VALID, 4, 4)
    unbias = torch.full((RS_CH,), ub, dtype=F)
    refs = {}
    for n_passes in (1, 2, 3):
        ups = [(mean_tab[p, g], var_tab[p, g], ub) for g in range(RS_CHUNKS) for p in range(n_passes)]
        refs[n_passes] = bn_running_ref(rm0, rv0, ups)
    return rm0, rv0, mean_tab, var_tab, unbias, refs


@pytest.mark.parametrize("n_passes", [1, 2, 3])
def test_bn_running_ref_honest_fp32_passes(running_case, n_passes):
    rm0, rv0, mean_tab, var_tab, unbias, refs = running_case
    m, v = _running_f32(rm0, rv0, mean_tab, var_tab, unbias, RS_CHUNKS, n_passes)
    rm, rv, Bm, Bv = refs[n_passes]
    a, b = within_bound(m, rm, Bm)[0], within_bound(v, rv, Bv)[0]
    print(f"running statistics, {n_passes} pass(es): honest fp32 worst error/bound mean {a:.3f}, var {b:.3f}; bound / (u |r|) median "
          f"{float((Bm / (U32 * rm.abs())).median()):.1f} / {float((Bv / (U32 * rv.abs())).median()):.1f}")
    assert a <= 1.0 and b <= 1.0
    # the decay of the start value is visible: (1 - m)^K of it is still there
    K = RS_CHUNKS * n_passes
    assert float((rm - (0.9 ** K) * rm0.double()).abs().max()) > 1e-3 and 0.9 ** K > 0.2


def test_bn_running_ref_planted_errors_fail(running_case):
    from tests.helpers import bessel
    rm0, rv0, mean_tab, var_tab, unbias, refs = running_case

    def ratios(n_passes, **kw):
        m, v = _running_f32(rm0, rv0, mean_tab, var_tab, kw.pop("unbias", unbias), RS_CHUNKS, n_passes, **kw)
        rm, rv, Bm, Bv = refs[n_passes]
        return within_bound(m, rm, Bm)[0], within_bound(v, rv, Bv)[0]

    a, b = ratios(1, biased=True)                         # biased instead of unbiased variance: the mean cannot see it, the variance must
    assert a <= 1.0 and b > 1.0
    # the Bessel factor of the STORED chunk (32 images) instead of the real one (30): 1/511 against 1/479, 1.3e-4 relative
    a, b = ratios(1, unbias=torch.full((RS_CH,), bessel(RS_CHUNK, 4, 4), dtype=F))
    assert a <= 1.0 and b > 1.0
    assert all(r > 1.0 for r in ratios(2, order="pass-major"))      # pass-major instead of chunk-major order
    assert all(r <= 1.0 for r in ratios(1, order="pass-major"))     # (one pass: the two orders are the same)
    assert all(r > 1.0 for r in ratios(2, drop=0))                  # one update dropped: the oldest one, whose weight 0.9^9 is the smallest
    assert all(r > 1.0 for r in ratios(3, drop=14))
    assert all(r > 1.0 for r in ratios(1, decay_new=True))          # momentum 0.1 applied to the old value instead of the new


def _eval_bn_f32(x_nhwc, gamma, beta, rm, rv, eps, with_eps=True):
    """bn_eval_coeffs_kernel + the apply pass (y = max(x scale + shift, 0)) in fp32 torch"""
    sc = gamma * (_f(1.0) / torch.sqrt(rv + _f(eps) if with_eps else rv))
    sh = beta - rm * sc
    return sc, sh, torch.relu(x_nhwc * sc + sh)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_eval_coefficient_without_eps_fails_the_walk_bounds(bf16):
    """The evaluation walk's tensor bounds (tests/test_gpu_bf16_structural._Checks: REL_L2 / REL_L2_F32, 2 ulp on all but BAD_FRACTION) and the
    coefficient bound of helpers.bn_eval_coeffs_ref: an honest fp32 emulation passes both, rsqrt(var) without eps fails both -- on the two
    epsilon-path channels (running_var 0: inf; 1e-6: a factor 3.3), two of 64."""
    from oracle import fb_oracle as orc
    from tests.helpers import BN_EPS, bn_eval_coeffs_ref
    from tests.test_gpu_bf16_structural import _Checks

    gen = torch.Generator().manual_seed(9)
    C, c0, c1 = 64, 3, 61
    x = torch.randn(6, C, 8, 8, generator=gen, dtype=torch.float64)
    x[:, c0] *= 1e-4
    x[:, c1] *= 1e-3
    q = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if bf16 else (lambda t: t.to(F).to(t.dtype))
    x = q(x)
    gamma, beta = (0.5 + torch.rand(C, generator=gen)).double(), (0.1 * torch.randn(C, generator=gen)).double()
    rm, rv = x.mean((0, 2, 3)).float().double(), x.var((0, 2, 3)).float().double()
    rv[c0], rv[c1] = 0.0, float(np.float32(1e-6))
    buffers = {"bn.running_mean": rm, "bn.running_var": rv}
    ref = q(torch.relu(orc.bn_eval_fwd(x, gamma, beta, buffers, "bn")))
    sc64, sh64, bsc, bsh = bn_eval_coeffs_ref(gamma, beta, rm, rv, BN_EPS)
    for with_eps in (True, False):
        sc, sh, y = _eval_bn_f32(x.permute(0, 2, 3, 1).float(), gamma.float(), beta.float(), rm.float(), rv.float(), BN_EPS, with_eps)
        ck = _Checks(fp32=not bf16)
        ck.close(y.to(torch.bfloat16) if bf16 else y, ref, "BN + ReLU, eval coefficients")
        coef = max(within_bound(sc, sc64, bsc)[0], within_bound(sh, sh64, bsh)[0])
        print(f"{'bf16' if bf16 else 'fp32'}, eps {'kept' if with_eps else 'dropped'}: {ck.report[0]}, coefficients error/bound {coef:.3g}")
        if with_eps:
            honest = y
            assert not ck.fails and coef <= 1.0
        else:
            assert ck.fails and coef > 1.0
            assert bool(((sc.double() - sc64).abs() > bsc)[[c0, c1]].all())
            if bf16:                                     # (the other channels are 5e-6 off: below a bf16 ulp, only the coefficient bound sees them)
                y[..., [c0, c1]] = honest[..., [c0, c1]]
                ck = _Checks(fp32=False)
                ck.close(y.to(torch.bfloat16), ref, "BN + ReLU, eps dropped on the ordinary channels only")
                assert not ck.fails
