"""The second half of a step -- everything csrc/multi_tensor.hip does to the per-chunk gradients once they are in the arena -- against float64 at
the sizes the benchmark runs: n = 11 173 962 (ResNet-18 / CIFAR-10; n % 4 == 2, so the scalar tails run), groups of 98 rows whose stride is n
rounded up to 64 (rows 48 and 96 straddle bytes 2^31 and 2^32 of the buffer) and of 13 rows (one full pass of 8 + 5), the single-vector kernels
also at n = 60 192 808 (ResNet-152 / ImageNet) and at 4096*256 + 1 and 1024*1024 + 3 around the launch caps.  Every grid-stride loop iterates
11 - 230 times per thread here; tests/test_gpu_ops.py never takes the second iteration.

References: the same formula in float64 on the device with plain torch ops, one row at a time, from the same fp32 inputs, host scalars rounded
to fp32; device scalars a kernel consumes (gnorm2, sq, vnorm2, pnorm2) are written by the test from a float64 reduction of the inputs.  Bounds:
elementwise, u = 2^-24 times the terms of the expression times the roundings on the longest path (tests/helpers.py; shown to bite by
tests/test_cpu_bounds.py); reductions relative, 1e-5 at n = 11 173 962 and (r iters + 16) u elsewhere.  Every case prints its worst
error/bound ratio.  fb_mt_ema and fb_mt_grad_noise are specified bit for bit against the fp32 torch expression evaluated ON THE DEVICE (one
torch kernel per operation: no contraction)."""
import gc
import math

import numpy as np
import pytest
import torch

from tests.helpers import (COEF_ROUNDINGS, SENTINEL, U32, clip_coef_ref, distinct_rows, f32r, fd_combine_ref, fd_perturb_ref,
                           make_data, norm_bias_ref, padding_untouched, reduction_bound, running_mean_ref, sam_ref, scale_ref, sgd_ref, within_bound)

pytestmark = pytest.mark.gpu

N18, N152 = 11_173_962, 60_192_808
STRIDE = (N18 + 63) // 64 * 64
N_SINGLE = [N18, N152, 4096 * 256 + 1, 1024 * 1024 + 3]
PAD = 64
RED_TOL = 1e-5                      # the project's bound for the norms at ResNet-18 size (>= the formula there: tests/test_cpu_bounds.py)

DECLARED, EXERCISED, RAN = {}, {}, set()
_current = [None]


def exercises(*names):
    def deco(fn):
        DECLARED[fn.__name__] = set(names)
        return fn
    return deco


@pytest.fixture(autouse=True)
def _track(request):
    gc.collect()
    torch.cuda.empty_cache()
    _current[0] = request.node.originalname
    yield
    RAN.add(_current[0])
    _current[0] = None
    gc.collect()
    torch.cuda.empty_cache()


def mt(name, *args, n):
    """One library call; counted as exercised at production size when its vector length is >= N18."""
    from fullbatchtraining_amd import lib
    lib.call(name, *args)
    if n >= N18:
        EXERCISED.setdefault(_current[0], set()).add(name)


def report(case, ratio, where=None):
    print(f"[update-production] {case}: worst error/bound {ratio:.3f}" + ("" if where is None else f" at {where}"))
    assert ratio <= 1.0, (case, ratio, where)


def report_rel(case, got, ref, bound):
    rel = float(((got.double() - ref).abs() / ref.abs()).max())
    report(case, rel / bound)


def f32_of(x64):
    """A float64 device scalar / vector rounded to fp32 (what the test writes where a kernel consumes a device scalar)."""
    return x64.to(torch.float32)


def vec(n, scale, seed, pad=PAD):
    """[n + pad] fp32: distinct_rows' recipe for one row, SENTINEL behind the n values."""
    return distinct_rows(1, n, n + pad, scale, seed, "cuda")[0]


def ws_for(G):
    from fullbatchtraining_amd import lib
    return torch.zeros(lib.load().fb_ws_mt_floats(int(G)), device="cuda")


def rows_worst(G, fn):
    """max over rows of fn(j) -> (ratio, index)."""
    worst, where = 0.0, None
    for j in range(G):
        r, i = fn(j)
        if not r <= worst:
            worst, where = r, (j, i)
    return worst, where


def assert_straddles(buf):
    """Rows 48 and 96 of a 98-row group hold bytes 2^31 and 2^32 of the buffer."""
    for row, byte in ((48, 2 ** 31), (96, 2 ** 32)):
        lo = buf[row].data_ptr() - buf.data_ptr()
        assert lo < byte < lo + 4 * buf.shape[1], (row, lo)


def blocks4(n):
    return max(1, min((n // 4 + 255) // 256, 1024))


def blocks1(n, cap):
    return max(1, min((n + 255) // 256, cap))


def tol4(n):        # float4 reductions (8 roundings per float4 and accumulator; + the scalar tail added by one thread)
    return RED_TOL if n == N18 else reduction_bound(n // 4, blocks4(n), 8, extra=8 * U32)


def tol1(n):        # scalar reductions (a product and a sum per element), FB_MT_BLOCKS workgroups at most
    return RED_TOL if n == N18 else reduction_bound(n, blocks1(n, 1024), 2)


# ------------------------------------------------------------------------------------------------------------------ group kernels --
@exercises("fb_mt_accumulate")
@pytest.mark.parametrize("G,c0", [(98, 0), (98, 292), (13, 292)])
def test_running_mean_and_chunk_norms(G, c0):
    n = N18
    g = distinct_rows(G, n, STRIDE, 1e-2, 100 + G, "cuda")
    if G == 98:
        assert_straddles(g)
    a0, ws = vec(n, 1e-2, 7), ws_for(G)
    ref, B, total = running_mean_ref(a0[:n], (g[j, :n] for j in range(G)), c0)
    closed = (c0 * a0[:n].double() + total) / (c0 + G)
    assert float((ref - closed).abs().max()) <= 1e-13 * max(1.0, float(closed.abs().max()))
    del closed, total
    sq64 = torch.stack([g[j, :n].double().pow(2).sum() for j in range(G)])
    avg, sq = a0.clone(), torch.zeros(G, device="cuda")
    mt("fb_mt_accumulate", avg.data_ptr(), g.data_ptr(), STRIDE, G, n, c0, sq.data_ptr(), ws.data_ptr(), n=n)
    report(f"fb_mt_accumulate G={G} c0={c0} mean", *within_bound(avg[:n], ref, B))
    report_rel(f"fb_mt_accumulate G={G} c0={c0} chunk norms", sq, sq64, tol4(n))
    assert padding_untouched(avg, n) and padding_untouched(g, n)
    avg2 = a0.clone()
    mt("fb_mt_accumulate", avg2.data_ptr(), g.data_ptr(), STRIDE, G, n, c0, None, ws.data_ptr(), n=n)
    assert torch.equal(avg2, avg)                                    # the pass without the norms: the same bits


@exercises("fb_mt_sqnorm", "fb_absmax")
def test_group_sqnorm_and_absmax():
    n, G = N18, 98
    g = distinct_rows(G, n, STRIDE, 1e-2, 211, "cuda")
    pre, ws = vec(n, 1e-2, 8), ws_for(G)
    for Gk in (98, 13):
        for scale, add, add_scale in ((1.0, None, 0.0), (0.5, pre, 0.3)):
            out = torch.zeros(Gk, device="cuda")
            mt("fb_mt_sqnorm", g.data_ptr(), STRIDE, Gk, n, scale, None if add is None else add.data_ptr(), add_scale, out.data_ptr(), ws.data_ptr(), n=n)
            ref = torch.stack([(f32r(scale) * g[j, :n].double() + (f32r(add_scale) * add[:n].double() if add is not None else 0.0)).pow(2).sum()
                               for j in range(Gk)])
            report_rel(f"fb_mt_sqnorm G={Gk} scale={scale} add={'yes' if add is not None else 'no'}", out, ref, tol4(n))
    # fb_absmax: exact.  98 sets a stride apart, per set and shared; the maximum planted in the last set's last element; the per-set launch
    # takes the blocks * n_sets > 8192 cap (1364 blocks per set otherwise)
    assert (n // 4 + 2047) // 2048 * G > 8192
    g[G - 1, n - 1] = -4321.5
    want = g[:, :n].abs().amax(1)
    assert float(want[G - 1]) == 4321.5
    out = torch.full((G,), -1.0, device="cuda")
    mt("fb_absmax", g.data_ptr(), n, G, STRIDE, 1, out.data_ptr(), n=n)
    assert torch.equal(out, want)
    one = torch.full((1,), -1.0, device="cuda")
    mt("fb_absmax", g.data_ptr(), n, G, STRIDE, 0, one.data_ptr(), n=n)
    assert float(one) == 4321.5
    # an unaligned slice start (pointer + 4 bytes): the scalar path; the slices are [1, n) of every row
    out.fill_(-1.0)
    mt("fb_absmax", g.data_ptr() + 4, n - 1, G, STRIDE, 1, out.data_ptr(), n=n)
    assert torch.equal(out, g[:, 1:n].abs().amax(1))
    print("[update-production] fb_absmax 98 sets per set / shared / unaligned: exact")


@exercises("fb_mt_fd_perturb")
@pytest.mark.parametrize("G", [98, 13])
def test_fd_perturb(G):
    n, eps = N18, 1e-2
    g = distinct_rows(G, n, STRIDE, 1e-2, 300 + G, "cuda")
    theta0, pre = vec(n, 1.0, 9), vec(n, 1e-2, 10)
    out = torch.full((G, STRIDE), SENTINEL, device="cuda")
    if G == 98:
        assert_straddles(out)
    for sign, s, p, acc in ((1.0, 0.5, None, 0.0), (-0.5, 0.5, pre, 0.3)):
        v2 = f32_of(torch.stack([(f32r(s) * g[j, :n].double() + (f32r(acc) * p[:n].double() if p is not None else 0.0)).pow(2).sum() for j in range(G)]))
        eps_n = torch.zeros(G, device="cuda")
        mt("fb_mt_fd_perturb", theta0.data_ptr(), g.data_ptr(), STRIDE, G, n, s, eps, sign, v2.data_ptr(), eps_n.data_ptr(),
           None if p is None else p.data_ptr(), acc, out.data_ptr(), n=n)
        eps64 = f32r(eps) / v2.double().sqrt()
        report(f"fb_mt_fd_perturb G={G} sign={sign} eps_n", *within_bound(eps_n, eps64, COEF_ROUNDINGS * U32 * eps64))
        worst, where = rows_worst(G, lambda j: within_bound(out[j, :n], *fd_perturb_ref(theta0[:n], g[j, :n], s, sign * float(eps64[j]),
                                                                                             None if p is None else p[:n], acc)))
        report(f"fb_mt_fd_perturb G={G} sign={sign} acc={acc}", worst, where)
        assert padding_untouched(out, n) and padding_untouched(theta0, n)


def _separate_clip(norms):
    """A clip value about which half of the rows clip, and the rows (indices, factors) to rescale so that every norm is at least 1 % away."""
    clip = float(norms.median())
    near = ((norms / clip - 1.0).abs() < 0.02).nonzero().flatten().tolist()
    return clip, [(j, 1.05 if float(norms[j]) >= clip else 0.95) for j in near]


@exercises("fb_mt_fd_combine_accumulate", "fb_mt_fd_combine", "fb_mt_chunk_clip")
@pytest.mark.parametrize("G,c0,central", [(98, 0, False), (98, 292, True), (13, 292, False)])
def test_fd_recombination_and_chunk_clip(G, c0, central):
    n, cf = N18, 0.1 / 4
    gen = torch.Generator(device="cuda").manual_seed(17)
    g = distinct_rows(G, n, STRIDE, 1e-2, 400 + G, "cuda")
    ga = torch.empty_like(g).normal_(generator=gen).mul_(1e-4).add_(g)
    ga[:, n:] = SENTINEL
    if central:
        gb = torch.empty_like(g).normal_(generator=gen).mul_(-1e-4).add_(g)
        gb[:, n:] = SENTINEL
    else:
        gb = g
    eps = torch.linspace(1e-3, 1.1e-2, G, device="cuda")            # distinct per row: a row mix-up changes the result
    a0 = vec(n, 1e-2, 12)

    def refs():
        for j in range(G):
            yield fd_combine_ref(g[j, :n], ga[j, :n], gb[j, :n], float(eps[j]), cf)

    ref, B, _ = running_mean_ref(a0[:n], refs(), c0)
    avg = a0.clone()
    mt("fb_mt_fd_combine_accumulate", avg.data_ptr(), g.data_ptr(), ga.data_ptr(), gb.data_ptr(), STRIDE, G, n, eps.data_ptr(), cf, c0, n=n)
    report(f"fb_mt_fd_combine_accumulate G={G} c0={c0} central={central}", *within_bound(avg[:n], ref, B))
    assert padding_untouched(avg, n) and padding_untouched(g, n)
    del ref, B
    # the two-step form: in place (gb aliases g in the forward variant, as in the engine)
    work = g.clone()
    mt("fb_mt_fd_combine", work.data_ptr(), ga.data_ptr(), (work if not central else gb).data_ptr(), STRIDE, G, n, eps.data_ptr(), cf, n=n)
    worst, where = rows_worst(G, lambda j: within_bound(work[j, :n], *fd_combine_ref(g[j, :n], ga[j, :n], gb[j, :n], float(eps[j]), cf)))
    report(f"fb_mt_fd_combine G={G} central={central}", worst, where)
    assert padding_untouched(work, n)
    del ga
    # per-chunk clip of what is in the buffer now: sq written by the test from float64 norms of that content
    norms = torch.stack([work[j, :n].double().pow(2).sum() for j in range(G)]).sqrt()
    clip, fix = _separate_clip(norms)
    for j, f in fix:
        work[j, :n] *= f
    sq64 = torch.stack([work[j, :n].double().pow(2).sum() for j in range(G)])
    sq, norms = f32_of(sq64), sq64.sqrt()
    assert float((norms / clip - 1.0).abs().min()) >= 0.01
    for name, c in (("half", clip), ("all", 0.5 * float(norms.min())), ("none", 2.0 * float(norms.max()))):
        buf, flags = work.clone(), torch.full((G,), -1.0, device="cuda")
        mt("fb_mt_chunk_clip", buf.data_ptr(), STRIDE, G, n, sq.data_ptr(), c, flags.data_ptr(), n=n)
        hits = [clip_coef_ref(float(sq[j]), c) for j in range(G)]
        assert flags.tolist() == [1.0 if h else 0.0 for _, h in hits]
        n_hit = sum(h for _, h in hits)
        assert n_hit == {"all": G, "none": 0}.get(name, n_hit) and (name != "half" or G // 3 <= n_hit <= G - G // 3)

        def row(j):
            coef, hit = hits[j]
            r = work[j, :n].double() * coef
            return within_bound(buf[j, :n], r, (1 + COEF_ROUNDINGS) * U32 * r.abs() if hit else 0.0)
        worst, where = rows_worst(G, row)
        report(f"fb_mt_chunk_clip G={G} {name} ({n_hit} rows clip)", worst, where)
        assert padding_untouched(buf, n)
        del buf
    mt("fb_mt_chunk_clip", work.data_ptr(), STRIDE, G, n, sq.data_ptr(), 2.0 * float(norms.max()), None, n=n)          # no flags wanted


# ---------------------------------------------------------------------------------------------------------- single-vector kernels --
@exercises("fb_mt_norms2", "fb_mt_absmax2", "fb_mt_pnorm2", "fb_mt_sqnorm", "fb_absmax", "fb_mt_accumulate")
@pytest.mark.parametrize("n", N_SINGLE)
def test_vector_reductions_and_means(n):
    a, b, ws = vec(n, 1e-2, 31), vec(n, 1.0, 32), ws_for(2)
    a64, b64 = a[:n].double(), b[:n].double()
    out = torch.full((2,), -1.0, device="cuda")
    mt("fb_mt_norms2", a.data_ptr(), b.data_ptr(), n, out.data_ptr(), ws.data_ptr(), n=n)
    report_rel(f"fb_mt_norms2 n={n} both slots", out, torch.stack([a64.pow(2).sum(), b64.pow(2).sum()]), tol1(n))
    out.fill_(-1.0)
    mt("fb_mt_norms2", b.data_ptr(), None, n, out.data_ptr(), ws.data_ptr(), n=n)
    report_rel(f"fb_mt_norms2 n={n} b=NULL", out[:1], b64.pow(2).sum().reshape(1), tol1(n))
    assert float(out[1]) == 0.0
    for x, nm in ((a, "a"), (b, "b")):
        one = torch.full((1,), -1.0, device="cuda")
        mt("fb_mt_sqnorm", x.data_ptr(), (n + 63) // 64 * 64, 1, n, 1.0, None, 0.0, one.data_ptr(), ws.data_ptr(), n=n)
        report_rel(f"fb_mt_sqnorm n={n} one row ({nm})", one, x[:n].double().pow(2).sum().reshape(1), tol4(n))
    for p in (1.0, 1.5, 3.0):
        one = torch.full((1,), -1.0, device="cuda")
        mt("fb_mt_pnorm2", a.data_ptr(), n, p, one.data_ptr(), ws.data_ptr(), n=n)
        ref = a64.abs().pow(p).sum().pow(2.0 / p).reshape(1)
        report_rel(f"fb_mt_pnorm2 n={n} p={p}", one, ref, (2.0 / p) * (tol1(n) + (0.0 if p == 1.0 else 4 * U32)) + 2 * U32)
    # L-infinity: exact, the extreme at index 0, at the last index, in the last n % 4 elements, at the first element of the second grid-stride pass
    grid = blocks1(n, 1024)
    assert grid * 256 < n
    for pos in (None, 0, n - 1, n - 2, grid * 256):
        x = a.clone()
        if pos is not None:
            x[pos] = -123.456
        m = x[:n].abs().max()
        assert pos is None or float(m) == f32r(123.456)
        one = torch.full((1,), -1.0, device="cuda")
        mt("fb_mt_absmax2", x.data_ptr(), n, one.data_ptr(), ws.data_ptr(), n=n)
        assert float(one) == float(m * m), (pos, float(one), float(m * m))
        one.fill_(-1.0)
        mt("fb_absmax", x.data_ptr(), n, 1, 0, 0, one.data_ptr(), n=n)
        assert float(one) == float(m), pos
        one.fill_(-1.0)
        mt("fb_absmax", x.data_ptr() + 4, n - 1, 1, 0, 1, one.data_ptr(), n=n)
        assert float(one) == float(x[1:n].abs().max()), pos
    print(f"[update-production] fb_mt_absmax2 / fb_absmax n={n}: exact at 4 planted positions")
    # the running mean of two rows at this length
    stride = (n + 63) // 64 * 64
    g = distinct_rows(2, n, stride, 1e-2, 33, "cuda")
    ws8 = ws_for(8)
    ref, B, _ = running_mean_ref(a[:n], (g[j, :n] for j in range(2)), 292)
    avg, sq = a.clone(), torch.zeros(2, device="cuda")
    mt("fb_mt_accumulate", avg.data_ptr(), g.data_ptr(), stride, 2, n, 292, sq.data_ptr(), ws8.data_ptr(), n=n)
    report(f"fb_mt_accumulate n={n} G=2 mean", *within_bound(avg[:n], ref, B))
    report_rel(f"fb_mt_accumulate n={n} G=2 chunk norms", sq, torch.stack([g[j, :n].double().pow(2).sum() for j in range(2)]), tol4(n))
    assert padding_untouched(avg, n)


SGD_CASES = [  # first, nesterov, dampening, momentum, clip
    (1, 1, 0.0, 0.9, None), (0, 1, 0.0, 0.9, None), (0, 0, 0.0, 0.9, "miss"), (0, 0, 0.1, 0.9, "hit"), (0, 1, 0.1, 0.9, "hit"), (1, 1, 0.0, 0.9, "hit"),
    (0, 1, 0.0, 0.0, "hit"), (0, 0, 0.0, 0.0, None)]


@exercises("fb_mt_clip_sgd")
@pytest.mark.parametrize("n", N_SINGLE)
def test_clip_sgd(n):
    lr, wd = 0.1, 5e-4
    p0, g0, m0 = vec(n, 1.0, 41), vec(n, 1e-2, 42), vec(n, 1e-2, 43)
    norm2 = f32_of(g0[:n].double().pow(2).sum().reshape(1))
    norm = float(norm2) ** 0.5
    for first, nesterov, damp, mu, clip in SGD_CASES:
        clipv = None if clip is None else (0.5 * norm if clip == "hit" else 2.0 * norm)
        coef, hit = clip_coef_ref(float(norm2), clipv)
        assert hit == (clip == "hit")
        p, g, m = p0.clone(), g0.clone(), (m0.clone() if mu else None)
        mt("fb_mt_clip_sgd", p.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(), n, norm2.data_ptr() if clip is not None else None,
           -1.0 if clipv is None else clipv, lr, wd, mu, damp, nesterov, first, n=n)
        ref = sgd_ref(p0[:n], g0[:n], m0[:n], coef, hit, lr, wd, mu, damp, nesterov, first)
        got = {"grad": g, "param": p, **({"mom": m} if mu else {})}
        assert set(got) == set(ref)
        for k, t in got.items():
            report(f"fb_mt_clip_sgd n={n} first={first} nesterov={nesterov} damp={damp} mu={mu} clip={clip}: {k}", *within_bound(t[:n], *ref[k]))
            assert padding_untouched(t, n)


@exercises("fb_mt_sam_ascent", "fb_mt_sam_restore", "fb_mt_clip_scale", "fb_mt_scale", "fb_mt_norm_bias", "fb_mt_ema", "fb_mt_grad_noise")
@pytest.mark.parametrize("n", N_SINGLE)
def test_elementwise_options(n):
    t0, g0, x0 = vec(n, 1.0, 51), vec(n, 1e-2, 52), vec(n, 1.0, 53)
    norm2 = f32_of(g0[:n].double().pow(2).sum().reshape(1))
    norm = float(norm2) ** 0.5
    for clip in (None, 0.5 * norm, 2.0 * norm):
        ref = sam_ref(t0[:n], g0[:n], float(norm2), clip, 0.05)
        assert ref["hit"] == (clip is not None and clip < norm)
        # the kernel's |g_c| = sqrt(norm2) * coef against the float64 norm of the clipped vector: the product, sqrt, and the allowance on coef
        assert abs(float(np.sqrt(np.float64(float(norm2)))) * ref["coef"] - ref["norm_c"]) <= 4 * U32 * ref["norm_c"]
        t, e = t0.clone(), torch.full_like(t0, SENTINEL)
        mt("fb_mt_sam_ascent", t.data_ptr(), g0.data_ptr(), e.data_ptr(), n, norm2.data_ptr(), -1.0 if clip is None else clip, 0.05, n=n)
        tag = "off" if clip is None else ("hit" if ref["hit"] else "miss")
        report(f"fb_mt_sam_ascent n={n} clip {tag}: e_w", *within_bound(e[:n], *ref["e"]))
        report(f"fb_mt_sam_ascent n={n} clip {tag}: theta", *within_bound(t[:n], *ref["theta"]))
        back = t[:n].double() - e[:n].double()
        mt("fb_mt_sam_restore", t.data_ptr(), e.data_ptr(), n, n=n)
        report(f"fb_mt_sam_restore n={n} clip {tag}", *within_bound(t[:n], back, U32 * back.abs()))
        assert padding_untouched(t, n) and padding_untouched(e, n)
        # clip applied in place
        if clip is not None:
            g = g0.clone()
            mt("fb_mt_clip_scale", g.data_ptr(), n, norm2.data_ptr(), clip, n=n)
            r = g0[:n].double() * ref["coef"]
            report(f"fb_mt_clip_scale n={n} clip {tag}", *within_bound(g[:n], r, (1 + COEF_ROUNDINGS) * U32 * r.abs() if ref["hit"] else 0.0))
            assert padding_untouched(g, n)
    x = x0.clone()
    mt("fb_mt_scale", x.data_ptr(), n, 0.9, n=n)
    report(f"fb_mt_scale n={n}", *within_bound(x[:n], *scale_ref(x0[:n], 0.9)))
    assert padding_untouched(x, n)
    pn2 = f32_of(t0[:n].double().pow(2).sum().reshape(1))
    for nt, rel_bias in ((1, 0.9), (1, 1.1), (2, 0.9), (2, 1.1)):
        bias = rel_bias * float(pn2) ** 0.5
        g = g0.clone()
        mt("fb_mt_norm_bias", g.data_ptr(), t0.data_ptr(), n, pn2.data_ptr(), 0.01, bias, nt, n=n)
        report(f"fb_mt_norm_bias n={n} type {nt} bias {rel_bias} |theta|", *within_bound(g[:n], *norm_bias_ref(g0[:n], t0[:n], float(pn2), 0.01, bias, nt)))
        assert padding_untouched(g, n)
    # bit for bit against the fp32 torch expression on the device (each torch operation is a kernel of its own: two roundings and an add)
    m, om = 0.99, float(1 - 0.99)
    ema = x0.clone()
    mt("fb_mt_ema", ema.data_ptr(), t0.data_ptr(), n, m, om, n=n)
    assert torch.equal(ema[:n], (x0[:n] * m) + (t0[:n] * om)) and padding_untouched(ema, n)
    for mode, strength in ((0, 0.01), (1, 0.1)):
        g = g0.clone()
        mt("fb_mt_grad_noise", g.data_ptr(), x0.data_ptr(), n, strength, mode, n=n)
        tn = x0[:n] * strength
        assert torch.equal(g[:n], g0[:n] + tn if mode == 0 else g0[:n] * (tn + 1.0)) and padding_untouched(g, n), mode
    print(f"[update-production] fb_mt_ema / fb_mt_grad_noise n={n}: the bits of the fp32 torch expression on the device")


# ------------------------------------------------------------------------------------------------- the engine, ResNet-18 plan --
def _engine(dtype, G, fd_sets=0, arena_align=None):
    from tests.test_gpu_engine import _build
    cfg, model, eng, stem_patches = _build(18, 32, 128, G, dtype, fd_sets=fd_sets)
    if arena_align is not None:
        from fullbatchtraining_amd.engine import Engine
        eng = Engine(model, 32, 128, G, compute_dtype=dtype, fd_sets=fd_sets, arena_align=arena_align)
    assert eng.plan.n_params == N18
    return eng, stem_patches


def _bucket_bound(eng, world):
    """parallel.exchange_bounds' rule: the start of the last stage rounded up to the shard granule lcm(4, world)."""
    granule = 4 * world // math.gcd(4, world)
    return (eng.plan.late_offset + granule - 1) // granule * granule


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_engine_fold_over_bucket_ranges(mode):
    """The running-mean fold of Engine.full_gradient (fb_mt_accumulate at arena offsets) over [0, b) and [b, P) for the bucket boundary of world sizes 2, 3
    and 8, counters 0 and 292, with and without the norms."""
    from fullbatchtraining_amd import lib
    G = 98
    eng, _ = _engine(torch.float32 if mode == "fp32" else torch.bfloat16, G)
    P = eng.plan.P
    eng.g[:G].copy_(distinct_rows(G, P, P, 1e-2, 61, "cuda"))
    assert_straddles(eng.g)
    g = eng.g
    a0 = vec(P, 1e-2, 62, pad=0)
    sq64_of = lambda lo, hi: torch.stack([g[j, lo:hi].double().pow(2).sum() for j in range(G)])
    bs = sorted({_bucket_bound(eng, w) for w in (2, 3, 8)})
    assert all(0 < b < P and b % 4 == 0 for b in bs)
    parts = {b: (sq64_of(0, b), sq64_of(b, P)) for b in bs}
    refs = {c0: running_mean_ref(a0, (g[j] for j in range(G)), c0)[:2] for c0 in (0, 292)}

    def fold(lo, hi, c0, sq_out):                        # (the call full_gradient makes for the arena range [lo, hi))
        lib.call("fb_mt_accumulate", eng.avg.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, P, G, hi - lo, c0, None if sq_out is None else sq_out.data_ptr(),
                 eng.mt_ws.data_ptr())

    for b in bs:
        for c0 in (0, 292):
            sq_lo, sq_hi = torch.zeros(G, device="cuda"), torch.zeros(G, device="cuda")
            eng.avg.copy_(a0)
            fold(0, b, c0, sq_lo)
            fold(b, P, c0, sq_hi)
            torch.cuda.synchronize()
            report(f"fold {mode} b={b} c0={c0} mean", *within_bound(eng.avg, *refs[c0]))
            report_rel(f"fold {mode} b={b} c0={c0} norms of [0,b)", sq_lo, parts[b][0], RED_TOL)
            report_rel(f"fold {mode} b={b} c0={c0} norms of [0,b)+[b,P)", sq_lo + sq_hi, parts[b][0] + parts[b][1], RED_TOL)
            with_sq = eng.avg.clone()
            eng.avg.copy_(a0)
            fold(0, b, c0, None)
            fold(b, P, c0, None)
            assert torch.equal(eng.avg, with_sq)


def _fill_state(eng, seed):
    P = eng.plan.P
    eng.theta.copy_(vec(P, 1.0, seed, pad=0))
    eng.avg.copy_(vec(P, 1e-2, seed + 1, pad=0))
    eng.mom.copy_(vec(P, 1e-2, seed + 2, pad=0))


def _tensor_ranges(eng):
    return [(name, eng.plan.offsets[name], math.prod(eng.plan.param_shapes[name])) for name in eng.plan.param_names]


def test_engine_per_tensor_update_and_norm_bias():
    """sgd_step_per_tensor (two steps, a weight decay per tensor, clip hit) and norm_bias (types 1 and 2) on the ResNet-18 plan against float64 per
    tensor; the arena's alignment padding between the tensors keeps its bits."""
    eng, _ = _engine(torch.bfloat16, 2)
    P, ranges = eng.plan.P, _tensor_ranges(eng)
    pad = torch.ones(P, dtype=torch.bool, device="cuda")
    for _, off, n in ranges:
        pad[off:off + n] = False
    assert int(pad.sum()) == P - N18 > 0
    _fill_state(eng, 71)
    lr, mu, damp = 0.1, 0.9, 0.0
    wds = [5e-4 * (1.0 + i / len(ranges)) for i in range(len(ranges))]
    eng.first_step = True
    for step in range(2):
        if step:
            eng.avg.copy_(vec(P, 1e-2, 75, pad=0))
        th0, g0, m0 = eng.theta.clone(), eng.avg.clone(), eng.mom.clone()
        n2 = sum(g0[off:off + n].double().pow(2).sum() for _, off, n in ranges)
        eng.norms2[0] = f32_of(n2)
        clip = 0.5 * float(n2) ** 0.5
        coef, hit = clip_coef_ref(float(eng.norms2[0]), clip)
        assert hit
        eng.sgd_step_per_tensor(lr, wds, mu, damp, True, grad_clip=clip)
        torch.cuda.synchronize()
        assert not eng.first_step
        worst = {}
        for (name, off, n), wd in zip(ranges, wds):
            sl = slice(off, off + n)
            ref = sgd_ref(th0[sl], g0[sl], m0[sl], coef, hit, lr, wd, mu, damp, True, step == 0)
            for k, t in (("grad", eng.avg), ("mom", eng.mom), ("param", eng.theta)):
                r, i = within_bound(t[sl], *ref[k])
                if not r <= worst.get(k, (0.0,))[0]:
                    worst[k] = (r, (name, i))
        for k, (r, where) in worst.items():
            report(f"sgd_step_per_tensor step {step}: {k}", r, where)
        for t, t0 in ((eng.theta, th0), (eng.avg, g0), (eng.mom, m0)):
            assert torch.equal(t[pad], t0[pad])
    for nt, rel_bias in ((1, 0.9), (2, 1.1)):
        th0, g0 = eng.theta.clone(), eng.avg.clone()
        pn2 = f32_of(sum(th0[off:off + n].double().pow(2).sum() for _, off, n in ranges))
        eng.norms2[1] = pn2
        bias = rel_bias * float(pn2) ** 0.5
        eng.norm_bias(0.01, nt, bias)
        torch.cuda.synchronize()
        worst, where = 0.0, None
        for name, off, n in ranges:
            r, i = within_bound(eng.avg[off:off + n], *norm_bias_ref(g0[off:off + n], th0[off:off + n], float(pn2), 0.01, bias, nt))
            if not r <= worst:
                worst, where = r, (name, i)
        report(f"norm_bias type {nt} per tensor", worst, where)
        assert torch.equal(eng.avg[pad], g0[pad]) and torch.equal(eng.theta, th0)


@pytest.mark.parametrize("world", [3, 8])
def test_engine_sharded_update_equals_the_whole_arena(world):
    """sgd_step(lo, n) over the ``world`` shard ranges of both buckets (parallel.BucketExchange.ranges with parallel.exchange_bounds' boundary)
    = one sgd_step over the whole arena, bit for bit (arena padded to lcm(64, world) as the trainer builds it)."""
    eng, _ = _engine(torch.bfloat16, 2, arena_align=math.lcm(64, world))
    P, b = eng.plan.P, _bucket_bound(eng, world)
    assert P % world == 0 and b % world == 0 and b % 4 == 0
    _fill_state(eng, 81)
    eng.norms2[0] = f32_of(eng.avg.double().pow(2).sum())
    clip = 0.5 * float(eng.norms2[0]) ** 0.5
    state = [t.clone() for t in (eng.theta, eng.avg, eng.mom)]
    eng.first_step = False
    eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True, grad_clip=clip)
    whole = [t.clone() for t in (eng.theta, eng.avg, eng.mom)]
    assert not torch.equal(whole[1], state[1])                     # the clip was applied
    for t, s in zip((eng.theta, eng.avg, eng.mom), state):
        t.copy_(s)
    for lo, hi in ((0, b), (b, P)):
        n = (hi - lo) // world
        for r in range(world):
            eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True, grad_clip=clip, lo=lo + r * n, n=n)
    torch.cuda.synchronize()
    for t, w in zip((eng.theta, eng.avg, eng.mom), whole):
        assert torch.equal(t, w)
    print(f"[update-production] sgd_step over {2 * world} shard ranges (world {world}, b={b}, P={P}): the bits of one launch")


@pytest.mark.parametrize("variant", ["forward", "central", "forward+acc", "forward+batch_clip"])
def test_engine_regularised_group(variant):
    """full_gradient on ONE fp32 group of 56 chunks (BASELINE config 3's group), block_strength 0.5, from counter0 = 0: what the engine still
    holds afterwards -- the raw gradients (g), the gradients at the perturbed parameters (g_fd), sq, vnorm2, eps_n, the LAST perturbed parameter
    sets (theta_k; central differences: the theta - eps/2 v sets, the theta + eps/2 v sets are overwritten) and avg -- recombined in float64 with
    the formulas of oracle/fb_oracle.py::gradreg: this checks the wiring (which buffer, which sign, which cf, which counter) at production
    size, not the convolutions.  'forward+acc': also the pre-pass mean (eng.pre) from the raw gradients -- the pre-pass evaluates the same
    gradients.  'forward+batch_clip': fb_mt_fd_combine overwrites g in place, so the recombination itself cannot be rechecked from inputs;
    checked are the clip decisions against the float64 norms the engine left in vnorm2's place, the clipped rows' norms, and avg = the mean of
    the rows the arena holds.  Not checked anywhere here: the plus-side parameter sets of central differences, and the raw gradients of the
    batch_clip variant (both overwritten by the time the call returns)."""
    G, lr, bs, eps = 56, 0.1, 0.5, 1e-2
    central, acc, clipped = variant == "central", 0.3 if variant == "forward+acc" else 0.0, variant == "forward+batch_clip"
    eng, stem_patches = _engine(torch.float32, G, fd_sets=2 if central else 1)
    P = eng.plan.P
    x, y = make_data(128 * G, 32, seed=77)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.float32), y.cuda()
    kw = dict(block_strength=bs, eps=eps, implementation="central-differences" if central else "forward-differences", counter0=0, acc_strength=acc)
    _, _, sq_all = eng.full_gradient(patches, yd, lr, **kw)
    torch.cuda.synchronize()
    g, ga = eng.g, eng.g_fd[0]
    gb = eng.g_fd[1] if central else g
    pre = eng.pre if acc else None
    assert torch.equal(sq_all, eng.sq[:G])
    report_rel(f"full_gradient {variant}: sq", eng.sq[:G], torch.stack([g[j].double().pow(2).sum() for j in range(G)]), RED_TOL)
    v2 = torch.stack([(f32r(bs) * g[j].double() + (f32r(acc) * pre.double() if acc else 0.0)).pow(2).sum() for j in range(G)])
    report_rel(f"full_gradient {variant}: vnorm2", eng.vnorm2[:G], v2, RED_TOL)
    eps64 = f32r(eps) / eng.vnorm2[:G].double().sqrt()
    report(f"full_gradient {variant}: eps_n", *within_bound(eng.eps_n[:G], eps64, COEF_ROUNDINGS * U32 * eps64))
    sign = -0.5 if central else 1.0
    worst, where = rows_worst(G, lambda j: within_bound(eng.theta_k[j], *fd_perturb_ref(eng.theta, g[j], bs, sign * float(eps64[j]), pre, acc)))
    report(f"full_gradient {variant}: perturbed parameters (sign {sign})", worst, where)

    def refs():
        for j in range(G):
            yield fd_combine_ref(g[j], ga[j], gb[j], float(eng.eps_n[j]), lr / 4)

    ref, B, _ = running_mean_ref(torch.zeros(P, device="cuda"), refs(), 0)
    report(f"full_gradient {variant}: avg", *within_bound(eng.avg, ref, B))
    if acc:
        ref, B, _ = running_mean_ref(torch.zeros(P, device="cuda"), (g[j] for j in range(G)), 0)
        report(f"full_gradient {variant}: pre-pass mean", *within_bound(eng.pre, ref, B))
    if not clipped:
        return
    # the same group with every regularised chunk gradient clipped to a norm about which half of them lie
    norms = torch.stack([fd_combine_ref(g[j], ga[j], gb[j], float(eng.eps_n[j]), lr / 4)[0].pow(2).sum() for j in range(G)]).sqrt()
    clip = float(norms.median())
    raw_sq = eng.sq[:G].clone()
    eng.full_gradient(patches, yd, lr, batch_clip=clip, **kw)
    torch.cuda.synchronize()
    assert torch.equal(eng.sq[:G], raw_sq)
    report_rel(f"full_gradient {variant}: norms of the regularised gradients", eng.vnorm2[:G], norms.pow(2), RED_TOL)
    sure = (norms / clip - 1.0).abs() > 1e-4
    assert int(sure.sum()) >= G - 2
    assert torch.equal(eng.clipped[:G][sure], (norms > clip).float()[sure]) and torch.equal(eng.clipped_all, eng.clipped[:G])
    assert G // 3 <= int(eng.clipped[:G].sum()) <= G - G // 3
    after = torch.stack([g[j].double().pow(2).sum() for j in range(G)]).sqrt()
    want = torch.where(eng.clipped[:G] > 0, clip * norms / (norms + 1e-6), norms)
    report_rel(f"full_gradient {variant}: row norms after the clip", after, want, RED_TOL)
    ref, B, _ = running_mean_ref(torch.zeros(P, device="cuda"), (g[j] for j in range(G)), 0)
    report(f"full_gradient {variant}: avg = mean of the clipped rows", *within_bound(eng.avg, ref, B))


def test_every_update_entry_point_is_exercised_at_production_size():
    """Every fb_mt_* entry point of the library's signature table and fb_absmax is declared by a case of this file, and every case that ran in
    this session did call what it declares with n >= 11 173 962."""
    from fullbatchtraining_amd import lib
    names = {k for k in lib._SIGS if k.startswith("fb_mt_")} | {"fb_absmax"}
    declared = set().union(*DECLARED.values())
    assert declared == names, (names - declared, declared - names)
    for test in RAN & set(DECLARED):
        assert EXERCISED.get(test, set()) >= DECLARED[test], (test, DECLARED[test] - EXERCISED.get(test, set()))
