"""``fb_mt_wolfe_direction`` / ``fb_mt_wolfe_trial`` / ``fb_mt_wolfe_phi_grad`` (csrc/wolfe.hip) against the float64 restatement of
tests/wolfe_ref.py, whose module docstring derives every bound used here:

  * elementwise |d mom|, |d p|, |d theta| <= k u (sum of the magnitudes of the terms), k counted from the roundings of the expression;
  * the reductions |d phi'| <= c u sum S_d,i S_p,i with c = (the lane's chain of fused multiply-adds) + 6 (wave tree) + 3 (across waves) + 1 (final
    cast) + 1 (the rounding of d) (+ k_p for the direction, whose second factor is its own output): ``wolfe_ref.phi_c``, evaluated with the spans
    the LIBRARY reports (FB_WOLFE_VEC, FB_WOLFE_BLOCK, FB_MT_BLOCKS), as are the sizes:
  * n = 1; one short of / exactly / one past a lane's vector, a wave's span, a workgroup's span and the grid's span; one vector and one element
    past the grid's span (the stride loop runs twice and ends ragged); the ResNet-20 arena; once the arena of the benchmark (declared to
    tests/test_gpu_update_production.py through ``exercises``);
  * two launches give the same bits; the momentum has the bits ``fb_mt_clip_sgd`` writes for the same inputs without a clip; theta0 equals theta
    bit for bit; inputs and the SENTINEL columns behind n untouched; argument errors return their code without a launch."""
import numpy as np
import pytest
import torch

from tests import wolfe_ref
from tests.helpers import SENTINEL, padding_untouched, within_bound
from tests.test_gpu_update_production import N18, exercises

pytestmark = pytest.mark.gpu

FB_ERR_ARG = -1
PAD = 64
LR, ALPHAS = 0.07, (1.0, 0.3217)
#                 mu   damp  nesterov wd    first
CONFIGS = {
    "nesterov": (0.9, 0.0, True, 5e-4, False),
    "nesterov-first": (0.9, 0.0, True, 5e-4, True),
    "heavy-ball-damped": (0.9, 0.25, False, 5e-4, False),
    "no-momentum": (0.0, 0.0, False, 0.0, False),
    "no-momentum-decay": (0.0, 0.0, False, 1e-2, False),
}


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _spans():
    h = _lib().load()
    vec, block, blocks = (h.fb_abi_constant(k) for k in (b"FB_WOLFE_VEC", b"FB_WOLFE_BLOCK", b"FB_MT_BLOCKS"))
    assert vec > 0 and block > 0 and blocks > 0
    return vec, block, blocks


def _sizes():
    vec, block, blocks = _spans()
    spans = (vec, 64 * vec, block * vec, blocks * block * vec)
    return sorted({1} | {s + d for s in spans for d in (-1, 0, 1)} | {spans[-1] + vec + 1})


def _resnet20_arena():
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    return sum(p.numel() for p in construct_model(compose(["model=resnet20"]).model, 3, 10).parameters())


def _vec(n, gen, kind):
    t = torch.full((n + PAD,), SENTINEL, device="cuda", dtype=torch.float32)
    t[:n].normal_(generator=gen)
    if kind == "grad":          # magnitudes log-uniform over 1e-6 .. 1e2
        t[:n].mul_(torch.pow(10.0, torch.rand(n, device="cuda", generator=gen) * 8 - 6))
    elif kind == "param":
        t[:n].mul_(0.1)
    return t


def _inputs(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ops = dict(theta=_vec(n, gen, "param"), grad=_vec(n, gen, "grad"), mom=_vec(n, gen, "grad"), grad2=_vec(n, gen, "grad"))
    for k in ("p", "theta0"):
        ops[k] = torch.full((n + PAD,), SENTINEL, device="cuda", dtype=torch.float32)
    ops["out"], ops["ws"] = torch.full((2,), SENTINEL, device="cuda"), torch.zeros(_lib().load().fb_ws_mt_floats(1), device="cuda")
    return ops


def _direction(ops, n, cfg, out_slot=0):
    mu, damp, nesterov, wd, first = cfg
    _lib().call("fb_mt_wolfe_direction", ops["theta"].data_ptr(), ops["grad"].data_ptr(), ops["mom"].data_ptr(), ops["p"].data_ptr(),
                ops["theta0"].data_ptr(), n, wd, mu, damp, 1 if nesterov else 0, 1 if first else 0, ops["out"].data_ptr() + 4 * out_slot,
                ops["ws"].data_ptr())


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(n, name, seed=0):
    mu, damp, nesterov, wd, first = cfg = CONFIGS[name]
    vec, block, blocks = _spans()
    ops = _inputs(n, seed)
    before = {k: v.clone() for k, v in ops.items()}
    _direction(ops, n, cfg)
    torch.cuda.synchronize()
    ref = wolfe_ref.direction_f64(before["theta"][:n], before["grad"][:n], before["mom"][:n], wd, mu, damp, nesterov, first)
    tag = f"[wolfe n={n} {name}]"
    # ---- direction: inputs, snapshot, momentum, p, phi'(0)
    assert _bits(ops["theta"], before["theta"]) and _bits(ops["grad"], before["grad"]), "theta / grad are read only"
    assert _bits(ops["theta0"][:n], before["theta"][:n]), "theta0 is theta, bit for bit"
    for k in ("p", "theta0", "mom"):
        assert padding_untouched(ops[k], n), k
    if mu == 0:
        assert _bits(ops["mom"], before["mom"]), "without momentum the buffer is not touched"
    else:
        ratio, where = within_bound(ops["mom"][:n], *ref["mom"])
        print(f"{tag} mom: worst error/bound {ratio:.3f} at {where}")
        assert ratio <= 1.0
        sgd = {k: before[k].clone() for k in ("theta", "grad", "mom")}
        _lib().call("fb_mt_clip_sgd", sgd["theta"].data_ptr(), sgd["grad"].data_ptr(), sgd["mom"].data_ptr(), n, None, -1.0, LR, wd, mu, damp,
                    1 if nesterov else 0, 1 if first else 0)
        torch.cuda.synchronize()
        diff = int((ops["mom"][:n].view(torch.int32) != sgd["mom"][:n].view(torch.int32)).sum())
        print(f"{tag} mom vs fb_mt_clip_sgd: {diff} of {n} elements differ in their bits")
        assert diff == 0
    ratio, where = within_bound(ops["p"][:n], *ref["p"])
    print(f"{tag} p: worst error/bound {ratio:.3f} at {where}")
    assert ratio <= 1.0
    c = wolfe_ref.phi_c(n, True, ref["mode"], vec, block, blocks)
    got, (want, mag) = float(ops["out"][0]), ref["dphi"]
    print(f"{tag} phi'(0): {got!r} vs {want!r}, error / (c u sum|ab|) = {abs(got - want) / (c * wolfe_ref.U32 * wolfe_ref.SLACK * mag):.3f} (c = {c})")
    assert abs(got - want) <= c * wolfe_ref.U32 * wolfe_ref.SLACK * mag
    assert _bits(ops["out"][1:], before["out"][1:]), "the direction writes out[0] alone"
    # ---- the same launch again: the same bits
    again = {k: before[k].clone() for k in before}
    _direction(again, n, cfg)
    torch.cuda.synchronize()
    assert all(_bits(again[k], ops[k]) for k in ("mom", "p", "theta0", "out")), "two launches differ"
    # ---- trial points and phi' there
    p_in = ops["p"].clone()
    for alpha in ALPHAS:
        _lib().call("fb_mt_wolfe_trial", ops["theta"].data_ptr(), ops["theta0"].data_ptr(), ops["p"].data_ptr(), n, LR * alpha)
        _lib().call("fb_mt_wolfe_phi_grad", ops["theta"].data_ptr(), ops["grad2"].data_ptr(), ops["p"].data_ptr(), n, wd, ops["out"].data_ptr() + 4,
                    ops["ws"].data_ptr())
        torch.cuda.synchronize()
        ratio, where = within_bound(ops["theta"][:n], *wolfe_ref.trial_f64(before["theta"][:n], p_in[:n], LR, alpha))
        print(f"{tag} theta(alpha={alpha}): worst error/bound {ratio:.3f} at {where}")
        assert ratio <= 1.0
        assert padding_untouched(ops["theta"], n) and _bits(ops["p"], p_in) and _bits(ops["theta0"][:n], before["theta"][:n])
        assert _bits(ops["grad2"], before["grad2"])
        want, mag = wolfe_ref.phi_grad_f64(ops["theta"][:n], before["grad2"][:n], p_in[:n], wd)
        c = wolfe_ref.phi_c(n, False, ref["mode"], vec, block, blocks)
        got = float(ops["out"][1])
        print(f"{tag} phi'({alpha}): {got!r} vs {want!r}, error / (c u sum|ab|) = {abs(got - want) / (c * wolfe_ref.U32 * wolfe_ref.SLACK * mag):.3f} (c = {c})")
        assert abs(got - want) <= c * wolfe_ref.U32 * wolfe_ref.SLACK * mag
        first_bits = ops["out"].clone()
        _lib().call("fb_mt_wolfe_phi_grad", ops["theta"].data_ptr(), ops["grad2"].data_ptr(), ops["p"].data_ptr(), n, wd, ops["out"].data_ptr() + 4,
                    ops["ws"].data_ptr())
        torch.cuda.synchronize()
        assert _bits(first_bits, ops["out"]), "two launches differ"
    assert n < 64 or not _bits(ops["theta"][:n], before["theta"][:n])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wolfe_kernels_at_the_span_edges(name):
    vec, block, blocks = _spans()
    sizes = _sizes()
    assert sizes[0] == 1 and blocks * block * vec + vec + 1 in sizes and len(sizes) == 14
    for n in sizes:
        _check(n, name, seed=n)


@pytest.mark.parametrize("name", ["nesterov", "no-momentum-decay"])
def test_wolfe_kernels_at_the_resnet20_arena(name):
    n = _resnet20_arena()
    assert n == 4_327_754          # (the presets' ResNet-20: 4.1 passes of the grid-stride loop, two trailing elements)
    _check(n, name)


@exercises("fb_mt_wolfe_direction", "fb_mt_wolfe_trial", "fb_mt_wolfe_phi_grad")
def test_wolfe_kernels_at_production_size():
    """ResNet-18's arena, n = 11 173 962 (n % 4 == 2: two trailing elements): 10.7 passes of the grid-stride loop."""
    assert N18 % 4 == 2
    _check(N18, "nesterov")


def test_wolfe_without_a_momentum_buffer():
    """momentum = 0: ``mom`` may be NULL."""
    n = 4099
    ops = _inputs(n, 1)
    want = {k: v.clone() for k, v in ops.items()}
    _direction(want, n, CONFIGS["no-momentum-decay"])
    _lib().call("fb_mt_wolfe_direction", ops["theta"].data_ptr(), ops["grad"].data_ptr(), None, ops["p"].data_ptr(), ops["theta0"].data_ptr(), n,
                1e-2, 0.0, 0.0, 0, 0, ops["out"].data_ptr(), ops["ws"].data_ptr())
    torch.cuda.synchronize()
    assert all(_bits(ops[k], want[k]) for k in ("p", "theta0", "out", "mom"))


def test_wolfe_refuses_bad_arguments_without_a_launch():
    lib = _lib()
    h = lib.load()
    n = 4099
    ops = _inputs(n, 2)
    before = {k: v.clone() for k, v in ops.items()}
    stream = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")
    P = {k: v.data_ptr() for k, v in ops.items()}

    def direction(**kw):
        a = dict(theta=P["theta"], grad=P["grad"], mom=P["mom"], p=P["p"], theta0=P["theta0"], n=n, wd=5e-4, mu=0.9, damp=0.0, nesterov=1, first=0,
                 out=P["out"], ws=P["ws"]) | kw
        return h.fb_mt_wolfe_direction(*a.values(), stream)

    def trial(**kw):
        a = dict(theta=P["theta"], theta0=P["theta0"], p=P["p"], n=n, step=0.1) | kw
        return h.fb_mt_wolfe_trial(*a.values(), stream)

    def phi_grad(**kw):
        a = dict(theta=P["theta"], grad=P["grad"], p=P["p"], n=n, wd=5e-4, out=P["out"], ws=P["ws"]) | kw
        return h.fb_mt_wolfe_phi_grad(*a.values(), stream)

    for fn, ptrs, scalars in ((direction, ("theta", "grad", "mom", "p", "theta0", "out", "ws"), ("wd", "mu", "damp")),
                              (trial, ("theta", "theta0", "p"), ("step",)), (phi_grad, ("theta", "grad", "p", "out", "ws"), ("wd",))):
        for k in ptrs:
            assert fn(**{k: None}) == FB_ERR_ARG, (fn.__name__, k)
            assert b"fb_mt_wolfe" in h.fb_last_error_string()
            if k not in ("out", "ws"):
                assert fn(**{k: P[k] + 4}) == FB_ERR_ARG, (fn.__name__, k, "misaligned")
        for k in scalars:
            for x in (nan, inf, -inf):
                assert fn(**{k: x}) == FB_ERR_ARG, (fn.__name__, k, x)
        assert fn(n=-1) == FB_ERR_ARG
    torch.cuda.synchronize()
    assert all(_bits(ops[k], before[k]) for k in ops), "a refused call launched something"
    assert trial(n=0) == 0
    torch.cuda.synchronize()
    assert _bits(ops["theta"], before["theta"])


def test_wolfe_through_a_recorded_command_list():
    """Recordable: the calls replayed by the native executor give the bits of the direct calls."""
    lib = _lib()
    n = 70_001
    want, ops = _inputs(n, 3), _inputs(n, 3)
    before = {k: v.clone() for k, v in ops.items()}

    def run(o):
        _direction(o, n, CONFIGS["nesterov"])
        lib.call("fb_mt_wolfe_trial", o["theta"].data_ptr(), o["theta0"].data_ptr(), o["p"].data_ptr(), n, LR)
        lib.call("fb_mt_wolfe_phi_grad", o["theta"].data_ptr(), o["grad2"].data_ptr(), o["p"].data_ptr(), n, 5e-4, o["out"].data_ptr() + 4, o["ws"].data_ptr())

    run(want)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        run(ops)
    cl = rec.finish()
    for k in ops:
        ops[k].copy_(before[k])
    cl.replay(streams)
    torch.cuda.synchronize()
    for k in ("theta", "mom", "p", "theta0", "out"):
        assert _bits(ops[k], want[k]), k
    assert np.isfinite(float(ops["out"].abs().max())) and not _bits(ops["theta"], before["theta"])
