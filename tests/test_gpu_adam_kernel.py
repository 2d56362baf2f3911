"""``fb_mt_adamw`` (csrc/adamw.hip) against ``tests/adam_ref.adamw_ref`` in float64 with its elementwise bounds (shown to bite by
tests/test_cpu_adam.py), every case printing its worst error / bound ratio:

  * n = 1024 * 1024 + 3 with the four operands 1 and 3 floats off a 16-byte boundary (scalar head, 16-byte body, scalar tail; more than one
    pass of the grid-stride loop), once with operands that do NOT share their misalignment (the all-scalar path), and n = 11 173 962, the arena
    of the benchmark (declared to tests/test_gpu_update_production.py through ``exercises``);
  * no clip, the clip hit in both forms, far above the norm (the bits of the gradient unchanged), t = 1 from zero state and t = 7 from a random
    one, lr = 0 (parameters bit-identical), weight decay 0, all zeros (stay exactly 0), a second moment in the denormal range;
  * the SENTINEL columns behind n untouched; two launches over the halves of a range = one launch over the whole, bit for bit; bad arguments
    refused without a launch; a recorded command list replays the same bits."""
import numpy as np
import pytest
import torch

from tests import adam_ref
from tests.helpers import SENTINEL, clip_coef_ref, f32r, padding_untouched, within_bound
from tests.test_gpu_update_production import N18, exercises

pytestmark = pytest.mark.gpu

FB_ERR_ARG = -1
PAD = 64
N_EDGE = 1024 * 1024 + 3
HYP = dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
NAMES = ("theta", "grad", "exp_avg", "exp_avg_sq")


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _carve(n, offs, seed=0, kind="random"):
    """Four [n + PAD] fp32 operands, operand k starting ``offs[k]`` floats behind a 256-byte boundary, SENTINEL behind the n values."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    scale = dict(theta=0.1, grad=0.01, exp_avg=0.01, exp_avg_sq=0.01)
    out = {}
    for name, off in zip(NAMES, offs):
        base = torch.empty(n + PAD + 8, device="cuda", dtype=torch.float32)
        assert base.data_ptr() % 256 == 0
        t = base[off:off + n + PAD]
        t[:n].normal_(generator=gen).mul_(scale[name])
        if name == "exp_avg_sq":
            t[:n].pow_(2)
        t[n:] = SENTINEL
        assert (t.data_ptr() % 16) // 4 == off % 4
        out[name] = t
    if kind in ("zero-state", "zeros"):
        out["exp_avg"][:n] = 0
        out["exp_avg_sq"][:n] = 0
    if kind == "zeros":
        out["theta"][:n] = 0
        out["grad"][:n] = 0
    if kind == "denormal":                   # |g| ~ 1e-21: (1 - b2) g^2 ~ 1e-45, v = 3e-42: the second moment stays denormal, eps decides the denominator
        out["grad"][:n] *= 1e-19
        out["exp_avg"][:n] *= 1e-19
        out["exp_avg_sq"][:n] = 3e-42
    return out


def _launch(ops, n, gnorm2, clip, hyp, t, lo=0):
    lib = _lib()
    h = adam_ref.host_scalars(hyp, t)
    lib.call("fb_mt_adamw", *[ops[k].data_ptr() + 4 * lo for k in NAMES], n, None if gnorm2 is None else gnorm2.data_ptr(),
             -1.0 if clip is None else float(clip), 1 if hyp.get("torch_clip") else 0, float(hyp["lr"]), float(hyp["weight_decay"]),
             float(hyp["betas"][0]), float(hyp["betas"][1]), float(hyp["eps"]), h["step_size"], h["bc2s"])


#                 state kind     clip: None | factor of the norm     hyp overrides                 t
CASES = {
    "no-clip-t7": ("random", None, {}, 7),
    "t1-zero-state": ("zero-state", None, {}, 1),
    "clip-hit": ("random", 0.5, {}, 7),
    "clip-hit-torch-form": ("random", 0.5, dict(torch_clip=True), 7),
    "clip-far-above-norm": ("random", 100.0, {}, 7),
    "clip-far-above-norm-torch-form": ("random", 100.0, dict(torch_clip=True), 7),
    "lr-0": ("random", None, dict(lr=0.0), 1),
    "wd-0": ("random", None, dict(weight_decay=0.0), 3),
    "all-zeros": ("zeros", None, {}, 1),
    "denormal-second-moment": ("denormal", None, {}, 7),
}


def _check(n, offs, case):
    kind, clip_rel, over, t = CASES[case]
    hyp = dict(HYP, **over)
    ops = _carve(n, offs, kind=kind)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = before["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = None if clip_rel is None else f32r(clip_rel * float(gnorm2) ** 0.5)
    _launch(ops, n, gnorm2, clip, hyp, t)
    torch.cuda.synchronize()
    coef, hit = (adam_ref.torch_clip_coef_ref if hyp.get("torch_clip") else clip_coef_ref)(float(gnorm2), clip)
    ref = adam_ref.adamw_ref(*[before[k][:n] for k in NAMES], coef, hit, hyp, t)
    for name, key in zip(NAMES, ("param", "grad", "exp_avg", "exp_avg_sq")):
        worst, where = within_bound(ops[name][:n], *ref[key])
        print(f"[adamw n={n} offs={offs} {case}] {name}: worst error / bound {worst:.3f} at {where}")
        assert worst <= 1.0, (name, worst, where)
        assert padding_untouched(ops[name], n), name
    g_same = torch.equal(ops["grad"].view(torch.int32), before["grad"].view(torch.int32))
    if case == "clip-hit":
        assert hit and coef < 0.6 and not g_same
    else:
        assert g_same                        # no clip, a clip that does not scale, the torch form: the bits of the gradient
    if "far-above" in case:
        assert not hit
    if case == "clip-hit-torch-form":
        assert hit and coef < 0.6
    if case == "lr-0":
        assert torch.equal(ops["theta"].view(torch.int32), before["theta"].view(torch.int32))
        assert not torch.equal(ops["exp_avg"], before["exp_avg"]) and not torch.equal(ops["exp_avg_sq"], before["exp_avg_sq"])
    elif case == "all-zeros":
        assert all(not bool(ops[k][:n].view(torch.int32).any()) for k in NAMES)          # +0 everywhere: the arena's alignment padding stays 0
    else:
        assert float((ops["theta"][:n] - before["theta"][:n]).abs().max()) > 0
    if case == "denormal-second-moment":
        assert 0 < float(ops["exp_avg_sq"][:n].max()) < 1.2e-38 and float(ops["exp_avg_sq"][:n].min()) > 0


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("off", [1, 3])
def test_adamw_against_float64(off, case):
    _check(N_EDGE, (off,) * 4, case)


@pytest.mark.parametrize("case", ["no-clip-t7", "clip-hit"])
def test_adamw_with_operands_of_different_misalignment(case):
    """theta, grad, exp_avg, exp_avg_sq 0 / 1 / 2 / 3 floats off a 16-byte boundary: no common vector body, every element on the scalar path."""
    _check(256 * 2048 + 5, (0, 1, 2, 3), case)


@pytest.mark.parametrize("case", ["no-clip-t7", "clip-hit"])
def test_adamw_small_ranges(case):
    """Ranges shorter than the head, shorter than one vector, and one vector exactly."""
    for n, off in ((1, 1), (2, 3), (3, 1), (4, 0), (5, 3), (7, 2)):
        _check(n, (off,) * 4, case)


@exercises("fb_mt_adamw")
@pytest.mark.parametrize("case", ["no-clip-t7", "clip-hit", "clip-hit-torch-form"])
def test_adamw_at_production_size(case):
    """ResNet-18's arena, n = 11 173 962 (n % 4 == 2: the scalar tail runs): 5.3 passes of the grid-stride loop."""
    assert N18 % 4 == 2
    _check(N18, (0,) * 4, case)


@pytest.mark.parametrize("case", ["no-clip-t7", "clip-hit"])
def test_adamw_result_does_not_depend_on_how_the_range_is_cut(case):
    """One launch over [0, n) = a launch over [0, h) and one over [h, n), h odd (the second range starts 1 float off: other head, other body)."""
    kind, clip_rel, over, t = CASES[case]
    n, h = N_EDGE, N_EDGE // 2 + 1
    whole, halves = _carve(n, (3,) * 4, kind=kind), _carve(n, (3,) * 4, kind=kind)
    assert all(torch.equal(whole[k], halves[k]) for k in NAMES)
    gnorm2 = whole["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = None if clip_rel is None else f32r(clip_rel * float(gnorm2) ** 0.5)
    _launch(whole, n, gnorm2, clip, HYP, t)
    _launch(halves, h, gnorm2, clip, HYP, t)
    _launch(halves, n - h, gnorm2, clip, HYP, t, lo=h)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(whole[k].view(torch.int32), halves[k].view(torch.int32)), k


def test_adamw_refuses_bad_arguments_without_a_launch():
    lib = _lib()
    h = lib.load()
    n = 4099
    ops = _carve(n, (1,) * 4)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = torch.ones(1, device="cuda")
    hs = adam_ref.host_scalars(HYP, 7)
    stream = torch.cuda.current_stream().cuda_stream
    #          gnorm2            clip torch lr   wd    b1   b2     eps   step_size        bc2s
    good = [n, gnorm2.data_ptr(), 0.5, 0, 1e-3, 0.01, 0.9, 0.999, 1e-8, hs["step_size"], hs["bc2s"]]
    ptrs = [ops[k].data_ptr() for k in NAMES]
    for i in range(4):
        assert h.fb_mt_adamw(*[None if j == i else p for j, p in enumerate(ptrs)], *good, stream) == FB_ERR_ARG, i
        assert b"fb_mt_adamw" in h.fb_last_error_string()
    for i, x in ((1, None), (6, 1.0), (6, -0.5), (7, 1.0), (7, 1.5), (8, 0.0), (8, -1e-8), (10, 0.0), (10, -0.5), (0, -1)):
        args = list(good)
        args[i] = x
        assert h.fb_mt_adamw(*ptrs, *args, stream) == FB_ERR_ARG, (i, x)
    assert h.fb_mt_adamw(ptrs[0] + 2, *ptrs[1:], *good, stream) == FB_ERR_ARG             # not a float boundary
    torch.cuda.synchronize()
    assert all(torch.equal(ops[k].view(torch.int32), before[k].view(torch.int32)) for k in NAMES)     # nothing was launched
    assert h.fb_mt_adamw(*ptrs, *good, stream) == 0                                       # (and the same operands are accepted as they are)
    torch.cuda.synchronize()
    assert not torch.equal(ops["theta"], before["theta"])


def test_adamw_through_a_recorded_command_list():
    """Recordable: the call replayed by the native executor gives the bits of the direct call."""
    lib = _lib()
    n = 70_001
    want, ops = _carve(n, (3,) * 4), _carve(n, (3,) * 4)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = ops["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)
    _launch(want, n, gnorm2, clip, HYP, 7)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        _launch(ops, n, gnorm2, clip, HYP, 7)
    cl = rec.finish()
    for k in NAMES:
        ops[k].copy_(before[k])
    cl.replay(streams)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(ops[k].view(torch.int32), want[k].view(torch.int32)), k
    assert not torch.equal(ops["grad"], before["grad"]) and np.isfinite(float(ops["theta"][:n].abs().max()))
