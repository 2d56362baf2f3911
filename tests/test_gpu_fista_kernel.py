"""``fb_mt_fista`` (csrc/fista.hip) against the float32 restatement of the reference's step (tests/fista_ref.py, held against recorded steps of
the reference by tests/test_cpu_fista.py): BIT FOR BIT in theta, x_minus and grad -- there is no tolerance.

  * n in {1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4099} with the three operands 0..3 floats off a 16-byte boundary (scalar head, 16-byte body,
    scalar tail), one layout whose operands do NOT share their misalignment (the all-scalar path), n = 2 100 003 (more 16-byte vectors than the
    capped grid has threads: the stride loop runs twice) and n = 11 173 962, the arena of the benchmark (declared to
    tests/test_gpu_update_production.py through ``exercises``);
  * no clip; the full-batch clip with norm > clip (the clipped gradient is written back) and norm <= clip (the gradient's bits untouched); the
    ``clip_grad_norm_`` form with coef < 1 and coef >= 1 (never written); lr = 0, ak = 0, ak != 0; gradient magnitudes over 1e-6 .. 1e2;
  * the SENTINEL columns behind n untouched; n = 0 and every argument error return their codes and touch nothing; two launches over the parts of
    a range = one launch over the whole; a recorded command list replays the same bits.

The clip coefficient is formed in float32 from the value in ``gnorm2`` the way the kernel states it (``fista_ref.clip_coef_f32``)."""
import numpy as np
import pytest
import torch

from tests import fista_ref
from tests.helpers import SENTINEL, f32r, padding_untouched
from tests.test_gpu_update_production import N18, exercises

pytestmark = pytest.mark.gpu

FB_ERR_ARG = -1
PAD = 64
NAMES = ("theta", "grad", "x_minus")
N_STRIDE = 2_100_003
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4099)
_AK3 = fista_ref.coefficients_ref(fista_ref.coefficients_ref(fista_ref.coefficients_ref(1.0, (1.0, 1.0, 4.0))[0], (1.0, 1.0, 4.0))[0], (1.0, 1.0, 4.0))[1]
assert 0.4 < _AK3 < 0.5


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _carve(n, offs, seed=0):
    """Three [n + PAD] fp32 operands inside ONE larger buffer, operand k starting ``offs[k]`` floats behind a 256-byte boundary of it, SENTINEL
    behind the n values (and everywhere else in the buffer); gradient magnitudes log-uniform over 1e-6 .. 1e2."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    slot = (n + PAD + 8 + 63) // 64 * 64
    base = torch.full((3 * slot,), SENTINEL, device="cuda", dtype=torch.float32)
    assert base.data_ptr() % 256 == 0
    for k, (name, off) in enumerate(zip(NAMES, offs)):
        t = base[k * slot + off:k * slot + off + n + PAD]
        t[:n].normal_(generator=gen)
        if name == "grad":
            t[:n].mul_(torch.pow(10.0, torch.rand(n, device="cuda", generator=gen) * 8 - 6))
        else:
            t[:n].mul_(0.1)
        t[n:] = SENTINEL
        assert (t.data_ptr() % 16) // 4 == off % 4
        out[name] = t
    return out


def _launch(ops, n, gnorm2, clip, torch_clip, lr, ak, lo=0):
    _lib().call("fb_mt_fista", *[ops[k].data_ptr() + 4 * lo for k in NAMES], n, None if gnorm2 is None else gnorm2.data_ptr(),
                -1.0 if clip is None else float(clip), 1 if torch_clip else 0, float(lr), float(ak), float(np.float32(1) + np.float32(ak)))


#                                   clip: None | factor of the norm   torch form   lr    ak
CASES = {
    "no-clip": (None, False, 0.1, _AK3),
    "clip-hit": (0.5, False, 0.1, _AK3),
    "clip-not-hit": (2.0, False, 0.1, _AK3),
    "clip-at-the-norm": (1.0, False, 0.07, _AK3),
    "torch-clip-hit": (0.5, True, 0.1, _AK3),
    "torch-clip-not-hit": (2.0, True, 0.1, _AK3),
    "lr-0": (None, False, 0.0, _AK3),
    "ak-0": (None, False, 0.1, 0.0),
    "lr-0-ak-0": (0.5, False, 0.0, 0.0),
}


def _expected(before, n, gnorm2, clip, torch_clip, lr, ak):
    coef, hit = fista_ref.clip_coef_f32(float(gnorm2), clip, torch_clip)
    theta, g, xm = fista_ref.fista_ref(*[before[k][:n].cpu().numpy() for k in NAMES], coef, lr, ak, np.float32(1) + np.float32(ak))
    grad = g if (hit and not torch_clip) else before["grad"][:n].cpu().numpy()
    return dict(theta=theta, grad=grad, x_minus=xm), coef, hit


def _check(n, offs, case, seed=0):
    clip_rel, torch_clip, lr, ak = CASES[case]
    ops = _carve(n, offs, seed=seed)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = before["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = None if clip_rel is None else f32r(clip_rel * float(np.sqrt(np.float32(float(gnorm2)), dtype=np.float32)))
    _launch(ops, n, gnorm2, clip, torch_clip, lr, ak)
    torch.cuda.synchronize()
    want, coef, hit = _expected(before, n, gnorm2, clip, torch_clip, lr, ak)
    for name in NAMES:
        got = ops[name][:n].cpu().numpy()
        diff = int(np.count_nonzero(got.view(np.int32) != want[name].view(np.int32)))
        print(f"[fista n={n} offs={offs} {case}] {name}: {diff} of {n} elements differ in their bits (coef {float(coef)!r})")
        assert diff == 0, (name, diff)
        assert padding_untouched(ops[name], n), name
    g_same = torch.equal(ops["grad"].view(torch.int32), before["grad"].view(torch.int32))
    assert g_same == (not (hit and not torch_clip))             # written back by the full-batch form that scales, and by nothing else
    if n >= 255:                                 # (a norm far above the 1e-6 in the coefficient: the case is the one its name says)
        assert hit == (case in ("clip-hit", "torch-clip-hit", "lr-0-ak-0")) and (not hit or float(coef) < 0.6)
    if lr == 0.0 and ak == 0.0:                  # nothing moves: x+ = theta, theta' = x+ * 1 - x- * 0
        assert torch.equal(ops["theta"][:n], before["theta"][:n]) and torch.equal(ops["x_minus"][:n], before["theta"][:n])
    elif ak == 0.0:
        assert torch.equal(ops["theta"][:n], ops["x_minus"][:n])
        assert n < 255 or not torch.equal(ops["theta"][:n], before["theta"][:n])
    elif n >= 255:
        assert not torch.equal(ops["theta"][:n], ops["x_minus"][:n])


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_fista_bit_for_bit_at_edge_sizes(off, case):
    for n in SIZES:
        _check(n, (off,) * 3, case, seed=n)


@pytest.mark.parametrize("case", ["no-clip", "clip-hit", "torch-clip-hit"])
def test_fista_with_operands_of_different_misalignment(case):
    """theta, grad, x_minus 0 / 1 / 3 floats off a 16-byte boundary: no common vector body, every element on the scalar path."""
    for n in (5, 257, 4099):
        _check(n, (0, 1, 3), case, seed=n)


@pytest.mark.parametrize("case", ["no-clip", "clip-hit"])
def test_fista_when_the_stride_loop_runs_more_than_once(case):
    """n = 2 100 003 at offset 1: 525 000 vectors for 2048 x 256 = 524 288 threads."""
    assert (N_STRIDE - 3) // 4 > 2048 * 256
    _check(N_STRIDE, (1,) * 3, case)


@exercises("fb_mt_fista")
@pytest.mark.parametrize("case", ["no-clip", "clip-hit", "torch-clip-hit"])
def test_fista_at_production_size(case):
    """ResNet-18's arena, n = 11 173 962 (n % 4 == 2: the scalar tail runs): 5.3 passes of the grid-stride loop."""
    assert N18 % 4 == 2
    _check(N18, (0,) * 3, case)


@pytest.mark.parametrize("case", ["no-clip", "clip-hit"])
def test_fista_result_does_not_depend_on_how_the_range_is_cut(case):
    """One launch over [0, n) = a launch over [0, h) and one over [h, n), h odd (the second range starts 1 float off: other head, other body)."""
    clip_rel, torch_clip, lr, ak = CASES[case]
    n, h = 70_001, 35_001
    whole, halves = _carve(n, (3,) * 3), _carve(n, (3,) * 3)
    assert all(torch.equal(whole[k], halves[k]) for k in NAMES)
    gnorm2 = whole["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = None if clip_rel is None else f32r(clip_rel * float(gnorm2) ** 0.5)
    _launch(whole, n, gnorm2, clip, torch_clip, lr, ak)
    _launch(halves, h, gnorm2, clip, torch_clip, lr, ak)
    _launch(halves, n - h, gnorm2, clip, torch_clip, lr, ak, lo=h)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(whole[k].view(torch.int32), halves[k].view(torch.int32)), k


def test_fista_refuses_bad_arguments_and_n_0_without_a_launch():
    lib = _lib()
    h = lib.load()
    n = 4099
    ops = _carve(n, (1,) * 3)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = torch.ones(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    #          gnorm2            clip torch lr   ak    one_plus_ak
    good = [n, gnorm2.data_ptr(), 0.5, 0, 0.1, 0.25, 1.25]
    ptrs = [ops[k].data_ptr() for k in NAMES]
    for i in range(3):
        assert h.fb_mt_fista(*[None if j == i else p for j, p in enumerate(ptrs)], *good, stream) == FB_ERR_ARG, i
        assert b"fb_mt_fista" in h.fb_last_error_string()
    nan, inf = float("nan"), float("inf")
    for i, x in ((1, None), (0, -1), (4, -0.1), (4, nan), (4, inf), (5, nan), (5, -inf), (6, nan), (6, inf)):
        args = list(good)
        args[i] = x
        assert h.fb_mt_fista(*ptrs, *args, stream) == FB_ERR_ARG, (i, x)
    assert h.fb_mt_fista(ptrs[0] + 2, *ptrs[1:], *good, stream) == FB_ERR_ARG              # not a float boundary
    args = list(good)
    args[0] = 0
    assert h.fb_mt_fista(*ptrs, *args, stream) == 0                                        # n = 0: FB_OK, nothing to do
    torch.cuda.synchronize()
    assert all(torch.equal(ops[k].view(torch.int32), before[k].view(torch.int32)) for k in NAMES)     # nothing was launched
    assert h.fb_mt_fista(*ptrs, *good, stream) == 0                                        # (and the same operands are accepted as they are)
    torch.cuda.synchronize()
    assert not torch.equal(ops["theta"], before["theta"])


def test_fista_through_a_recorded_command_list():
    """Recordable: the call replayed by the native executor gives the bits of the direct call."""
    lib = _lib()
    n = 70_001
    want, ops = _carve(n, (3,) * 3), _carve(n, (3,) * 3)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = ops["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)
    _launch(want, n, gnorm2, clip, False, 0.1, _AK3)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        _launch(ops, n, gnorm2, clip, False, 0.1, _AK3)
    cl = rec.finish()
    for k in NAMES:
        ops[k].copy_(before[k])
    cl.replay(streams)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(ops[k].view(torch.int32), want[k].view(torch.int32)), k
    assert not torch.equal(ops["grad"], before["grad"]) and np.isfinite(float(ops["theta"][:n].abs().max()))
