"""``fb_mt_sgd_prep`` (csrc/sgd_prep.hip): the mini-batch update and both weight copies in one launch, against

  * the composition it replaces -- ``fb_mt_sgd_torch`` + one ``fb_weight_prep`` per layer -- BIT FOR BIT (parameters, momentum, copies),
  * ``fb_mt_clip_sgd`` bit for bit where the two clip forms give the same coefficient,
  * ``helpers.sgd_ref`` in float64 with its elementwise bounds, and the copies as plain torch casts / permutations of the new parameters,

on ResNet-20's real plan at 16 px (4.3 M parameters: arena size) and on a synthetic table with every awkward case at once: a 27 -> 64
layer without a transposed copy (Cin_pad 32), a 32 -> 64 3x3 layer, a 64 -> 32 1x1 layer whose offset is not a multiple of 4, gaps of 64
and 10 floats, a tail of 650 and n not a multiple of 256.  Padding columns of the copies must stay untouched; bad arguments are refused
without a launch; one run goes through ``helpers.confined`` (guard bands, three fills)."""
import numpy as np
import pytest
import torch

from tests.helpers import COEF_ROUNDINGS, U32, confined, f32r, sgd_ref, within_bound
from tests.test_gpu_update_production import N18, exercises

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = 1.2345e30
FB_ERR_ARG = -1
LR, WD = 0.1, 5e-4


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _synthetic():
    """rows {w_off, Cout, taps, Cin_real, Cin_pad, wc_off, has_dgrad, 0}, n, wc_total"""
    rows, off, wc = [], 0, 0
    for cout, taps, cin, cin_pad, dgrad, gap in ((64, 1, 27, 32, 0, 64), (64, 9, 32, 32, 1, 10), (32, 1, 64, 64, 1, 650)):
        rows.append([off, cout, taps, cin, cin_pad, wc, dgrad, 0])
        off += cout * taps * cin + gap
        wc += cout * taps * cin_pad
    assert rows[2][0] % 4 != 0 and off % 256 != 0 and off - (rows[2][0] + 32 * 64) == 650
    return rows, off, wc


_PLAN = {}


def _resnet20():
    if "rows" not in _PLAN:
        from fullbatchtraining_amd.cfg import compose
        from fullbatchtraining_amd.engine import Plan
        from fullbatchtraining_amd.models import construct_model
        torch.manual_seed(0)
        plan = Plan(construct_model(compose(["model=resnet20"]).model, 3, 10), 16)
        rows = [[L.w_off, L.cout, L.taps, L.cin_real, L.cin_pad, L.wc_off, 0 if L is plan.stem else 1, 0] for L in sorted(plan.layers, key=lambda L: L.w_off)]
        assert plan.stem.cin_real == 27 and plan.P > 4_000_000 and any(r[2] == 1 and r[6] for r in rows) and any(r[2] == 9 for r in rows)
        _PLAN["rows"] = (rows, plan.P, plan.wc_total)
    return _PLAN["rows"]


def _resnet18():
    """ResNet-18 at 32 px: the arena of the benchmark, the size tests/test_gpu_update_production.py holds every fb_mt_* entry point to."""
    if "r18" not in _PLAN:
        from fullbatchtraining_amd.cfg import compose
        from fullbatchtraining_amd.engine import Plan
        from fullbatchtraining_amd.models import construct_model
        torch.manual_seed(0)
        plan = Plan(construct_model(compose(["model=resnet18"]).model, 3, 10), 32)
        rows = [[L.w_off, L.cout, L.taps, L.cin_real, L.cin_pad, L.wc_off, 0 if L is plan.stem else 1, 0] for L in sorted(plan.layers, key=lambda L: L.w_off)]
        assert plan.P >= N18
        _PLAN["r18"] = (rows, plan.P, plan.wc_total)
    return _PLAN["r18"]


TABLES = {"synthetic": _synthetic, "resnet20": _resnet20, "resnet18": _resnet18}
_KEEP = []          # every layer table handed to the library stays alive: it keys its host copy of a table by the table's address


def _state(table, dtype, seed=0):
    rows, n, wc = TABLES[table]()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    s = dict(rows=rows, n=n, wc=wc, dtype=dtype,
             theta=torch.randn(n, device="cuda", generator=gen) * 0.1, grad=torch.randn(n, device="cuda", generator=gen) * 0.01,
             mom=torch.randn(n, device="cuda", generator=gen) * 0.01, gnorm2=torch.zeros(2, device="cuda"),
             tab=torch.tensor(rows, dtype=torch.int32, device="cuda"))
    _KEEP.append(s["tab"])
    return s


def _copies(s):
    return (torch.full((s["wc"],), SENTINEL, device="cuda", dtype=s["dtype"]), torch.full((s["wc"],), SENTINEL, device="cuda", dtype=s["dtype"]))


def _hyp_args(h):
    return (-1.0 if h["clip"] is None else float(h["clip"]), LR, WD, h["mu"], h["damp"], 1 if h["nesterov"] else 0, 1 if h["first"] else 0)


def _run_fused(s, h):
    lib = _lib()
    theta, mom, (wf, wd) = s["theta"].clone(), s["mom"].clone(), _copies(s)
    lib.call("fb_mt_sgd_prep", theta.data_ptr(), s["grad"].data_ptr(), mom.data_ptr(), s["n"], s["gnorm2"].data_ptr(), *_hyp_args(h),
             s["tab"].data_ptr(), len(s["rows"]), wf.data_ptr(), wd.data_ptr(), lib.dtype_code(s["dtype"]))
    torch.cuda.synchronize()
    return theta, mom, wf, wd


def _run_composition(s, h):
    lib = _lib()
    theta, mom, (wf, wd) = s["theta"].clone(), s["mom"].clone(), _copies(s)
    lib.call("fb_mt_sgd_torch", theta.data_ptr(), s["grad"].data_ptr(), mom.data_ptr(), s["n"], s["gnorm2"].data_ptr(), *_hyp_args(h))
    es = wf.element_size()
    for w_off, cout, taps, cin, cin_pad, wc_off, dgrad, _ in s["rows"]:
        lib.call("fb_weight_prep", theta.data_ptr() + 4 * w_off, s["n"], s["wc"], 1, cout, taps, cin, cin_pad, wf.data_ptr() + es * wc_off,
                 wd.data_ptr() + es * wc_off if dgrad else None, lib.dtype_code(s["dtype"]), None)
    torch.cuda.synchronize()
    return theta, mom, wf, wd


def _masks(s):
    """(written by the fused pass, written by fb_weight_prep only = padding columns) for the forward and the transposed copy"""
    fw, fp, dw, dp = (torch.zeros(s["wc"], dtype=torch.bool, device="cuda") for _ in range(4))
    for w_off, cout, taps, cin, cin_pad, wc_off, dgrad, _ in s["rows"]:
        size = cout * taps * cin_pad
        real = torch.zeros(cout, taps, cin_pad, dtype=torch.bool, device="cuda")
        real[:, :, :cin] = True
        fw[wc_off:wc_off + size] = real.reshape(-1)
        fp[wc_off:wc_off + size] = ~real.reshape(-1)
        if dgrad:
            realt = real.permute(2, 1, 0).reshape(-1)
            dw[wc_off:wc_off + size] = realt
            dp[wc_off:wc_off + size] = ~realt
    return fw, fp, dw, dp


def _bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int16)


def _torch_coef(s, h):
    """(coef, hit) of clip_grad_norm_ from the fp32 device scalar, in float64"""
    if h["clip"] is None:
        return 1.0, False
    norm = float(np.sqrt(np.float64(np.float32(float(s["gnorm2"][0])))))
    coef = min(1.0, f32r(h["clip"]) / (norm + f32r(1e-6)))
    return coef, coef < 1.0


#  first  mu   damp nesterov  clip: None | ("rel", factor of the norm) | "edge" (norm within 1e-6 below the clip)
HYPS = {
    "first-step-no-clip": dict(first=True, mu=0.9, damp=0.0, nesterov=True, clip=None),
    "clip-far-above-norm": dict(first=False, mu=0.9, damp=0.0, nesterov=True, clip=("rel", 100.0)),
    "clip-far-below-norm-plain-momentum": dict(first=False, mu=0.9, damp=0.1, nesterov=False, clip=("rel", 0.01)),
    "momentum-0": dict(first=False, mu=0.0, damp=0.0, nesterov=False, clip=None),
    "first-step-clipped": dict(first=True, mu=0.9, damp=0.0, nesterov=False, clip=("rel", 0.5)),
    "norm-within-1e-6-below-clip": dict(first=False, mu=0.9, damp=0.0, nesterov=True, clip="edge"),
}


def _prepare(table, dtype, hyp):
    s, h = _state(table, dtype), dict(HYPS[hyp])
    if h["clip"] == "edge":
        # the clip reads the device scalar, so the edge is set there: |g| = 0.5 exactly, clip = 0.5 + 5e-7 -- min(1, clip / (norm + 1e-6)) = 1 - 1e-6
        # scales, `norm > clip` does not
        s["gnorm2"][0] = 0.25
        h["clip"] = f32r(0.5 + 5e-7)
        assert 0.5 < h["clip"] < 0.5 + 1e-6
    else:
        s["gnorm2"][0] = s["grad"].double().pow(2).sum().float()
        if h["clip"] is not None:
            h["clip"] = f32r(h["clip"][1] * float(s["gnorm2"][0]) ** 0.5)
    return s, h


@pytest.mark.parametrize("hyp", list(HYPS))
@pytest.mark.parametrize("table", ["synthetic", "resnet20"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sgd_prep_against_composition_and_float64(dtype, table, hyp):
    _against_composition_and_float64(dtype, table, hyp)


@exercises("fb_mt_sgd_prep", "fb_mt_sgd_torch")
@pytest.mark.parametrize("hyp", ["first-step-clipped", "clip-far-below-norm-plain-momentum"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sgd_prep_at_production_size(dtype, hyp):
    """The same checks on ResNet-18's arena (n = 11 174 016 >= the 11 173 962 of tests/test_gpu_update_production.py, whose completeness check
    counts this case through its ``exercises`` registry): 11 000 tiles, every tile form of the 3x3 and 1x1 layers of four widths."""
    s, _ = _prepare("resnet18", dtype, hyp)
    assert s["n"] >= N18
    del s
    _against_composition_and_float64(dtype, "resnet18", hyp)


def _against_composition_and_float64(dtype, table, hyp):
    lib = _lib()
    s, h = _prepare(table, dtype, hyp)
    theta, mom, wf, wd = _run_fused(s, h)
    theta_c, mom_c, wf_c, wd_c = _run_composition(s, h)
    # ---- the composition, bit for bit
    assert torch.equal(_bits(theta), _bits(theta_c)) and torch.equal(_bits(mom), _bits(mom_c))
    fw, fp, dw, dp = _masks(s)
    assert torch.equal(_bits(wf)[fw], _bits(wf_c)[fw]) and torch.equal(_bits(wd)[dw], _bits(wd_c)[dw])
    # ---- padding columns: fb_weight_prep writes their zeros, the fused pass leaves them alone; what belongs to no layer (the stem's slot of the
    # transposed copy) is nobody's
    sent = torch.tensor(SENTINEL, device="cuda").to(dtype)
    assert bool((wf[fp] == sent).all()) and bool((wd[dp] == sent).all()) and bool((wf_c[fp] == 0).all()) and bool((wd_c[dp] == 0).all())
    assert bool((wf[~(fw | fp)] == sent).all()) and bool((wd[~(dw | dp)] == sent).all()) and bool((wd_c[~(dw | dp)] == sent).all())
    assert int(fp.sum()) > 0 and int((~(dw | dp)).sum()) > 0
    # ---- fb_mt_clip_sgd, where its clip form gives the same coefficient (everywhere but at the edge)
    coef, hit = _torch_coef(s, h)
    if hyp != "norm-within-1e-6-below-clip":
        theta_o, grad_o, mom_o = s["theta"].clone(), s["grad"].clone(), s["mom"].clone()
        lib.call("fb_mt_clip_sgd", theta_o.data_ptr(), grad_o.data_ptr(), mom_o.data_ptr(), s["n"], s["gnorm2"].data_ptr(), *_hyp_args(h))
        torch.cuda.synchronize()
        assert torch.equal(_bits(theta), _bits(theta_o)) and torch.equal(_bits(mom), _bits(mom_o))
    else:
        assert hit and 0 < 1.0 - coef < 2e-6
    if hyp.startswith("clip-far-above"):
        assert not hit
    if "clipped" in hyp or "far-below" in hyp:
        assert hit and coef < 0.6
    # ---- float64, with the bounds of the update kernels
    ref = sgd_ref(s["theta"], s["grad"], s["mom"], coef, hit, LR, WD, h["mu"], h["damp"], h["nesterov"], h["first"])
    worst, where = within_bound(theta, *ref["param"])
    print(f"[{table} {hyp}] theta': worst error / bound {worst:.3f} at {where}")
    assert worst <= 1.0
    if h["mu"] != 0.0:
        worst, where = within_bound(mom, *ref["mom"])
        print(f"[{table} {hyp}] mom': worst error / bound {worst:.3f} at {where}")
        assert worst <= 1.0
    else:
        assert torch.equal(mom, s["mom"])
    assert float((theta - s["theta"]).abs().max()) > 0
    # ---- the copies are the new parameters in the compute dtype: [co][tap][ci] padded, and [ci][tap][co]
    for w_off, cout, taps, cin, cin_pad, wc_off, dgrad, _ in s["rows"]:
        w = theta[w_off:w_off + cout * taps * cin].view(cout, taps, cin).to(dtype)
        size = cout * taps * cin_pad
        assert torch.equal(wf[wc_off:wc_off + size].view(cout, taps, cin_pad)[:, :, :cin], w)
        if dgrad:
            assert torch.equal(wd[wc_off:wc_off + size].view(cin_pad, taps, cout)[:cin], w.permute(2, 1, 0))
    # the gradient is read only
    assert float(s["grad"].double().pow(2).sum().float()) == float(s["gnorm2"][0]) or hyp == "norm-within-1e-6-below-clip"


def test_sgd_prep_result_does_not_depend_on_earlier_content_of_the_momentum_on_the_first_step():
    """first_step: the buffer is initialised, never read (NaNs in it do not travel)."""
    s, h = _prepare("synthetic", BF16, "first-step-no-clip")
    want = _run_fused(s, h)
    s["mom"].fill_(float("nan"))
    got = _run_fused(s, h)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(want, got))


def test_sgd_prep_refuses_bad_arguments_without_a_launch():
    lib = _lib()
    h = lib.load()
    s, hyp = _prepare("synthetic", F32, "clip-far-below-norm-plain-momentum")
    theta, mom, (wf, wd) = s["theta"].clone(), s["mom"].clone(), _copies(s)
    code = lib.dtype_code(F32)

    def call(theta_p, grad_p, mom_p, gn_p, tab, wf_p, wd_p, n=s["n"], dtype=code):
        return h.fb_mt_sgd_prep(theta_p, grad_p, mom_p, n, gn_p, *_hyp_args(hyp), None if tab is None else tab.data_ptr(),
                                0 if tab is None else tab.shape[0], wf_p, wd_p, dtype, torch.cuda.current_stream().cuda_stream)

    good = (theta.data_ptr(), s["grad"].data_ptr(), mom.data_ptr(), s["gnorm2"].data_ptr(), s["tab"], wf.data_ptr(), wd.data_ptr())
    for i in (0, 1, 2, 3, 5, 6):                                   # one null pointer at a time (6: a table with has_dgrad rows and no transposed copy)
        args = list(good)
        args[i] = None
        assert call(*args) == FB_ERR_ARG, i
        assert b"fb_mt_sgd_prep" in h.fb_last_error_string()
    unsorted = torch.tensor([s["rows"][1], s["rows"][0], s["rows"][2]], dtype=torch.int32, device="cuda")
    overlapping = torch.tensor([s["rows"][0], [s["rows"][0][0] + 8] + s["rows"][1][1:], s["rows"][2]], dtype=torch.int32, device="cuda")
    beyond = torch.tensor(s["rows"], dtype=torch.int32, device="cuda")
    narrow = torch.tensor([[0, 64, 1, 27, 16, 0, 0, 0]], dtype=torch.int32, device="cuda")      # Cin_pad < Cin_real
    _KEEP.extend([unsorted, overlapping, beyond, narrow])
    for tab in (unsorted, overlapping, narrow):
        assert call(*good[:4], tab, *good[5:]) == FB_ERR_ARG
        assert b"sorted" in h.fb_last_error_string()
    assert call(*good[:4], beyond, *good[5:], n=s["n"] - 700) == FB_ERR_ARG          # the last layer ends behind n
    assert call(*good, dtype=5) == FB_ERR_ARG
    torch.cuda.synchronize()
    # nothing was launched: every operand still holds what it held
    assert torch.equal(theta, s["theta"]) and torch.equal(mom, s["mom"]) and bool((wf == SENTINEL).all()) and bool((wd == SENTINEL).all())
    assert call(*good) == 0                                        # (and the same operands are accepted as they are)
    torch.cuda.synchronize()
    assert not torch.equal(theta, s["theta"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sgd_prep_is_confined_to_its_operands(dtype):
    """Guard bands around every operand, three fills (tests/test_gpu_confinement.py): reads and writes confined, the gradient, the norm and the
    table unchanged, the results independent of what surrounds the operands -- and equal to the unconfined run."""
    lib = _lib()
    s, h = _prepare("synthetic", dtype, "clip-far-below-norm-plain-momentum")
    wf0, wd0 = _copies(s)
    code = lib.dtype_code(dtype)
    out = confined(lambda o: lib.call("fb_mt_sgd_prep", o["theta"].data_ptr(), o["grad"].data_ptr(), o["mom"].data_ptr(), s["n"], o["gnorm2"].data_ptr(),
                                      *_hyp_args(h), o["tab"].data_ptr(), len(s["rows"]), o["w_fwd"].data_ptr(), o["w_dgrad"].data_ptr(), code),
                   inputs=dict(grad=s["grad"], gnorm2=s["gnorm2"], tab=s["tab"]), outputs={},
                   inout=dict(theta=s["theta"], mom=s["mom"], w_fwd=wf0, w_dgrad=wd0))
    want = _run_fused(s, h)
    for name, ref in zip(("theta", "mom", "w_fwd", "w_dgrad"), want):
        assert torch.equal(_bits(out[name].reshape(-1)), _bits(ref)), name
    out = confined(lambda o: lib.call("fb_mt_sgd_torch", o["theta"].data_ptr(), o["grad"].data_ptr(), o["mom"].data_ptr(), s["n"], o["gnorm2"].data_ptr(),
                                      *_hyp_args(h)),
                   inputs=dict(grad=s["grad"], gnorm2=s["gnorm2"]), outputs={}, inout=dict(theta=s["theta"], mom=s["mom"]))
    assert torch.equal(_bits(out["theta"].reshape(-1)), _bits(want[0])) and torch.equal(_bits(out["mom"].reshape(-1)), _bits(want[1]))


def test_sgd_prep_through_a_recorded_command_list():
    """Recordable: the call replayed by the native executor gives the bits of the direct call."""
    lib = _lib()
    s, h = _prepare("synthetic", BF16, "clip-far-below-norm-plain-momentum")
    want = _run_fused(s, h)
    theta, mom, (wf, wd) = s["theta"].clone(), s["mom"].clone(), _copies(s)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        lib.call("fb_mt_sgd_prep", theta.data_ptr(), s["grad"].data_ptr(), mom.data_ptr(), s["n"], s["gnorm2"].data_ptr(), *_hyp_args(h),
                 s["tab"].data_ptr(), len(s["rows"]), wf.data_ptr(), wd.data_ptr(), lib.dtype_code(BF16))
    cl = rec.finish()
    theta.copy_(s["theta"])
    mom.copy_(s["mom"])
    wf.fill_(SENTINEL)
    wd.fill_(SENTINEL)
    cl.replay(streams)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(want, (theta, mom, wf, wd)))
    assert COEF_ROUNDINGS * U32 < 1e-6          # (the edge case above is resolvable in fp32: 1e-6 is 16 ulp of 0.5)
