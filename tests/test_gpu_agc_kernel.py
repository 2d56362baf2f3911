"""``fb_mt_agc_sgd`` (csrc/agc_sgd.hip) against ``tests/agc_ref.agc_ref`` in float64 with its elementwise bounds (shown to bite by
tests/test_cpu_agc.py), every case printing its worst error / bound ratio and the number of triggered / untriggered / near units:

  * synthetic unit tables with unit lengths 1, 3, 27 (rows that are not 16-byte aligned), 63 / 64 / 65, 255 / 256 / 257, 576, 1024 / 1025 (one wave
    owns a unit up to 1024 floats, the workgroup a longer one), 2048 / 2049, 4608, 5120 = L (the limit of the kernel's register-resident path),
    5121 = L + 1 and 20 011 (the loop path); many units in one table and tables of ONE unit; 4-
    and 12-byte gaps between the tensors, a ``clip_on = 0`` tensor, a 1-D tensor of one unit; the operands 0 and 1 float off a 16-byte boundary;
  * no global clip, the global clip hit in both forms, the first step, ``momentum = 0`` with a null ``mom``, ``clipping < 0`` (the bits of
    ``fb_mt_clip_sgd``), ``lr = 0``, all zeros, a zero-gradient unit and a zero-parameter unit (in every many-unit table);
  * the data alternate between units whose gradient norm is about 0.5 and about 4 times the trigger (0.25 and 2 once the global clip halves
    them): the float64 reference must count triggered AND untriggered units in every table (a table of one unit runs once with each);
  * SENTINEL in the gaps and behind n untouched in theta, grad and mom; the bits of grad unchanged unless the full-batch global clip hit;
  * two launches over the halves of a table = one launch over the whole, bit for bit; bad tables refused without a launch;
  * ResNet-18's own table on its arena of 11 174 016 floats (declared to tests/test_gpu_update_production.py through ``exercises``)."""
import pytest
import torch

from tests import adam_ref, agc_ref
from tests.helpers import SENTINEL, clip_coef_ref, f32r, within_bound
from tests.test_gpu_update_production import N18, exercises, mt

pytestmark = pytest.mark.gpu

FB_ERR_ARG = -1
PAD = 64
L = 5120                                    # AGC_L of csrc/agc_sgd.hip
HYP = dict(lr=0.1, weight_decay=2e-5, momentum=0.9, dampening=0.0, nesterov=True, clipping=0.01, eps=1e-3)
NAMES = ("theta", "grad", "mom")
KEYS = ("param", "grad", "mom")

#        (unit_len, n_units, clip_on), gap in floats behind the tensor
MANY = [((1, 5, 1), 3), ((3, 4, 1), 0), ((27, 64, 1), 1), ((63, 3, 1), 3), ((64, 3, 1), 0), ((65, 3, 1), 3), ((255, 2, 1), 1), ((256, 2, 1), 0),
        ((257, 2, 1), 3), ((576, 3, 1), 0), ((300, 1, 1), 0), ((1024, 5, 1), 0), ((1025, 2, 1), 3), ((2048, 2, 1), 0), ((2049, 2, 1), 3),
        ((4608, 3, 1), 0), ((L, 3, 1), 0), ((L + 1, 2, 1), 3), ((20011, 2, 1), 1), ((512, 4, 0), 0), ((1500, 2, 0), 1), ((7, 1, 1), 1)]
SINGLE = [1, 3, 27, 256, 576, 1024, 1025, 4608, L, L + 1, 20011]


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _rows(spec, start=0):
    rows, off = [], start
    for (unit_len, units, on), gap in spec:
        rows.append([off, unit_len, units, on])
        off += unit_len * units + gap
    return rows, off


def _carve(rows, n, off=0, seed=0, kind="random", scales=(0.5, 4.0)):
    """theta / grad / mom of n + PAD floats, each ``off`` floats behind a 256-byte boundary; SENTINEL in every element outside the units and behind
    n; unit k's gradient norm about scales[k % 2] times its trigger; unit 0 with a zero gradient, unit 1 with zero parameters (from 3 units on)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    uid, lens, _, _ = agc_ref.unit_ids(rows, n, "cuda")
    cov = uid >= 0
    sc = torch.tensor(scales, device="cuda")[uid.clamp(min=0) % 2]
    out = {}
    for name in NAMES:
        base = torch.empty(n + PAD + 8, device="cuda", dtype=torch.float32)
        assert base.data_ptr() % 256 == 0
        t = base[off:off + n + PAD]
        t[:n].normal_(generator=gen).mul_(0.1)
        if name == "grad":
            t[:n] *= HYP["clipping"] * sc
        if name == "mom":
            t[:n] *= 0.01
        if kind == "zeros":
            t[:n] = 0
        elif lens.numel() >= 3:
            if name == "grad":
                t[:n][uid == 0] = 0
            if name == "theta":
                t[:n][uid == 1] = 0
        t[:n][~cov] = SENTINEL
        t[n:] = SENTINEL
        out[name] = t
    return out


def _tab(rows):
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


def _launch(ops, n, tab, gnorm2, clip, hyp, first, call=None):
    mom = None if hyp["momentum"] == 0 else ops["mom"].data_ptr()
    args = (ops["theta"].data_ptr(), ops["grad"].data_ptr(), mom, n, None if gnorm2 is None else gnorm2.data_ptr(), -1.0 if clip is None else float(clip),
            1 if hyp.get("torch_clip") else 0, hyp["lr"], hyp["weight_decay"], hyp["momentum"], hyp["dampening"], 1 if hyp["nesterov"] else 0,
            1 if first else 0, -1.0 if hyp["clipping"] is None else hyp["clipping"], hyp["eps"], tab.data_ptr(), tab.shape[0])
    if call is None:
        _lib().call("fb_mt_agc_sgd", *args)
    else:
        call("fb_mt_agc_sgd", *args, n=n)


#                  state kind  global clip: None | factor of the norm   hyp overrides        first
CASES = {
    "no-clip": ("random", None, {}, False),
    "clip-hit": ("random", 0.5, {}, False),
    "clip-hit-torch-form": ("random", 0.5, dict(torch_clip=True), False),
    "clip-far-above-norm": ("random", 100.0, {}, False),
    "first-step": ("random", None, {}, True),
    "momentum-0-null-mom": ("random", None, dict(momentum=0.0, nesterov=False), False),
    "dampening-no-nesterov": ("random", 0.5, dict(dampening=0.1, nesterov=False), False),
    "unit-clip-off": ("random", 0.5, dict(clipping=None), False),
    "lr-0": ("random", None, dict(lr=0.0), False),
    "all-zeros": ("zeros", None, {}, False),
}


def _gnorm2(ops, rows, n):
    uid = agc_ref.unit_ids(rows, n, "cuda")[0]
    return ops["grad"][:n][uid >= 0].double().pow(2).sum().float().reshape(1)


def _check(rows, n, case, off=0, scales=(0.5, 4.0), both=True, call=None, label=""):
    kind, clip_rel, over, first = CASES[case]
    hyp = dict(HYP, **over)
    ops = _carve(rows, n, off, kind=kind, scales=scales)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = _gnorm2(ops, rows, n)
    clip = None if clip_rel is None else f32r(clip_rel * float(gnorm2) ** 0.5)
    tab = _tab(rows)
    _launch(ops, n, tab, gnorm2, clip, hyp, first, call)
    torch.cuda.synchronize()
    coef, hit = (adam_ref.torch_clip_coef_ref if hyp.get("torch_clip") else clip_coef_ref)(float(gnorm2), clip)
    ref = agc_ref.agc_ref(before["theta"][:n], before["grad"][:n], before["mom"][:n], rows, coef, hit, hyp, first)
    trig, clipped, near = int(ref["triggered"].sum()), int(ref["clipped"].sum()), int(ref["near"].sum())
    uid = agc_ref.unit_ids(rows, n, "cuda")[0]
    for name, key in zip(NAMES, KEYS):
        if key not in ref:                       # momentum 0: mom is not an operand
            assert torch.equal(ops[name].view(torch.int32), before[name].view(torch.int32))
            continue
        worst, where = within_bound(ops[name][:n], *ref[key])
        print(f"[agc_sgd {label} n={n} off={off} {case}] {name}: worst error / bound {worst:.3f} at {where}; units triggered {trig}, not {clipped - trig}, near {near}")
        assert worst <= 1.0, (name, worst, where)
        assert bool((ops[name][:n][uid < 0] == SENTINEL).all()) and bool((ops[name][n:] == SENTINEL).all()), name
    if both and hyp["clipping"] is not None and kind != "zeros":
        assert trig > 0 and clipped - trig > 0, (trig, clipped)
    g_same = torch.equal(ops["grad"].view(torch.int32), before["grad"].view(torch.int32))
    full_batch_hit = hit and not hyp.get("torch_clip")
    assert g_same != full_batch_hit              # the bits of the gradient unless the full-batch global clip hit
    if "far-above" in case:
        assert not hit
    if case.startswith("clip-hit"):
        assert hit and coef < 0.6
    if case == "lr-0":
        assert torch.equal(ops["theta"].view(torch.int32), before["theta"].view(torch.int32)) and not torch.equal(ops["mom"], before["mom"])
    elif case == "all-zeros":
        cov = uid >= 0
        assert all(not bool(ops[k][:n][cov].view(torch.int32).any()) for k in NAMES)       # +0 everywhere
    else:
        assert float((ops["theta"][:n] - before["theta"][:n]).abs().max()) > 0
    return ops, before, gnorm2, clip, hyp


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("off", [0, 1])
def test_agc_sgd_against_float64_many_units(off, case):
    rows, n = _rows(MANY, start=0 if off == 0 else 2)
    ops, before, gnorm2, clip, hyp = _check(rows, n + 5, case, off, label="many")
    if case == "unit-clip-off":                  # clipping < 0: fb_mt_clip_sgd over every tensor's range, bit for bit
        want = {k: v.clone() for k, v in before.items()}
        for o, unit_len, units, _ in rows:
            _lib().call("fb_mt_clip_sgd", want["theta"].data_ptr() + 4 * o, want["grad"].data_ptr() + 4 * o, want["mom"].data_ptr() + 4 * o, unit_len * units,
                        gnorm2.data_ptr(), clip, hyp["lr"], hyp["weight_decay"], hyp["momentum"], hyp["dampening"], 1 if hyp["nesterov"] else 0, 0)
        torch.cuda.synchronize()
        for k in NAMES:
            assert torch.equal(ops[k].view(torch.int32), want[k].view(torch.int32)), k


@pytest.mark.parametrize("case", ["no-clip", "clip-hit", "clip-hit-torch-form", "first-step"])
@pytest.mark.parametrize("unit_len", SINGLE)
def test_agc_sgd_against_float64_one_unit(unit_len, case):
    """A table of ONE unit, 1 float off a 16-byte boundary, once with a gradient far below the trigger and once far above it (the next test holds
    that the two scales do land on either side)."""
    for scale in (0.25, 8.0):
        _check([[1, unit_len, 1, 1]], unit_len + 3, case, 1, scales=(scale, scale), both=False, label=f"one unit x {scale}")


def test_agc_sgd_one_unit_tables_take_both_branches():
    """The two data scales of the one-unit test above do put the unit on either side of the trigger, for every length from 27 on."""
    for unit_len in [u for u in SINGLE if u >= 27]:
        got = []
        for scale in (0.25, 8.0):
            rows = [[1, unit_len, 1, 1]]
            ops = _carve(rows, unit_len + 3, 1, scales=(scale, scale))
            ref = agc_ref.agc_ref(ops["theta"][:unit_len + 3], ops["grad"][:unit_len + 3], ops["mom"][:unit_len + 3], rows, 1.0, False, HYP, False)
            got.append(int(ref["triggered"].sum()))
        assert got == [0, 1], (unit_len, got)


@pytest.mark.parametrize("case", ["no-clip", "clip-hit"])
def test_agc_sgd_split_table_equals_one_launch(case):
    kind, clip_rel, over, first = CASES[case]
    rows, n = _rows(MANY)
    whole, halves = _carve(rows, n), _carve(rows, n)
    assert all(torch.equal(whole[k], halves[k]) for k in NAMES)
    gnorm2 = _gnorm2(whole, rows, n)
    clip = None if clip_rel is None else f32r(clip_rel * float(gnorm2) ** 0.5)
    half = len(rows) // 2
    _launch(whole, n, _tab(rows), gnorm2, clip, HYP, first)
    _launch(halves, n, _tab(rows[:half]), gnorm2, clip, HYP, first)
    _launch(halves, n, _tab(rows[half:]), gnorm2, clip, HYP, first)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(whole[k].view(torch.int32), halves[k].view(torch.int32)), k
    # and a tensor's units as separate rows: the same bits again (the sums depend on the unit's length alone)
    units = _carve(rows, n)
    split = [[o + k * unit_len, unit_len, 1, on] for o, unit_len, cnt, on in rows for k in range(cnt)]
    _launch(units, n, _tab(split), gnorm2, clip, HYP, first)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(whole[k].view(torch.int32), units[k].view(torch.int32)), k


def test_agc_sgd_refuses_bad_tables_without_a_launch():
    lib = _lib()
    h = lib.load()
    rows, n = _rows(MANY)
    ops = _carve(rows, n)
    before = {k: v.clone() for k, v in ops.items()}
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [ops[k].data_ptr() for k in NAMES]
    #       n  gnorm2 clip torch lr   wd    mu   damp nest first clipping eps
    good = [n, None, -1.0, 0, 0.1, 2e-5, 0.9, 0.0, 1, 0, 0.01, 1e-3]
    bad_tables = {
        "unsorted": [rows[1], rows[0]] + rows[2:],
        "overlapping": [rows[0], [rows[0][0] + 2, 3, 4, 1]],
        "behind n": [[n - 10, 11, 1, 1]],
        "units behind n": [[0, 27, n // 27 + 1, 1]],
        "unit_len 0": [[0, 0, 4, 1]],
        "n_units 0": [[0, 4, 0, 1]],
        "negative offset": [[-4, 4, 1, 1]],
    }
    keep = []
    for what, table in bad_tables.items():
        tab = _tab(table)
        keep.append(tab)
        assert h.fb_mt_agc_sgd(*ptrs, *good, tab.data_ptr(), tab.shape[0], stream) == FB_ERR_ARG, what
        assert b"fb_mt_agc_sgd" in h.fb_last_error_string()
    tab = _tab(rows)
    assert h.fb_mt_agc_sgd(*ptrs, *good, tab.data_ptr(), 1025, stream) == FB_ERR_ARG            # more rows than the kernel's prefix table holds
    assert h.fb_mt_agc_sgd(*ptrs, *good, None, len(rows), stream) == FB_ERR_ARG
    torch.cuda.synchronize()
    assert all(torch.equal(ops[k].view(torch.int32), before[k].view(torch.int32)) for k in NAMES)     # nothing was launched
    assert h.fb_mt_agc_sgd(*ptrs, *good, tab.data_ptr(), len(rows), stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(ops["theta"], before["theta"])


def test_agc_sgd_through_a_recorded_command_list():
    """Recordable: the call replayed by the native executor gives the bits of the direct call."""
    lib = _lib()
    rows, n = _rows(MANY)
    want, ops = _carve(rows, n), _carve(rows, n)
    before = {k: v.clone() for k, v in ops.items()}
    gnorm2 = _gnorm2(ops, rows, n)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)
    tab = _tab(rows)
    _launch(want, n, tab, gnorm2, clip, HYP, False)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        _launch(ops, n, tab, gnorm2, clip, HYP, False)
    cl = rec.finish()
    for k in NAMES:
        ops[k].copy_(before[k])
    cl.replay(streams)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(ops[k].view(torch.int32), want[k].view(torch.int32)), k
    assert not torch.equal(ops["grad"], before["grad"])


def _resnet18_rows():
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Plan, agc_unit_rows
    from fullbatchtraining_amd.models import construct_model
    plan = Plan(construct_model(compose(["model=resnet18", "model.stem=CIFAR"]).model, 3, 10), 32)
    assert plan.n_params == N18
    return agc_unit_rows(plan), plan.P


@exercises("fb_mt_agc_sgd")
@pytest.mark.parametrize("case", ["no-clip", "clip-hit", "clip-hit-torch-form"])
def test_agc_sgd_at_production_size(case):
    """ResNet-18's own unit table (62 tensors, 4 851 units of 27 to 4 608 floats) on its arena of P = 11 174 016 floats."""
    rows, P = _resnet18_rows()
    assert P == 11_174_016 >= N18 and sum(r[2] for r in rows) == 4851
    _check(rows, P, case, call=mt, label="resnet18")
