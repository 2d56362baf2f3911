"""GD-AGC (``hyp/optim=gd_agc``), host side: the float64 reference of ``fb_mt_agc_sgd`` (tests/agc_ref.py) against the reference's own ``SGD_AGC``
run in float64 (tests/golden/agc_optimizer.npz), its elementwise bounds shown to bite (an fp32 emulation of the kernel, summation order
included, passes; five planted errors fail), the preset, the state container, the scope checks, the unit tables of the supported models and
the entry point in the library's table."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from fullbatchtraining_amd.cfg import compose
from tests import adam_ref, agc_ref
from tests.helpers import clip_coef_ref, f32r, within_bound

HERE = os.path.dirname(os.path.abspath(__file__))
FB_ERR_ARG = -1
HYP = dict(lr=0.1, weight_decay=2e-5, momentum=0.9, dampening=0.0, nesterov=True, clipping=0.01, eps=1e-3)


def _units_of(shape):
    """The reference's ``unitwise_norm``, literally: a tensor that squeezes to <= 1-D is summed over its axis 0 (one norm per remaining index)."""
    return int(np.prod(shape)) // shape[0] if sum(1 for s in shape if s != 1) <= 1 else shape[0]


# ---------------------------------------------------------------------------------------------- the reference against the reference --
def test_reference_is_the_references_sgd_agc_in_float64():
    """Two steps of the reference's SGD_AGC (float64, recorded by tests/golden/make_golden_agc.py) on tensors [5,3,3,3], [1,4,1,1], [7], [4,6] and
    an unclipped ``linear.weight``; a zero-gradient unit, a zero-parameter unit (the eps floor), a unit 1e-9 below the trigger and one 1e-9
    above: parameters and momentum buffers to 1e-12, the triggered counts equal.  [1,4,1,1] squeezes to 1-D, so ``unitwise_norm`` sums it over
    axis 0 -- of the UNSQUEEZED tensor, an axis of length 1: the reference clips it per element (its own count says 14 clipped units: 5 + 4 + 1 +
    4), where [7] is one unit.  The table follows the reference's code, not the shape's look."""
    data = np.load(os.path.join(HERE, "golden", "agc_optimizer.npz"))
    names = [str(n) for n in data["names"]]
    hyp = dict(zip([str(k) for k in data["hyp_keys"]], [float(v) for v in data["hyp_values"]]))
    hyp["nesterov"] = bool(hyp["nesterov"])
    shapes = [data[f"p0/{i}"].shape for i in range(len(names))]
    assert shapes == [(5, 3, 3, 3), (1, 4, 1, 1), (7,), (4, 6), (3, 5)] and names[-1] == "linear.weight"
    rows, off = [], 0
    for name, shape in zip(names, shapes):
        numel, units = int(np.prod(shape)), _units_of(shape)
        rows.append([off, numel // units, units, 0 if name.startswith("linear") else 1])
        off += numel + 3                          # (gaps: elements of no unit keep their values)
    assert [r[2] for r in rows] == [5, 4, 1, 4, 3] and [r[3] for r in rows] == [1, 1, 1, 1, 0]

    def flat(prefix):
        out = torch.full((off,), 7.0, dtype=torch.float64)
        for i, r in enumerate(rows):
            out[r[0]:r[0] + r[1] * r[2]] = torch.from_numpy(data[f"{prefix}/{i}"]).reshape(-1)
        return out

    p, m = flat("p0"), None
    for t in (1, 2):
        g = flat(f"g{t}")
        out = agc_ref.agc_ref(p, g, m, rows, 1.0, False, hyp, t == 1, rounded=False)
        p, m = out["param"][0], out["mom"][0]
        cov = agc_ref.unit_ids(rows, off)[0] >= 0
        for got, want in ((p, flat(f"p{t}")), (m, flat(f"buf{t}"))):
            assert float(((got - want).abs() / want.abs().clamp(min=1e-300))[cov].max()) < 1e-12
        assert bool((p[~cov] == 7.0).all())          # elements of no unit keep their values
        assert [int(out["triggered"].sum()), int(out["clipped"].sum())] == [int(v) for v in data[f"triggered{t}"]]
        assert torch.equal(out["grad"][0], g) and not bool(out["grad"][1].any())
        if t == 1:
            trig = out["triggered"].tolist()
            assert trig[1] and not trig[2] and trig[3] and not trig[0]          # eps floor; just below; just above; the zero gradient
            assert out["near"].tolist()[:4] == [False, False, True, True]       # (1e-9 is inside the fp32 allowance of ~1e-6: an fp32 run may take either branch)
            assert not bool(out["triggered"][-3:].any()) and not bool(out["clipped"][-3:].any())   # linear.weight


# ------------------------------------------------------------------------------------------------------------------ the bounds bite --
SPEC = [(1, 4, 1), (3, 3, 1), (27, 6, 1), (64, 2, 1), (257, 2, 1), (576, 2, 1), (1025, 2, 1), (5121, 2, 1), (40, 1, 1), (12, 3, 0)]


def _state(seed=0, scales=(0.5, 4.0)):
    rows, off = [], 1
    for k, (unit_len, units, on) in enumerate(SPEC):
        rows.append([off, unit_len, units, on])
        off += unit_len * units + (1, 3, 0)[k % 3]
    n = off + 2
    gen = torch.Generator().manual_seed(seed)
    uid = agc_ref.unit_ids(rows, n)[0]
    sc = torch.tensor(scales)[uid.clamp(min=0) % 2]
    p, g, m = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1 * HYP["clipping"] * sc, torch.randn(n, generator=gen) * 1e-3
    g[uid == 0] = 0.0
    p[uid == 1] = 0.0
    p[uid == 8] = 0.0                             # a 27-float unit of zero parameters as well
    for t in (p, g, m):
        t[uid < 0] = 5.0
    return rows, n, p, g, m


def _cases():
    rows, n, p, g, m = _state()
    cov = agc_ref.unit_ids(rows, n)[0] >= 0
    norm2 = float(g[cov].double().pow(2).sum().float())
    norm = norm2 ** 0.5
    return [
        ("no-clip", None, HYP, False),
        ("first-step", None, HYP, True),
        ("clip-hit", f32r(0.5 * norm), HYP, False),
        ("clip-hit-torch-form", f32r(0.5 * norm), dict(HYP, torch_clip=True), False),
        ("clip-far-above", f32r(100 * norm), HYP, False),
        ("momentum-0", None, dict(HYP, momentum=0.0, nesterov=False), False),
        ("dampening", None, dict(HYP, dampening=0.1, nesterov=False), False),
        ("unit-clip-off", f32r(0.5 * norm), dict(HYP, clipping=None), False),
        ("lr-0", None, dict(HYP, lr=0.0), False),
    ], norm2


def _coef(norm2, clip, hyp):
    return adam_ref.torch_clip_coef_ref(norm2, clip) if hyp.get("torch_clip") else clip_coef_ref(norm2, clip)


def _worst(got, ref):
    return {k: within_bound(got[k], *ref[k])[0] for k in ("param", "grad", "mom") if k in ref}


@pytest.mark.parametrize("case", _cases()[0], ids=lambda c: c[0])
def test_fp32_emulation_of_the_kernel_is_within_the_bounds(case):
    name, clip, hyp, first = case
    rows, n, p, g, m = _state()
    norm2 = _cases()[1]
    coef, hit = _coef(norm2, clip, hyp)
    ref = agc_ref.agc_ref(p, g, m, rows, coef, hit, hyp, first)
    got = agc_ref.emulate_fp32(p, g, m, rows, norm2, clip, hyp, first)
    worst = _worst(got, ref)
    print(name, worst, "triggered", int(ref["triggered"].sum()), "of", int(ref["clipped"].sum()))
    assert all(w <= 1.0 for w in worst.values()), worst
    assert worst["param"] > 0.01 or name == "lr-0"                   # (the bounds are not slack by orders of magnitude)
    if hyp["clipping"] is not None:
        assert 0 < int(ref["triggered"].sum()) < int(ref["clipped"].sum())
    gaps = agc_ref.unit_ids(rows, n)[0] < 0
    assert all(bool((got[k][gaps] == 5.0).all()) for k in got)
    if name in ("clip-hit", "unit-clip-off"):    # the full-batch global clip hit: the globally clipped gradient is written back
        assert hit and not torch.equal(got["grad"], g)
    else:
        assert torch.equal(got["grad"], g)
    if name == "unit-clip-off":                  # plain SGD: the bounds of helpers.sgd_ref's kind, and nothing triggered
        assert not bool(ref["triggered"].any())


@pytest.mark.parametrize("plant,fails", [("whole-tensor-norm", "param"), ("trigger-ignored", "param"), ("no-eps-floor", "param"),
                                         ("agc-after-weight-decay", "param"), ("clipped-gradient-written-back", "grad")])
@pytest.mark.parametrize("clipped", [False, True], ids=["no-global-clip", "global-clip-hit"])
def test_planted_errors_exceed_the_bounds(plant, fails, clipped):
    rows, n, p, g, m = _state()
    norm2 = _cases()[1]
    clip = f32r(0.5 * norm2 ** 0.5) if clipped else None
    coef, hit = clip_coef_ref(norm2, clip)
    ref = agc_ref.agc_ref(p, g, m, rows, coef, hit, HYP, False)
    assert max(_worst(agc_ref.emulate_fp32(p, g, m, rows, norm2, clip, HYP, False), ref).values()) <= 1.0
    worst = _worst(agc_ref.emulate_fp32(p, g, m, rows, norm2, clip, HYP, False, plant=plant), ref)
    print(plant, worst)
    assert worst[fails] > 1.0, worst


def test_a_unit_at_the_trigger_is_covered_whichever_branch_is_taken():
    """|g| set to maxn (1 +- 2e-7) in fp32: inside the allowance on the factor, so the reference files the unit as near; the emulation (which takes
    whichever branch its fp32 sums say) and a copy forced onto the OTHER branch both stay within the bounds: the update is continuous there."""
    rows = [[0, 576, 4, 1]]
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(4 * 576, generator=gen) * 0.1
    g = torch.randn(4 * 576, generator=gen)
    for k, rel in enumerate((1 - 2e-7, 1 + 2e-7, 1 - 1e-3, 1 + 1e-3)):
        s = slice(576 * k, 576 * (k + 1))
        g[s] *= float(p[s].double().norm()) * f32r(0.01) * rel / float(g[s].double().norm())
    m = torch.zeros_like(p)
    ref = agc_ref.agc_ref(p, g, m, rows, 1.0, False, HYP, False)
    assert ref["near"].tolist() == [True, True, False, False] and ref["triggered"].tolist()[2:] == [False, True]
    got = agc_ref.emulate_fp32(p, g, m, rows, 1.0, None, HYP, False)
    assert max(_worst(got, ref).values()) <= 1.0
    forced = agc_ref.emulate_fp32(p, g, m, rows, 1.0, None, HYP, False, plant="trigger-ignored")
    near = slice(0, 2 * 576)
    for k in ("param", "mom"):
        assert within_bound(forced[k][near], ref[k][0][near], ref[k][1][near])[0] <= 1.0
    far = slice(2 * 576, 3 * 576)                # the unit 1e-3 below the trigger is NOT covered when the trigger is ignored
    assert within_bound(forced["param"][far], ref["param"][0][far], ref["param"][1][far])[0] > 1.0


def test_exact_zeros_stay_zero():
    z = torch.zeros(64)
    got = agc_ref.emulate_fp32(z, z, z, [[0, 16, 4, 1]], 0.0, None, HYP, False)
    assert all(not bool(t.any()) for t in got.values())
    ref = agc_ref.agc_ref(z, z, z, [[0, 16, 4, 1]], 1.0, False, HYP, False)
    assert not bool(ref["triggered"].any()) and not bool(ref["param"][0].any())


def test_kernel_summation_order_is_a_function_of_the_length():
    """The emulated order: 64 lanes, chunks of four, the butterfly -- within sum_roundings(len) u of the float64 sum, for every length."""
    gen = torch.Generator().manual_seed(5)
    for n in (1, 3, 27, 255, 256, 257, 1024, 1025, 4608, 5120, 5121, 20011):
        x = (torch.randn(n, generator=gen) * 0.1).numpy()
        want = float((x.astype(np.float64) ** 2).sum())
        assert abs(float(agc_ref.kernel_sumsq(x)) - want) <= agc_ref.sum_roundings(n) * 2.0 ** -24 * want
    assert agc_ref.sum_roundings(27) == 10 and agc_ref.sum_roundings(1024) == 22 and agc_ref.sum_roundings(1025) == 17 and agc_ref.sum_roundings(4608) == 29


# -------------------------------------------------------------------------------------------------------------------- golden runs --
SCENARIOS = ["agc_plain", "agc_clip_warm", "agc_reg_r18", "agc_sgd_mode"]


def test_golden_agc_scenarios_are_admissible():
    """The rule of tests/golden/make_golden_adam.py on tests/golden/scenarios_agc.npz: the reference's own fp32 and float64 runs agree within 1e-3
    on the losses and the parameter norm and within HALF of the tolerance the engine tests judge the scenario at on every statistic; both
    branches of the unit clip occur on every trajectory; the figures in meta_agc.json are those of the arrays."""
    data = np.load(os.path.join(HERE, "golden", "scenarios_agc.npz"))
    with open(os.path.join(HERE, "golden", "meta_agc.json")) as handle:
        meta = json.load(handle)
    assert set(meta["scenarios"]) == set(SCENARIOS) and meta["spread_limit"] == 1e-3
    assert meta["judged_at"] == {"agc_plain": 2e-4, "agc_clip_warm": 2e-4, "agc_reg_r18": 3e-3, "agc_sgd_mode": 2e-4}
    assert not [k for k in data.files if "/chunk" in k or "/probe_state" in k]
    for name in SCENARIOS:
        tol, sc = meta["judged_at"][name], meta["scenarios"][name]
        assert "hyp/optim=gd_agc" in sc["overrides"] and any(o.startswith("hyp.optim.lr=") for o in sc["overrides"])
        assert sc["shuffling_loader"] == (name == "agc_sgd_mode") == ("hyp=base_sgd" in sc["overrides"])
        keys = [str(k) for k in data[f"{name}@f64/stat_keys"]]
        assert ("preclip_gradnorm" in keys) == (name in ("agc_clip_warm", "agc_reg_r18"))
        worst_chunk = 0.0
        for stat in keys:
            r32, r64 = data[f"{name}/stat/{stat}"], data[f"{name}@f64/stat/{stat}"]
            if stat in ("train_acc", "clipped_step"):
                assert np.array_equal(r32, r64), (name, stat)
                continue
            if stat.startswith("valid_"):        # (one evaluation at the end; the engine tests only ask that it is finite)
                continue
            spread = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
            if stat.startswith("grad_norm_train_"):
                worst_chunk = max(worst_chunk, spread)
                continue
            limit = max(tol, 1e-3) / 2 if stat in ("grad_norm", "preclip_gradnorm") else min(tol / 2, 1e-3)
            assert spread < limit and abs(spread - meta["spread"][name][stat]) <= 1e-12, (name, stat, spread)
        assert worst_chunk < max(tol, 1e-3) / 2 and abs(worst_chunk - meta["spread"][name]["grad_norm_train_max"]) <= 1e-12, (name, worst_chunk)
        runs = meta["final_rel_l2_fp32_runs"][name]
        assert set(runs) == {"8", "2", "1"} and runs["8"] == meta["spread"][name]["final_rel_l2"]
        assert meta["final_rel_l2_bound"][name] == 5 * max(runs.values()) < 5e-3
        trig = meta["triggered_units"][name]
        assert trig and any(h > 0 for h, _ in trig) and any(h < n for h, n in trig), (name, trig)
        assert all(n == (4851 if name == "agc_reg_r18" else 3189) for _, n in trig)
    assert data["agc_clip_warm/stat/train_loss"][0] == data["agc_clip_warm/stat/train_loss"][1]      # warm-up from lr 0
    assert set(meta["checkpoint"]["state0"]) == {"momentum_buffer"} and meta["checkpoint"]["optimizer"] == "SGD_AGC"


# ------------------------------------------------------------------------------------------------------------ preset and containers --
def test_gd_agc_preset_carries_the_reference_values():
    cfg = compose(["hyp=fb1", "hyp/optim=gd_agc"])
    assert dict(cfg.hyp.optim) == dict(name="GD-AGC", lr=1.6, momentum=0.9, weight_decay=2e-5, dampening=0.0, nesterov=True, clipping=0.01, eps=1e-3)
    assert "line_search" not in cfg.hyp.optim
    assert compose(["hyp=fb1"]).hyp.optim.name == "Gradient Descent"
    assert compose(["hyp=fbclip", "hyp/optim=gd_agc", "hyp.optim.lr=0.03"]).hyp.optim.lr == 0.03
    with open(os.path.join(HERE, "golden", "meta_agc.json")) as handle:
        assert json.load(handle)["reference_preset"] == dict(cfg.hyp.optim)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3, bias=False)
        self.linear = torch.nn.Linear(4, 2)
        self.fc = torch.nn.Linear(4, 2)


def test_optim_interface_returns_the_state_container_and_schedules_it():
    from fullbatchtraining_amd.training import SGD_AGC, GradualWarmupScheduler, optim_interface
    cfg = compose(["hyp=fb1", "hyp/optim=gd_agc", "hyp.steps=6", "hyp.warmup=2"])
    model = _Net()
    optimizer, scheduler = optim_interface(model, cfg.hyp)
    assert type(optimizer) is SGD_AGC and isinstance(scheduler, GradualWarmupScheduler) and optimizer._opt_called is True
    groups = optimizer.param_groups
    assert [g["name"] for g in groups] == ["conv.weight", "linear.weight", "linear.bias", "fc.weight", "fc.bias"]
    assert [g["clipping"] for g in groups] == [0.01, None, None, 0.01, 0.01]                # the linear* rule; the engine's classifier `fc` IS clipped
    for g in groups:
        assert len(g["params"]) == 1
        assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["eps"], g["initial_lr"]) == (0.0, 0.9, 0.0, 2e-5, True, 1e-3, 1.6)
    seq = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # no "lr_scheduler.step() before optimizer.step()"
        for _ in range(4):
            seq.append([g["lr"] for g in groups])
            scheduler.step()
    assert all(len(set(s)) == 1 for s in seq)
    seq = [s[0] for s in seq]
    assert seq[0] == 0.0 and abs(seq[1] - 0.8) < 1e-12 and abs(seq[2] - 1.6) < 1e-12 and 0 < seq[3] <= 1.6
    with pytest.raises(RuntimeError, match="state container"):
        optimizer.step()
    plain, sched = optim_interface(model, compose(["hyp=fb1", "hyp/optim=gd_agc", "hyp.warmup=0"]).hyp)
    assert isinstance(sched, torch.optim.lr_scheduler.CosineAnnealingLR) and plain.param_groups[0]["lr"] == 1.6
    for other in ("FISTA", "L-BFGS", "Adaptive Gradient Descent"):
        cfg.hyp.optim.name = other
        with pytest.raises(NotImplementedError):
            optim_interface(model, cfg.hyp)


def test_check_scope_accepts_gd_agc_in_both_branches():
    from fullbatchtraining_amd.training import _check_scope
    _check_scope(compose(["hyp=fb1", "hyp/optim=gd_agc"]))
    _check_scope(compose(["hyp=gradreg", "hyp/optim=gd_agc", "hyp.optim.lr=0.03", "hyp.grad_noise.additive=0.1", "hyp.norm_bias.strength=0.1"]))
    _check_scope(compose(["hyp=base_sgd", "hyp/optim=gd_agc", "hyp.grad_clip=0.5"]), branch="stochastic")


@pytest.mark.parametrize("over,needle", [
    (["hyp/optim_modification=SAM"], "GD-AGC with optim_modification 'SAM'"),
    (["hyp/optim_modification=LARC"], "GD-AGC with optim_modification 'LARC'"),
    (["hyp.only_linear_layers_weight_decay=True"], "GD-AGC with only_linear_layers_weight_decay"),
])
def test_scope_checks_name_what_gd_agc_does_not_cover(over, needle):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    for base, branch in ((["hyp=fb1"], "full-batch"), (["hyp=base_sgd"], "stochastic")):
        cfg = compose(base + ["hyp/optim=gd_agc"] + over)
        with pytest.raises(NotImplementedError, match=re.escape(needle)):
            _check_scope(cfg, branch=branch)
        with pytest.raises(NotImplementedError, match=re.escape(needle)):
            optim_interface(_Net(), cfg.hyp)
    _check_scope(compose(["hyp=fb1"] + over))                       # (gradient descent keeps its scope)


def test_gd_agc_is_refused_on_more_than_one_rank(monkeypatch):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    cfg = compose(["hyp=fb1", "hyp/optim=gd_agc"])
    with pytest.raises(NotImplementedError, match="GD-AGC on more than one rank"):
        _check_scope(cfg)
    with pytest.raises(NotImplementedError, match="cut through units"):
        optim_interface(_Net(), cfg.hyp)
    _check_scope(compose(["hyp=fb1"]))


def test_checkpoint_round_trip_in_the_recorded_layout(tmp_path):
    """``_save_to_checkpoint`` / ``_load_from_checkpoint`` with the container: the optimizer part has the key structure the generator recorded
    from the reference's own checkpoint (one group per tensor with its name, ``momentum_buffer`` state), and the momentum comes back."""
    from fullbatchtraining_amd.training import _load_from_checkpoint, _save_to_checkpoint, optim_interface
    with open(os.path.join(HERE, "golden", "meta_agc.json")) as handle:
        recorded = json.load(handle)["checkpoint"]

    class FakeEngine:
        first_step = False
        loaded = None

        def __init__(self, model):
            self.model = model

        def store_to_model(self, model):
            pass

        def load_from_model(self, model):
            pass

        def momentum_state(self):
            return [torch.full_like(p, 0.5 + i) for i, p in enumerate(self.model.parameters())]

        def load_momentum(self, bufs):
            self.loaded = [b.clone() for b in bufs]

    class Counter:
        step = 3

    cfg = compose(["hyp=fb1", "hyp/optim=gd_agc", "hyp.warmup=2"])
    model = _Net()
    optimizer, scheduler = optim_interface(model, cfg.hyp)
    path = str(tmp_path / "ck.pth")
    _save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=path, engine=FakeEngine(model))
    optim_state = torch.load(path, weights_only=False)[0]
    groups = optim_state["param_groups"]
    assert len(groups) == 5 and [g["name"] for g in groups] == [n for n, _ in model.named_parameters()]
    mine0 = adam_ref.describe(groups[0])
    assert set(mine0) == set(recorded["group0"]), (set(mine0) ^ set(recorded["group0"]))
    assert {k: type(v) for k, v in mine0.items() if k not in ("name", "params", "lr", "initial_lr")} == \
        {k: type(v) for k, v in recorded["group0"].items() if k not in ("name", "params", "lr", "initial_lr")}
    assert set(adam_ref.describe(optim_state["state"][0])) == set(recorded["state0"]) == {"momentum_buffer"}
    assert len(optim_state["state"]) == 5 and recorded["n_state"] == recorded["n_groups"]
    fresh_model = _Net()
    fresh, fresh_sched = optim_interface(fresh_model, cfg.hyp)
    engine = FakeEngine(fresh_model)
    counter = Counter()
    counter.step = 0
    _load_from_checkpoint(fresh_model, fresh, fresh_sched, None, counter, 10, file=path, engine=engine)
    assert counter.step == 3 and [float(b.flatten()[0]) for b in engine.loaded] == [0.5, 1.5, 2.5, 3.5, 4.5]
    assert [g["clipping"] for g in fresh.param_groups] == [0.01, None, None, 0.01, 0.01]


# ------------------------------------------------------------------------------------------------------------------- unit tables --
@pytest.mark.parametrize("model,units", [("resnet18", 4851), ("resnet20", 3189), ("resnet50", None)])
def test_unit_table_covers_every_parameter_once_and_no_padding(model, units):
    import math

    from fullbatchtraining_amd.engine import Plan, agc_unit_rows
    from fullbatchtraining_amd.models import construct_model
    net = construct_model(compose([f"model={model}"]).model, 3, 10)
    plan = Plan(net, 32)
    rows = agc_unit_rows(plan)
    assert len(rows) == len(plan.param_names) and rows == sorted(rows)
    count = torch.zeros(plan.P, dtype=torch.int32)
    is_param = torch.zeros(plan.P, dtype=torch.bool)
    want_units = 0
    for (off, unit_len, n_units, on), name in zip(rows, plan.param_names):
        shape = plan.param_shapes[name]
        assert off == plan.offsets[name] and unit_len * n_units == math.prod(shape) and on == 1
        assert n_units == _units_of(shape) and (n_units == shape[0] or (n_units == 1 and len(shape) == 1))
        for k in range(n_units):
            count[off + k * unit_len:off + (k + 1) * unit_len] += 1
        is_param[off:off + math.prod(shape)] = True
        want_units += n_units
    assert int(is_param.sum()) == plan.n_params < plan.P
    assert bool((count[is_param] == 1).all()) and not bool(count[~is_param].any())
    assert sum(r[2] for r in rows) == want_units and (units is None or want_units == units)
    if model == "resnet50":
        assert plan.kind != "basic" and max(r[1] for r in rows) == 4608
    # the reference's own rule on the tensors themselves: one norm per unit
    for (off, unit_len, n_units, _), (name, p) in zip(rows, net.named_parameters()):
        assert n_units == (p.sum(0).numel() if p.squeeze().dim() <= 1 else p.shape[0]), name


def test_unit_table_carries_the_linear_rule():
    from fullbatchtraining_amd.engine import agc_unit_rows

    class P:
        param_names = ["conv.weight", "linear.weight", "linear.bias", "gain"]
        param_shapes = {"conv.weight": (5, 3, 3, 3), "linear.weight": (4, 6), "linear.bias": (4,), "gain": (1, 4, 1, 1)}
        offsets = {"conv.weight": 0, "linear.weight": 136, "linear.bias": 160, "gain": 164}
    assert agc_unit_rows(P) == [[0, 27, 5, 1], [136, 6, 4, 0], [160, 4, 1, 0], [164, 1, 4, 1]]      # (a [1,4,1,1] tensor: per element, as the reference does)


# ---------------------------------------------------------------------------------------------------------------- entry table --
def test_entry_table_lists_fb_mt_agc_sgd():
    from fullbatchtraining_amd import lib
    h = lib.load()
    assert lib.EXPECTED_ABI == 17 == h.fb_abi_version()
    table = {h.fb_entry_name(i).decode(): (h.fb_entry_sig(i).decode(), h.fb_entry_kind(i)) for i in range(h.fb_entry_count())}
    header = open(os.path.join(os.path.dirname(HERE), "include", "fb_engine.h")).read()
    proto = re.search(r"int fb_mt_agc_sgd\((.*?)\);", header, re.S).group(1)
    code = {"float*": "p", "const float*": "p", "const int64_t*": "p", "void*": "p", "int64_t": "l", "int32_t": "i", "float": "f"}
    args = [" ".join(a.split()[:-1]) for a in proto.replace("\n", " ").split(",")]
    assert args[-1] == "void*" and len(args) == 18
    assert table["fb_mt_agc_sgd"] == ("i:" + "".join(code[a] for a in args), 2) and table["fb_mt_agc_sgd"][0] == "i:ppplpfiffffiiffpip"
    fn = h.fb_cmd_fn_id(b"fb_mt_agc_sgd")
    assert fn >= 0 and h.fb_cmd_fn_nargs(fn) == 18 == len(lib._SIGS["fb_mt_agc_sgd"])


def test_fb_mt_agc_sgd_refuses_bad_arguments_without_a_device():
    from fullbatchtraining_amd import lib
    h = lib.load()
    #       n   gnorm2 clip torch lr   wd    mu   damp nest first clipping eps  table rows
    good = (64, None, -1.0, 0, 0.1, 2e-5, 0.9, 0.0, 1, 0, 0.01, 1e-3, 16, 0)

    def with_(i, x):
        a = list(good)
        a[i] = x
        return a
    for ptrs in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        assert h.fb_mt_agc_sgd(*ptrs, *good, None) == FB_ERR_ARG
        assert b"fb_mt_agc_sgd" in h.fb_last_error_string()
    assert h.fb_mt_agc_sgd(16, 16, None, *with_(6, 0.0), None) == 0                       # momentum 0: mom may be null
    assert h.fb_mt_agc_sgd(16, 16, 16, *with_(2, 0.5), None) == FB_ERR_ARG                # a global clip without the norm
    for i, x in ((0, -1), (13, -1), (13, 1025), (11, 0.0), (11, -1e-3), (11, float("nan"))):
        assert h.fb_mt_agc_sgd(16, 16, 16, *with_(i, x), None) == FB_ERR_ARG, (i, x)
        assert b"fb_mt_agc_sgd" in h.fb_last_error_string()
    a = with_(12, None)
    a[13] = 3
    assert h.fb_mt_agc_sgd(16, 16, 16, *a, None) == FB_ERR_ARG                            # rows without a table
    assert h.fb_mt_agc_sgd(16, 16, 16, *with_(12, 20), None) == FB_ERR_ARG                # the table is not 8-byte aligned
    assert h.fb_mt_agc_sgd(16, 18, 16, *good, None) == FB_ERR_ARG                         # not 4-byte aligned
    b = with_(10, -1.0)
    b[11] = 0.0
    assert h.fb_mt_agc_sgd(16, 16, 16, *b, None) == 0                                     # no unit clip: eps is not looked at; no rows: nothing launched
    assert h.fb_mt_agc_sgd(16, 16, 16, *good, None) == 0
