"""AdamW (``hyp/optim=adam``), host side: the float64 reference of ``fb_mt_adamw`` (tests/adam_ref.py) against torch's own AdamW, its
elementwise bounds shown to bite (an fp32 emulation of the kernel passes, five planted errors fail), the preset, the state containers,
the scope checks and the entry point in the library's table."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from fullbatchtraining_amd.cfg import compose
from tests import adam_ref
from tests.helpers import clip_coef_ref, f32r, within_bound

HERE = os.path.dirname(os.path.abspath(__file__))
FB_ERR_ARG = -1
F32, F64 = torch.float32, torch.float64
HYP = dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)


def _state(n=4099, seed=0, zero=False):
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.01
    m, v = torch.randn(n, generator=gen) * 0.01, (torch.randn(n, generator=gen) * 0.01).pow(2)
    if zero:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


def test_reference_is_torch_adamw_in_float64():
    """Three steps of ``torch.optim.AdamW`` (float64, CPU, single-tensor form) with a new gradient each: parameters and both moments to 1e-12."""
    hyp = dict(lr=3e-3, weight_decay=0.05, betas=(0.8, 0.99), eps=1e-8)
    gen = torch.Generator().manual_seed(1)
    p = torch.nn.Parameter(torch.randn(257, generator=gen, dtype=F64))
    opt = torch.optim.AdamW([p], lr=hyp["lr"], betas=hyp["betas"], eps=hyp["eps"], weight_decay=hyp["weight_decay"], amsgrad=False, foreach=False)
    mine, m, v = p.detach().clone(), torch.zeros(257, dtype=F64), torch.zeros(257, dtype=F64)
    for t in (1, 2, 3):
        g = torch.randn(257, generator=gen, dtype=F64) * 10.0 ** (-t)
        p.grad = g.clone()
        opt.step()
        out = adam_ref.adamw_ref(mine, g, m, v, 1.0, False, hyp, t, rounded=False)
        mine, m, v = out["param"][0], out["exp_avg"][0], out["exp_avg_sq"][0]
        st = opt.state[p]
        assert float(st["step"]) == t
        for got, want in ((mine, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert float(((got - want).abs() / want.abs().clamp(min=1e-300)).max()) < 1e-12
        assert torch.equal(out["grad"][0], g) and not bool(out["grad"][1].any())


def _cases():
    """(name, state, norm2, clip, hyp, t): every path of the kernel's arithmetic."""
    p, g, m, v = _state()
    norm2 = float(g.double().pow(2).sum().float())
    norm = norm2 ** 0.5
    return [
        ("no-clip-t7", (p, g, m, v), norm2, None, HYP, 7),
        ("t1-zero-state", _state(zero=True), norm2, None, HYP, 1),
        ("clip-hit", (p, g, m, v), norm2, f32r(0.5 * norm), HYP, 7),
        ("clip-hit-torch-form", (p, g, m, v), norm2, f32r(0.5 * norm), dict(HYP, torch_clip=True), 7),
        ("clip-far-above", (p, g, m, v), norm2, f32r(100 * norm), HYP, 7),
        ("lr-0", (p, g, m, v), norm2, None, dict(HYP, lr=0.0), 1),
        ("wd-0", (p, g, m, v), norm2, None, dict(HYP, weight_decay=0.0), 3),
    ]


def _coef(norm2, clip, hyp):
    return adam_ref.torch_clip_coef_ref(norm2, clip) if hyp.get("torch_clip") else clip_coef_ref(norm2, clip)


def _worst(got, ref):
    return {k: within_bound(got[k], *ref[k])[0] for k in ("param", "grad", "exp_avg", "exp_avg_sq")}


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_fp32_emulation_of_the_kernel_is_within_the_bounds(case):
    name, (p, g, m, v), norm2, clip, hyp, t = case
    coef, hit = _coef(norm2, clip, hyp)
    ref = adam_ref.adamw_ref(p, g, m, v, coef, hit, hyp, t)
    got = adam_ref.emulate_fp32(p, g, m, v, norm2, clip, hyp, t)
    worst = _worst(got, ref)
    print(name, worst)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert max(worst["param"], worst["exp_avg"]) > 0.01              # (the bounds are not slack by orders of magnitude)
    if name == "lr-0":
        assert torch.equal(got["param"], p) and not torch.equal(got["exp_avg"], m)
    if name == "clip-far-above" or hyp.get("torch_clip"):
        assert torch.equal(got["grad"], g)
    if name == "clip-hit":
        assert hit and not torch.equal(got["grad"], g)


@pytest.mark.parametrize("plant,fails", [("eps-inside-sqrt", "param"), ("no-bias-correction-2", "param"), ("decay-after-step", "param"),
                                         ("beta2-on-g", "exp_avg_sq"), ("other-clip-form", "grad")])
def test_planted_errors_exceed_the_bounds(plant, fails):
    p, g, m, v = _state()
    norm2 = float(g.double().pow(2).sum().float())
    clip = f32r(0.5 * norm2 ** 0.5)
    coef, hit = clip_coef_ref(norm2, clip)
    ref = adam_ref.adamw_ref(p, g, m, v, coef, hit, HYP, 7)
    assert max(_worst(adam_ref.emulate_fp32(p, g, m, v, norm2, clip, HYP, 7), ref).values()) <= 1.0
    worst = _worst(adam_ref.emulate_fp32(p, g, m, v, norm2, clip, HYP, 7, plant=plant), ref)
    print(plant, worst)
    assert worst[fails] > 1.0, worst


def test_the_other_clip_form_is_caught_at_the_edge_too():
    """|g| = 0.5 exactly, clip within 1e-6 above it: ``norm > clip`` does not scale, min(1, clip / (norm + 1e-6)) does (by 1 - 1e-6), and from
    zero state that is 10 bounds of exp_avg away; asked the torch form, the full-batch form is as far off."""
    p, g, m, v = _state(zero=True)
    norm2, clip = 0.25, f32r(0.5 + 5e-7)
    for torch_clip in (False, True):
        hyp = dict(HYP, torch_clip=torch_clip)
        coef, hit = _coef(norm2, clip, hyp)
        assert hit == torch_clip and (coef == 1.0) == (not torch_clip)
        ref = adam_ref.adamw_ref(p, g, m, v, coef, hit, hyp, 1)
        assert max(_worst(adam_ref.emulate_fp32(p, g, m, v, norm2, clip, hyp, 1), ref).values()) <= 1.0
        assert _worst(adam_ref.emulate_fp32(p, g, m, v, norm2, clip, hyp, 1, plant="other-clip-form"), ref)["exp_avg"] > 1.0


def test_denormal_second_moment_and_exact_zeros():
    """v' in the denormal range (|g| ~ 1e-21: eps decides the denominator) stays within the bounds; g = m = v = p = 0 gives exact zeros."""
    p, g, m, v = _state()
    g = g * 1e-19
    m, v = m * 1e-19, torch.full_like(v, 3e-42)
    ref = adam_ref.adamw_ref(p, g, m, v, 1.0, False, HYP, 7)
    assert 0 < float(ref["exp_avg_sq"][0].max()) < 1.2e-38
    got = adam_ref.emulate_fp32(p, g, m, v, 1.0, None, HYP, 7)
    assert all(w <= 1.0 for w in _worst(got, ref).values())
    z = torch.zeros(5)
    got = adam_ref.emulate_fp32(z, z, z, z, 1.0, None, HYP, 1)
    assert all(not bool(t.any()) for t in got.values())


# -------------------------------------------------------------------------------------------------------------------- golden runs --
SCENARIOS = ["adam_plain", "adam_clip_warm", "adam_reg_r18", "adam_sgd_mode"]


def test_golden_adam_scenarios_are_admissible():
    """The reference's own fp32 and float64 runs (tests/golden/scenarios_adam.npz) agree within 1e-3 on the losses and the parameter norm, and
    within HALF of the tolerance the engine tests judge the scenario at on every statistic -- ``judged_at`` for losses and parameter norm,
    max(judged_at, 1e-3) for every gradient norm -- at every recorded step; the figures in meta_adam.json are those of the arrays."""
    data = np.load(os.path.join(HERE, "golden", "scenarios_adam.npz"))
    with open(os.path.join(HERE, "golden", "meta_adam.json")) as handle:
        meta = json.load(handle)
    assert set(meta["scenarios"]) == set(SCENARIOS) and meta["spread_limit"] == 1e-3
    assert meta["judged_at"] == {"adam_plain": 2e-4, "adam_clip_warm": 2e-4, "adam_reg_r18": 3e-3, "adam_sgd_mode": 2e-4}
    assert not [k for k in data.files if "/chunk" in k or "/probe_state" in k]
    for name in SCENARIOS:
        tol, sc = meta["judged_at"][name], meta["scenarios"][name]
        assert "hyp/optim=adam" in sc["overrides"] and any(o.startswith("hyp.optim.lr=") for o in sc["overrides"])
        assert sc["shuffling_loader"] == (name == "adam_sgd_mode") == ("hyp=base_sgd" in sc["overrides"])
        keys = [str(k) for k in data[f"{name}@f64/stat_keys"]]
        assert ("preclip_gradnorm" in keys) == (name in ("adam_clip_warm", "adam_reg_r18"))
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
    # warm-up from lr 0: the reference's first two records are equal
    assert data["adam_clip_warm/stat/train_loss"][0] == data["adam_clip_warm/stat/train_loss"][1]
    assert set(meta["checkpoint"]["state0"]) == {"step", "exp_avg", "exp_avg_sq"} and meta["checkpoint"]["state0"]["step"] == {"tensor": [], "dtype": "torch.float32"}


# ------------------------------------------------------------------------------------------------------------ preset and containers --
def test_adam_preset_carries_the_reference_values():
    cfg = compose(["hyp=fb1", "hyp/optim=adam"])
    assert dict(cfg.hyp.optim) == dict(name="Adam", lr=0.001, betas=[0.9, 0.999], eps=1e-8, weight_decay=0.01, amsgrad=False)
    assert compose(["hyp=fb1"]).hyp.optim.name == "Gradient Descent"
    assert compose(["hyp=fbclip", "hyp/optim=adam", "hyp.optim.lr=0.0003"]).hyp.optim.lr == 0.0003
    with open(os.path.join(HERE, "golden", "meta_adam.json")) as handle:
        assert json.load(handle)["reference_preset"] == dict(cfg.hyp.optim)


def test_optim_interface_returns_adamw_and_schedules_it():
    from fullbatchtraining_amd.training import GradualWarmupScheduler, optim_interface
    cfg = compose(["hyp=fb1", "hyp/optim=adam", "hyp.steps=6", "hyp.warmup=2"])
    model = torch.nn.Linear(3, 2)
    optimizer, scheduler = optim_interface(model, cfg.hyp)
    assert type(optimizer) is torch.optim.AdamW and isinstance(scheduler, GradualWarmupScheduler) and optimizer._opt_called is True
    group = optimizer.param_groups[0]
    assert (group["lr"], tuple(group["betas"]), group["eps"], group["weight_decay"], group["amsgrad"]) == (0.0, (0.9, 0.999), 1e-8, 0.01, False)
    assert len(optimizer.param_groups) == 1 and group["initial_lr"] == 0.001
    seq = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # no "lr_scheduler.step() before optimizer.step()"
        for _ in range(4):
            seq.append(optimizer.param_groups[0]["lr"])
            scheduler.step()
    assert seq[0] == 0.0 and abs(seq[1] - 0.0005) < 1e-15 and abs(seq[2] - 0.001) < 1e-15 and 0 < seq[3] <= 0.001
    plain, sched = optim_interface(model, compose(["hyp=fb1", "hyp/optim=adam", "hyp.warmup=0"]).hyp)
    assert isinstance(sched, torch.optim.lr_scheduler.CosineAnnealingLR) and plain.param_groups[0]["lr"] == 0.001
    cfg.hyp.optim.name = "FISTA"
    with pytest.raises(NotImplementedError):
        optim_interface(model, cfg.hyp)


def test_check_scope_accepts_adam_in_both_branches():
    from fullbatchtraining_amd.training import _check_scope
    _check_scope(compose(["hyp=fb1", "hyp/optim=adam"]))
    _check_scope(compose(["hyp=gradreg", "hyp/optim=adam", "hyp.optim.lr=0.0003", "hyp.grad_noise.additive=0.1", "hyp.norm_bias.strength=0.1"]))
    _check_scope(compose(["hyp=base_sgd", "hyp/optim=adam", "hyp.grad_clip=0.5"]), branch="stochastic")


@pytest.mark.parametrize("over,needle", [
    (["hyp.optim.amsgrad=True"], "amsgrad"),
    (["hyp/optim_modification=SAM"], "Adam with optim_modification 'SAM'"),
    (["hyp/optim_modification=LARC"], "Adam with optim_modification 'LARC'"),
    (["hyp.only_linear_layers_weight_decay=True"], "Adam with only_linear_layers_weight_decay"),
])
def test_scope_checks_name_what_adam_does_not_cover(over, needle):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    for base, branch in ((["hyp=fb1"], "full-batch"), (["hyp=base_sgd"], "stochastic")):
        cfg = compose(base + ["hyp/optim=adam"] + over)
        with pytest.raises(NotImplementedError, match=re.escape(needle)):
            _check_scope(cfg, branch=branch)
        with pytest.raises(NotImplementedError, match=re.escape(needle)):
            optim_interface(torch.nn.Linear(2, 2), cfg.hyp)
    _check_scope(compose(["hyp=fb1"] + [o for o in over if "amsgrad" not in o]))          # (gradient descent keeps its scope)


def test_adam_is_refused_on_more_than_one_rank(monkeypatch):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    cfg = compose(["hyp=fb1", "hyp/optim=adam"])
    with pytest.raises(NotImplementedError, match="Adam on more than one rank"):
        _check_scope(cfg)
    with pytest.raises(NotImplementedError, match="gather_sharded_state"):
        optim_interface(torch.nn.Linear(2, 2), cfg.hyp)
    _check_scope(compose(["hyp=fb1"]))


def test_sync_and_load_keep_torch_adamw_state_layout():
    """``_sync_optimizer_state`` fills ``state[p]`` the way torch's own AdamW does after a step (float32 scalar ``step``, buffers shaped like p);
    a plain torch.optim.AdamW loads the resulting state_dict."""
    from fullbatchtraining_amd.training import _sync_optimizer_state, optim_interface

    class FakeEngine:
        adam_step = 3

        def __init__(self, model):
            self.model = model

        def adam_state(self):
            ps = list(self.model.parameters())
            return [torch.full_like(p, 0.5) for p in ps], [torch.full_like(p, 0.25) for p in ps], self.adam_step

    model = torch.nn.Linear(3, 2)
    optimizer, _ = optim_interface(model, compose(["hyp=fb1", "hyp/optim=adam"]).hyp)
    _sync_optimizer_state(FakeEngine(model), model, optimizer)
    own = torch.optim.AdamW(torch.nn.Linear(3, 2).parameters(), lr=0.001)
    for q in own.param_groups[0]["params"]:
        q.grad = torch.zeros_like(q)
    own.step()
    for p, q in zip(model.parameters(), own.param_groups[0]["params"]):
        mine, theirs = optimizer.state[p], own.state[q]
        assert set(mine) == set(theirs) == {"step", "exp_avg", "exp_avg_sq"}
        for key in mine:
            assert mine[key].dtype == theirs[key].dtype and mine[key].shape == theirs[key].shape, key
        assert float(mine["step"]) == 3.0 and float(mine["exp_avg"].flatten()[0]) == 0.5
    own.load_state_dict(optimizer.state_dict())
    assert float(own.state[own.param_groups[0]["params"][0]]["step"]) == 3.0
    engine = FakeEngine(model)
    engine.adam_step = 0                                            # nothing to expose before the first update
    fresh, _ = optim_interface(model, compose(["hyp=fb1", "hyp/optim=adam"]).hyp)
    _sync_optimizer_state(engine, model, fresh)
    assert len(fresh.state) == 0


# ---------------------------------------------------------------------------------------------------------------- entry table --
def test_entry_table_lists_fb_mt_adamw():
    from fullbatchtraining_amd import lib
    h = lib.load()
    assert lib.EXPECTED_ABI == 17 == h.fb_abi_version()
    table = {h.fb_entry_name(i).decode(): (h.fb_entry_sig(i).decode(), h.fb_entry_kind(i)) for i in range(h.fb_entry_count())}
    # the signature from the header's prototype, independently: one code per argument
    header = open(os.path.join(os.path.dirname(HERE), "include", "fb_engine.h")).read()
    proto = re.search(r"int fb_mt_adamw\((.*?)\);", header, re.S).group(1)
    code = {"float*": "p", "const float*": "p", "void*": "p", "int64_t": "l", "int32_t": "i", "float": "f"}
    args = [" ".join(a.split()[:-1]) for a in proto.replace("\n", " ").split(",")]
    assert args[-1] == "void*" and len(args) == 16
    assert table["fb_mt_adamw"] == ("i:" + "".join(code[a] for a in args), 2) and table["fb_mt_adamw"][0] == "i:pppplpfifffffffp"
    fn = h.fb_cmd_fn_id(b"fb_mt_adamw")
    assert fn >= 0 and h.fb_cmd_fn_nargs(fn) == 16 == len(lib._SIGS["fb_mt_adamw"])


def test_fb_mt_adamw_refuses_bad_arguments_without_a_device():
    from fullbatchtraining_amd import lib
    h = lib.load()
    #        n   gnorm2 clip torch lr   wd    b1   b2     eps   step_size bc2s
    good = (64, None, -1.0, 0, 1e-3, 0.01, 0.9, 0.999, 1e-8, 1e-2, 0.0316)
    def with_(i, x):
        a = list(good)
        a[i] = x
        return a
    for ptrs in ((None, 16, 16, 16), (16, None, 16, 16), (16, 16, None, 16), (16, 16, 16, None)):
        assert h.fb_mt_adamw(*ptrs, *good, None) == FB_ERR_ARG
    assert h.fb_mt_adamw(16, 16, 16, 16, *with_(2, 0.5), None) == FB_ERR_ARG             # a clip without the norm
    for i, x in ((6, 1.0), (6, -0.1), (7, 1.0), (7, float("nan")), (8, 0.0), (8, -1e-8), (10, 0.0), (10, -1.0), (0, -1)):
        assert h.fb_mt_adamw(16, 16, 16, 16, *with_(i, x), None) == FB_ERR_ARG, (i, x)
        assert b"fb_mt_adamw" in h.fb_last_error_string()
    assert h.fb_mt_adamw(16, 18, 16, 16, *good, None) == FB_ERR_ARG                       # not 4-byte aligned
    assert h.fb_mt_adamw(16, 16, 16, 16, *with_(0, 0), None) == 0                         # n = 0: nothing to do, nothing launched
