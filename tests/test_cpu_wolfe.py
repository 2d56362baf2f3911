"""CPU-side checks of ``hyp.optim.line_search=wolfe`` (the reference's ``WolfeGradientDescent``): the search controller replays every recorded
search of the reference exactly; the float32 restatement of the kernels reproduces recorded steps of the reference; scope and wiring; the
checkpoint layout; the entry-point table."""
import json
import os
import re

import numpy as np
import pytest
import torch

from fullbatchtraining_amd.cfg import compose
from tests import wolfe_ref
from tests.adam_ref import describe

HERE = os.path.dirname(os.path.abspath(__file__))
FB_ERR_ARG = -1
WOLFE = ["hyp=fb1", "hyp.optim.line_search=wolfe"]
EXITS = ("accepted at alpha = 1", "rule-1 zoom", "rule-2 zoom", "growth to alpha_max", "outer max_iter exhausted", "zoom 1e-4 exit",
         "zoom exhausted", "table hit", "ValueError", "phi'(0) > 0")


def _meta():
    with open(os.path.join(HERE, "golden", "meta_wolfe.json")) as handle:
        return json.load(handle)


# ------------------------------------------------------------------------------------------------------------------- the controller --
def _replay(key, info, data):
    from fullbatchtraining_amd.training import WolfeSearch
    evals = [tuple(float(v) for v in row) for row in data[f"{key}/evals"]]
    phi0 = [float(v) for v in data[f"{key}/phi0"]]
    todo = list(evals)
    ctl = WolfeSearch(**info["constants"])

    def evaluate(alpha):
        assert todo, f"{key}: the controller asks for alpha {alpha!r} after the reference's last evaluation"
        want = todo.pop(0)
        assert isinstance(alpha, float) and alpha == want[0], (key, alpha, want[0])
        return want[1], want[2]

    try:
        got, exc = ctl.search(phi0[0], phi0[1], evaluate), None
    except Exception as e:      # noqa: BLE001  (the type is what is compared)
        got, exc = None, type(e).__name__
    assert not todo, (key, "the controller stopped before the reference did", todo)
    return ctl, got, exc, evals


def test_controller_replays_every_recorded_search_of_the_reference_exactly():
    meta, data = _meta(), np.load(os.path.join(HERE, "golden", "wolfe_search.npz"))
    assert tuple(meta["coverage"]) == EXITS
    seen = set()
    for key, info in meta["search_cases"].items():
        ctl, got, exc, evals = _replay(key, info, data)
        assert exc == info["exception"], (key, exc)
        want = float(data[f"{key}/returned"][0])
        if exc is None:
            assert got == want, (key, got, want)                                  # the returned alpha, as Python floats
        else:
            assert np.isnan(want)
        assert ctl.evaluated == [e[0] for e in evals] and len(evals) == info["n_evals"]       # the same alphas in the same order ...
        assert (ctl.evaluated[-1] if ctl.evaluated else None) == (evals[-1][0] if evals else None)     # ... so the same last evaluated one
        assert (got in ctl.evaluated) == info["returned_is_evaluated"], key
        assert (ctl.exit, ctl.zoom_exit, ctl.table_hits) == (info["outer_exit"], info["zoom_exit"], info["table_hits"]) or exc is not None, key
        seen |= set(info["exits"])
    assert seen == set(EXITS), set(EXITS) - seen


def test_controller_quirks_of_the_reference():
    """The ones the issue names: a zoom that runs out of rounds returns an alpha that was never evaluated; a table hit spares the evaluation;
    ``prev_loss`` is never updated (a loss that rises against the previous trial does not zoom); the defaults."""
    from fullbatchtraining_amd.training import WOLFE_DEFAULTS, WolfeSearch
    meta = _meta()
    assert WOLFE_DEFAULTS == meta["reference_defaults"] == dict(c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10)
    ctl = WolfeSearch()
    assert (ctl.c1, ctl.c2, ctl.alpha_max, ctl.max_iter) == (1e-4, 0.9, 10.0, 10)
    cases = meta["search_cases"]
    assert cases["uphill/1"]["zoom_exit"] == "exhausted" and not cases["uphill/1"]["returned_is_evaluated"]
    assert cases["hit_stationary/0"]["table_hits"] == 10 and cases["hit_stationary/0"]["n_evals"] == 1
    # phi decreasing in value at 1 and 2.5 but higher at 2.5 than at 1, slopes still steep and negative: the reference grows on
    table = {1.0: (0.5, -1.0), 2.5: (0.6, -1.0), 6.25: (0.1, -1.0)}
    assert ctl.search(1.0, -1.0, lambda a: table[a]) == 10.0 and ctl.evaluated == [1.0, 2.5, 6.25] and ctl.exit == "alpha_max"
    with pytest.raises(ValueError):          # quotient -0.9, d_1 = 0.7: d_1^2 - phi'(0) phi'(1) = 0.49 - 1 < 0
        WolfeSearch._interpolate(0, 1.0, {0: dict(val=0.0, grad=-1.0), 1.0: dict(val=-0.9, grad=-1.0)})
    with pytest.raises(ZeroDivisionError):
        WolfeSearch._interpolate(0, 1.0, {0: dict(val=0.0, grad=0.0), 1.0: dict(val=0.0, grad=0.0)})


# ------------------------------------------------------------------------------------------------------- the float32 restatement --
def test_wolfe_ref_reproduces_the_recorded_steps_of_the_reference():
    """Direction, momentum and trial points bit for bit; phi' within the reduction bound of the reference's own float32 sum (torch sums a tensor
    in chunks of its own choosing: <= n roundings per term is the loosest order there is, and the bound used)."""
    data = np.load(os.path.join(HERE, "golden", "wolfe_optimizer.npz"))
    form, lr, alphas = str(data["trial_form"]), float(data["lr"][0]), [float(a) for a in data["alphas"]]
    assert form == "fma"                     # what csrc/wolfe.hip does (fb_mt_wolfe_trial); the other form would need the kernel changed
    n_tensors = len([k for k in data.files if k.startswith("c0/theta0/")])
    assert n_tensors == 4
    compared = 0
    for c, (mu, damp, nesterov, wd) in enumerate(data["configs"]):
        theta = [data[f"c{c}/theta0/{i}"] for i in range(n_tensors)]
        mom = [None] * n_tensors
        t = 1
        while f"c{c}/g{t}/0" in data.files:
            dphi, mag, p_all = 0.0, 0.0, []
            for i in range(n_tensors):
                g = data[f"c{c}/g{t}/{i}"]
                buf, p, d = wolfe_ref.direction_f32(theta[i], g, mom[i], wd, mu, damp, bool(nesterov), mom[i] is None)
                assert p.dtype == np.float32 and np.array_equal(p.view(np.int32), data[f"c{c}/p{t}/{i}"].view(np.int32)), (c, t, i, "p")
                if mu != 0:
                    assert np.array_equal(buf.view(np.int32), data[f"c{c}/mom{t}/{i}"].view(np.int32)), (c, t, i, "mom")
                    mom[i] = buf
                dphi += float((d.astype(np.float64) * p).sum())
                mag += float(np.abs(d.astype(np.float64) * p).sum())
                p_all.append(p)
                compared += p.size
            n = sum(p.size for p in p_all)
            assert abs(dphi - float(data[f"c{c}/dphi0_{t}"][0])) <= n * wolfe_ref.U32 * mag, (c, t)
            for a, alpha in enumerate(alphas):
                dphi, mag, new = 0.0, 0.0, []
                for i in range(n_tensors):
                    th = wolfe_ref.trial_f32(theta[i], p_all[i], lr, alpha, form)
                    assert np.array_equal(th.view(np.int32), data[f"c{c}/theta{t}_{a}/{i}"].view(np.int32)), (c, t, a, i, "theta")
                    d, p = wolfe_ref.phi_grad_terms_f32(th, data[f"c{c}/ga{t}_{a}/{i}"], p_all[i], wd)
                    dphi += float((d.astype(np.float64) * p).sum())
                    mag += float(np.abs(d.astype(np.float64) * p).sum())
                    new.append(th)
                assert abs(dphi - float(data[f"c{c}/dphi{t}_{a}"][0])) <= n * wolfe_ref.U32 * mag, (c, t, a)
            theta = new                       # no final step: the parameters stay at the last trial point
            t += 1
        assert t == 4
    assert compared == 5 * 3 * (5 + 12 + 54 + 259)


def test_the_two_restatements_agree_within_their_bounds():
    rng = np.random.default_rng(3)
    n = 1000
    theta, g, mom = (rng.standard_normal(n).astype(np.float32) * s for s in (0.1, 1.0, 0.5))
    g *= (10.0 ** (rng.random(n) * 8 - 6)).astype(np.float32)
    for mu, damp, nesterov, wd, first in ((0.9, 0.0, True, 5e-4, False), (0.9, 0.25, False, 5e-4, False), (0.9, 0.0, True, 5e-4, True),
                                          (0.0, 0.0, False, 1e-2, False)):
        buf, p, d = wolfe_ref.direction_f32(theta, g, mom, wd, mu, damp, nesterov, first)
        ref = wolfe_ref.direction_f64(*(torch.from_numpy(x) for x in (theta, g, mom)), wd, mu, damp, nesterov, first)
        assert bool(((torch.from_numpy(p).double() - ref["p"][0]).abs() <= ref["p"][1]).all())
        if mu != 0:
            assert bool(((torch.from_numpy(buf).double() - ref["mom"][0]).abs() <= ref["mom"][1]).all())
        th = wolfe_ref.trial_f32(theta, p, 0.07, 2.5)
        t64, bound = wolfe_ref.trial_f64(torch.from_numpy(theta), torch.from_numpy(p), 0.07, 2.5)
        assert bool(((torch.from_numpy(th).double() - t64).abs() <= bound).all())
    assert wolfe_ref.chain_length(1, 4, 256, 1024) == 1 and wolfe_ref.chain_length(4, 4, 256, 1024) == 4
    assert wolfe_ref.chain_length(1024 * 1024 + 5, 4, 256, 1024) == 9 and wolfe_ref.phi_c(1024, False) == 4 + 11
    assert wolfe_ref.phi_c(1024, True, "nesterov") == 4 + 11 + 6


# ------------------------------------------------------------------------------------------------------------------ scope, wiring --
def test_line_search_wolfe_composes_with_and_without_the_four_keys():
    from fullbatchtraining_amd.training import GradualWarmupScheduler, WolfeGradientDescent, _check_scope, optim_interface, wolfe_constants
    cfg = compose(WOLFE + ["hyp.warmup=2", "hyp.steps=6"])
    assert not any(k in cfg.hyp.optim for k in ("c1", "c2", "alpha_max", "max_iter"))
    assert wolfe_constants(cfg.hyp.optim) == (1e-4, 0.9, 10.0, 10)
    _check_scope(cfg)
    optimizer, scheduler = optim_interface(torch.nn.Linear(3, 2), cfg.hyp)
    assert type(optimizer) is WolfeGradientDescent and isinstance(scheduler, GradualWarmupScheduler) and optimizer._opt_called is True
    group = optimizer.param_groups[0]
    assert {k: group[k] for k in ("c1", "c2", "alpha_max", "max_iter")} == dict(c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10)
    assert (group["momentum"], group["weight_decay"], group["nesterov"], group["dampening"], group["initial_lr"]) == (0.9, 5e-4, True, 0.0, 0.1)
    cfg = compose(WOLFE + ["+hyp.optim.c1=0.001", "+hyp.optim.c2=0.5", "+hyp.optim.alpha_max=4.0", "+hyp.optim.max_iter=3"])
    assert wolfe_constants(cfg.hyp.optim) == (0.001, 0.5, 4.0, 3)
    _check_scope(cfg)
    group = optim_interface(torch.nn.Linear(3, 2), cfg.hyp)[0].param_groups[0]
    assert {k: group[k] for k in ("c1", "c2", "alpha_max", "max_iter")} == dict(c1=0.001, c2=0.5, alpha_max=4.0, max_iter=3)
    with pytest.raises(RuntimeError, match="state container"):
        optimizer.step(lambda: None)
    with pytest.raises(ValueError, match="Nesterov momentum requires"):
        WolfeGradientDescent(torch.nn.Linear(2, 2).parameters(), nesterov=True, momentum=0.0)
    _check_scope(compose(WOLFE + ["hyp.grad_clip=0.5", "hyp.grad_noise.additive=0.1", "hyp.norm_bias.strength=0.1"]))
    _check_scope(compose(["hyp=gradreg", "hyp.optim.line_search=wolfe"]))


@pytest.mark.parametrize("over,needle", [
    (["hyp/optim_modification=SAM"], "line_search=wolfe with optim_modification 'SAM'"),
    (["hyp/optim_modification=LARC"], "line_search=wolfe with optim_modification 'LARC'"),
    (["hyp.only_linear_layers_weight_decay=True"], "line_search=wolfe with only_linear_layers_weight_decay"),
    (["hyp.train_stochastic=True"], "line_search=wolfe with hyp.train_stochastic"),
])
def test_scope_checks_name_what_the_wolfe_search_does_not_cover(over, needle):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    cfg = compose(WOLFE + over)
    with pytest.raises(NotImplementedError, match=re.escape(needle)):
        _check_scope(cfg, branch="stochastic" if "hyp.train_stochastic=True" in over else "full-batch")
    with pytest.raises(NotImplementedError, match=re.escape(needle)):
        optim_interface(torch.nn.Linear(2, 2), cfg.hyp)
    _check_scope(compose(["hyp=fb1"] + [o for o in over if "stochastic" not in o]))        # (line_search none keeps its scope)


@pytest.mark.parametrize("search", ["non-monotone", "restarting"])
def test_the_other_two_line_searches_stay_refused_and_are_named_as_follow_ups(search):
    from fullbatchtraining_amd.training import optim_interface
    cfg = compose(["hyp=fb1", f"hyp.optim.line_search={search}"])
    with pytest.raises(NotImplementedError, match=f"line_search '{search}'.*follow-ups"):
        optim_interface(torch.nn.Linear(2, 2), cfg.hyp)


def test_wolfe_is_refused_on_more_than_one_rank(monkeypatch):
    from fullbatchtraining_amd.training import _check_scope, optim_interface
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    cfg = compose(WOLFE)
    with pytest.raises(NotImplementedError, match="line_search=wolfe on more than one rank"):
        _check_scope(cfg)
    with pytest.raises(NotImplementedError, match="line_search=wolfe on more than one rank"):
        optim_interface(torch.nn.Linear(2, 2), cfg.hyp)
    _check_scope(compose(["hyp=fb1"]))


def test_the_multi_process_code_path_refuses_wolfe(monkeypatch):
    """FB_FORCE_DIST=1 with an initialised process group of ONE rank takes the multi-process code path: the trainer's constructor refuses there,
    before it touches the loaders or a device.  Without the switch the same group of one is the 1-process path and gets past that point."""
    from fullbatchtraining_amd.training import FullBatchTrainer
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 1)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda *a, **k: 0)
    setup = dict(device=torch.device("cpu"), dtype=torch.float, memory_format=torch.contiguous_format)
    monkeypatch.setenv("FB_FORCE_DIST", "1")
    with pytest.raises(NotImplementedError, match="line_search=wolfe on the multi-process code path"):
        FullBatchTrainer(torch.nn.Linear(3, 2), None, None, setup, compose(WOLFE))
    monkeypatch.delenv("FB_FORCE_DIST")
    with pytest.raises(Exception) as info:          # (no loader: the constructor fails later, not with the refusal)
        FullBatchTrainer(torch.nn.Linear(3, 2), None, None, setup, compose(WOLFE))
    assert "multi-process code path" not in str(info.value)


# --------------------------------------------------------------------------------------------------------------------- checkpoints --
class _StubEngine:
    """The engine's momentum surface with a state of its own making: momentum = 0.5 * parameter + 0.25."""

    def __init__(self, model, stepped=True):
        self.model, self.loaded, self.first_step = model, None, not stepped

    def store_to_model(self, model):
        pass

    def load_from_model(self, model):
        pass

    def momentum_state(self):
        return [p.detach() * 0.5 + 0.25 for p in self.model.parameters()]

    def load_momentum(self, bufs):
        self.loaded = [b.clone() for b in bufs]


def test_checkpoint_has_the_reference_layout_and_round_trips(tmp_path):
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import _load_from_checkpoint, _save_to_checkpoint, optim_interface
    want = _meta()["checkpoint"]
    cfg = compose(["hyp=fb1", "model=resnet20", "hyp.optim.line_search=wolfe", "hyp.warmup=2"])
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, 10)
    optimizer, scheduler = optim_interface(model, cfg.hyp)
    scheduler.step()
    optimizer.state["alpha"] = want["alpha"]  # what FullBatchTrainer._wolfe_step stores after a search (here: what the reference's search returned)

    class Counter:
        step = 1

    path = str(tmp_path / "ck.pth")
    _save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=path, engine=_StubEngine(model))
    optim_state, _, sched_state, scaler_state, step = torch.load(path, weights_only=False)
    tensors = [k for k in optim_state["state"] if k != "alpha"]
    got = dict(optimizer=type(optimizer).__name__, param_groups=describe(optim_state["param_groups"]), state0=describe(optim_state["state"][0]),
               state_last=describe(optim_state["state"][tensors[-1]]), n_state=len(optim_state["state"]), alpha=optim_state["state"]["alpha"],
               bare_keys=sorted(k for k in optim_state["state"] if isinstance(k, str)), scheduler_keys=sorted(sched_state),
               scaler_state=scaler_state, step=step)
    assert got == want and want["bare_keys"] == ["alpha"] and want["n_state"] == 66 and list(optim_state["state"][0]) == ["momentum_buffer"]
    # load: a fresh container and engine take the momentum and alpha
    torch.manual_seed(1)
    model2 = construct_model(cfg.model, 3, 10)
    optimizer2, scheduler2 = optim_interface(model2, cfg.hyp)
    engine2 = _StubEngine(model2, stepped=False)
    counter2 = type("Counter", (), {"step": 0})
    optimizer.state["alpha"] = 0.4375
    _save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=path, engine=_StubEngine(model))
    _load_from_checkpoint(model2, optimizer2, scheduler2, None, counter2, 10, file=path, engine=engine2)
    assert counter2.step == 1 and optimizer2.param_groups[0]["lr"] == 0.05 and optimizer2.state["alpha"] == 0.4375
    assert len(engine2.loaded) == 65
    for b, p in zip(engine2.loaded, model.parameters()):
        assert torch.equal(b, p.detach() * 0.5 + 0.25)


# ------------------------------------------------------------------------------------------------------------------- entry table --
PROTOS = {"fb_mt_wolfe_direction": "i:ppppplfffiippp", "fb_mt_wolfe_trial": "i:ppplfp", "fb_mt_wolfe_phi_grad": "i:ppplfppp"}


def test_entry_table_and_header_list_the_three_entry_points():
    from fullbatchtraining_amd import lib
    h = lib.load()
    assert lib.EXPECTED_ABI == 17 == h.fb_abi_version()
    table = {h.fb_entry_name(i).decode(): (h.fb_entry_sig(i).decode(), h.fb_entry_kind(i)) for i in range(h.fb_entry_count())}
    header = open(os.path.join(os.path.dirname(HERE), "include", "fb_engine.h")).read()
    code = {"float*": "p", "const float*": "p", "void*": "p", "int64_t": "l", "int32_t": "i", "float": "f"}
    for name, sig in PROTOS.items():
        proto = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        args = [" ".join(a.split()[:-1]) for a in proto.replace("\n", " ").split(",")]
        assert args[-1] == "void*"
        assert table[name] == ("i:" + "".join(code[a] for a in args), 2) and table[name][0] == sig, (name, table[name])
        fn = h.fb_cmd_fn_id(name.encode())
        assert fn >= 0 and h.fb_cmd_fn_nargs(fn) == len(args) == len(lib._SIGS[name])
        assert name in lib.EXPORTS
    assert (h.fb_abi_constant(b"FB_WOLFE_VEC"), h.fb_abi_constant(b"FB_WOLFE_BLOCK")) == (4, 256)
    assert "#define FB_WOLFE_VEC 4" in header and "#define FB_WOLFE_BLOCK 256" in header


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    from fullbatchtraining_amd import lib
    h = lib.load()
    nan = float("nan")
    assert h.fb_mt_wolfe_direction(16, 16, 16, 16, None, 64, 0.0, 0.9, 0.0, 1, 0, 16, 16, None) == FB_ERR_ARG
    assert b"fb_mt_wolfe_direction" in h.fb_last_error_string()
    assert h.fb_mt_wolfe_direction(16, 16, None, 16, 16, 64, 0.0, 0.9, 0.0, 1, 0, 16, 16, None) == FB_ERR_ARG       # momentum without a buffer
    assert h.fb_mt_wolfe_direction(16, 16, 16, 20, 16, 64, 0.0, 0.9, 0.0, 1, 0, 16, 16, None) == FB_ERR_ARG         # p not 16-byte aligned
    assert h.fb_mt_wolfe_direction(16, 16, 16, 16, 16, 64, nan, 0.9, 0.0, 1, 0, 16, 16, None) == FB_ERR_ARG
    assert h.fb_mt_wolfe_direction(16, 16, 16, 16, 16, -1, 0.0, 0.9, 0.0, 1, 0, 16, 16, None) == FB_ERR_ARG
    assert h.fb_mt_wolfe_trial(16, 16, None, 64, 0.1, None) == FB_ERR_ARG and b"fb_mt_wolfe_trial" in h.fb_last_error_string()
    assert h.fb_mt_wolfe_trial(16, 16, 16, 64, float("inf"), None) == FB_ERR_ARG
    assert h.fb_mt_wolfe_trial(16, 24, 16, 64, 0.1, None) == FB_ERR_ARG
    assert h.fb_mt_wolfe_trial(16, 16, 16, 0, 0.1, None) == 0                                                     # n = 0: FB_OK without a launch
    assert h.fb_mt_wolfe_phi_grad(16, 16, 16, 64, 0.0, None, 16, None) == FB_ERR_ARG and b"fb_mt_wolfe_phi_grad" in h.fb_last_error_string()
    assert h.fb_mt_wolfe_phi_grad(16, 16, 16, 64, nan, 16, 16, None) == FB_ERR_ARG
    assert h.fb_mt_wolfe_phi_grad(16, 16, 28, 64, 0.0, 16, 16, None) == FB_ERR_ARG


# ------------------------------------------------------------------------------------------------------------ golden admissibility --
def test_golden_scenarios_are_admissible():
    """Recomputed from the arrays: the reference's fp32 and float64 runs take the identical alpha sequence; the controller replays every step of
    both; every inequality it decided has at least 4 tolerances of margin; the scenarios contain an accepted alpha = 1 and a growth step; one
    statistics record per closure evaluation; the rung used is the first of the ladder that was not refused."""
    from fullbatchtraining_amd.training import WolfeSearch
    meta = _meta()
    data = np.load(os.path.join(HERE, "golden", "scenarios_wolfe.npz"))
    assert set(meta["scenarios"]) == {"wolfe_plain", "wolfe_clip", "wolfe_reg"} and meta["margin"] == 4.0 and meta["spread_limit"] == 1e-3
    seen = set()
    for name, sc in meta["scenarios"].items():
        assert "hyp.optim.line_search=wolfe" in sc["overrides"] and "model=resnet20" in sc["overrides"] and sc["pixels"] == 16
        assert sc["n"] == (64 if name == "wolfe_reg" else 128) and sc["steps"] in (2, 3)
        assert [sc["lr"], sc["model_seed"]] in meta["ladder"][name] and sc["tried"][-1]["refused"] == [] and sc["worst_margin"] >= 1.0
        assert all(t["refused"] for t in sc["tried"][:-1]) and [[t["lr"], t["seed"]] for t in sc["tried"]] == meta["ladder"][name][:len(sc["tried"])]
        assert sc["judged_at"] == {"wolfe_plain": 2e-4, "wolfe_clip": 2e-4, "wolfe_reg": 3e-3}[name]
        records = 0
        for tag in ("", "@f64"):
            evals, phi0 = data[f"{name}{tag}/evals"], data[f"{name}{tag}/phi0"]
            assert len(phi0) == sc["steps"]
            for s in range(sc["steps"]):
                rows = [tuple(float(v) for v in r[1:4]) for r in evals[evals[:, 0] == s]]
                todo = list(rows)

                def evaluate(alpha):
                    want = todo.pop(0)
                    assert alpha == want[0]
                    return want[1], want[2]

                ctl = WolfeSearch(**sc["constants"])
                got = ctl.search(float(phi0[s, 0]), float(phi0[s, 1]), evaluate)
                assert not todo and got == float(phi0[s, 3]) and ctl.evaluated == [r[0] for r in rows], (name, tag, s)
                if tag == "":
                    records += 1 + len(rows)
                    seen |= ({"accepted at alpha = 1"} if ctl.exit == "accepted" and got == 1.0 else set()) | ({"growth step"} if 2.5 in ctl.evaluated else set())
                    assert ctl.zoom_exit is None
        assert np.array_equal(data[f"{name}/evals"][:, :2], data[f"{name}@f64/evals"][:, :2]), name       # rule 1: the identical alpha sequence
        assert np.array_equal(data[f"{name}/phi0"][:, 3], data[f"{name}@f64/phi0"][:, 3]), name
        ineq = data[f"{name}/inequalities"]                         # rule 2: [step, kind, alpha, left, right, tolerance]
        assert len(ineq) > 0 and np.all(np.abs(ineq[:, 3] - ineq[:, 4]) >= 4.0 * ineq[:, 5])
        assert len(data[f"{name}/stat/train_loss"]) == len(data[f"{name}@f64/stat/train_loss"]) == records
        for key in ("train_loss", "full_loss", "param_norm"):
            r32, r64 = data[f"{name}/stat/{key}"], data[f"{name}@f64/stat/{key}"]
            spread = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
            assert spread < min(sc["judged_at"] / 2, 1e-3) and abs(spread - sc["spread"][key]) <= 1e-12, (name, key, spread)
        assert sc["final_rel_l2_bound"] == 5 * max(sc["final_rel_l2_fp32_runs"].values()) < 5e-3
    assert seen == set(meta["required"]) == {"accepted at alpha = 1", "growth step"}
