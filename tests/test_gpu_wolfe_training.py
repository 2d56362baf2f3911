"""``hyp.optim.line_search=wolfe`` end to end on the GPU: ``train()`` against runs of the REAL reference with its ``WolfeGradientDescent``
(tests/golden/scenarios_wolfe.npz, written by tests/golden/make_golden_wolfe.py): the alpha sequence of every search EXACTLY, the statistics of
every closure evaluation (not only of every step), the final state, one statistics record per closure evaluation; the wiring of the three
kernels against tests/wolfe_ref.py on snapshots; a checkpoint taken after step 1 and resumed equals the uninterrupted run bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from tests import wolfe_ref
from tests.adam_ref import describe
from tests.helpers import make_data, rel_err, summarise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETUP = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
STAT_KEYS = ("train_loss", "train_acc", "param_norm", "full_loss", "clipped_step")
NORM_KEYS = ("grad_norm", "preclip_gradnorm")
SMALL = ["hyp=fbclip", "model=resnet20", "hyp.optim.line_search=wolfe", "hyp.optim.lr=0.05", "hyp.warmup=0", "hyp.scheduler=cosine-4000",
         "data.batch_size=32", "hyp.sub_batch=32"]


@pytest.fixture(scope="module")
def golden_wolfe():
    with open(os.path.join(HERE, "golden", "meta_wolfe.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "golden", "scenarios_wolfe.npz"))), meta


@pytest.fixture()
def searches(monkeypatch):
    """Every ``WolfeSearch.search`` of the test, as (alphas evaluated, alpha returned)."""
    from fullbatchtraining_amd import training
    log, inner = [], training.WolfeSearch.search

    def search(self, loss0, phi_grad0, evaluate):
        got = inner(self, loss0, phi_grad0, evaluate)
        log.append((list(self.evaluated), got, (loss0, phi_grad0)))
        return got

    monkeypatch.setattr(training.WolfeSearch, "search", search)
    return log


def _train(overrides, n, pixels, seed, name, extra=(), tmp_path=None):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import train

    cfg = compose(list(overrides) + [f"data.pixels={pixels}", "impl.validate_every_nth_step=1000"] + list(extra),
                  original_cwd=str(tmp_path) if tmp_path else os.getcwd(), name=name)
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(n, pixels)
    return cfg, model, train(model, (x, y), (x[:64], y[:64]), SETUP, cfg)


@pytest.mark.parametrize("name", ["wolfe_plain", "wolfe_clip", "wolfe_reg"])
def test_wolfe_train_matches_reference_run_f32(golden_wolfe, searches, name, tmp_path):
    """The alpha sequence of every step exactly (admissible: the reference's fp32 and float64 runs take it too, and every inequality behind it is
    decided by 4 tolerances: tests/golden/make_golden_wolfe.py).  Every statistic of every EVALUATION within ``max(tol |r64|, 5 |r32 - r64|)`` of the
    reference's float64 run, tol = the scenario's ``judged_at`` (``max(tol, 1e-3)`` for gradient norms); phi'(0) of every step likewise; the
    final state in relative l2 against the float64 run within ``max(5 x noise, meta bound)``; one record per closure evaluation."""
    data, meta = golden_wolfe
    sc = meta["scenarios"][name]
    tol = sc["judged_at"]
    cfg, model, stats = _train(sc["overrides"], sc["n"], sc["pixels"], sc["model_seed"], name, (), tmp_path)
    assert cfg.hyp.optim.line_search == "wolfe" and len(searches) == sc["steps"]
    evals, phi0, phi0_64 = data[f"{name}/evals"], data[f"{name}/phi0"], data[f"{name}@f64/phi0"]
    n_records = 0
    for s, (evaluated, returned, (loss0, dphi0)) in enumerate(searches):
        rows = evals[evals[:, 0] == s]
        print(f"{name} step {s}: engine alphas {evaluated} -> {returned!r}; reference {list(rows[:, 1])} -> {phi0[s, 3]!r}")
        assert evaluated == [float(a) for a in rows[:, 1]] and returned == float(phi0[s, 3]), (s, evaluated, returned)
        n_records += 1 + len(evaluated)
        b = max(tol * abs(phi0_64[s, 1]), 5 * abs(phi0[s, 1] - phi0_64[s, 1]))
        print(f"{name} step {s}: phi'(0) engine {dphi0!r} ref32 {phi0[s, 1]!r} ref64 {phi0_64[s, 1]!r} bound {b:.3e}")
        assert abs(dphi0 - phi0_64[s, 1]) <= b, ("phi'(0)", s, dphi0, phi0[s, 1], phi0_64[s, 1])
    for key in STAT_KEYS + NORM_KEYS:
        if f"{name}@f64/stat/{key}" not in data:
            assert key not in stats
            continue
        r64, r32 = data[f"{name}@f64/stat/{key}"], data[f"{name}/stat/{key}"]
        print(f"{name} {key}: engine {np.array(stats[key])} ref32 {r32} ref64 {r64}")
        t = max(tol, 1e-3) if key in NORM_KEYS else tol
        bound = np.maximum(t * np.abs(r64) + 1e-6, 5 * np.abs(r32 - r64))
        if key == "train_acc":       # one prediction may flip on the fp32 noise floor
            bound = np.maximum(bound, 1.0 / sc["n"] + 1e-9)
        assert len(stats[key]) == len(r64) == n_records, (key, len(stats[key]), len(r64), n_records)      # one record per closure evaluation
        assert np.all(np.abs(np.array(stats[key]) - r64) <= bound), (key, stats[key], r32, r64)
    n_chunks = len([k for k in stats if k.startswith("grad_norm_train_")])
    assert n_chunks == sc["n"] // min(cfg.data.batch_size, cfg.hyp.sub_batch)
    for k in range(n_chunks):
        r64, r32 = data[f"{name}@f64/stat/grad_norm_train_{k}"], data[f"{name}/stat/grad_norm_train_{k}"]
        bound = np.maximum(max(tol, 1e-3) * np.abs(r64), 5 * np.abs(r32 - r64))
        assert np.all(np.abs(np.array(stats[f"grad_norm_train_{k}"]) - r64) <= bound), (k, stats[f"grad_norm_train_{k}"], r32, r64)
    err = rel_err(summarise([v.double() for v in model.state_dict().values()])[1], data[f"{name}@f64/final_sample"])
    noise = rel_err(data[f"{name}/final_sample"], data[f"{name}@f64/final_sample"])
    print(f"{name}: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e}, bound {sc['final_rel_l2_bound']:.2e})")
    assert err < max(5 * noise, sc["final_rel_l2_bound"])
    # every closure evaluation advances the BatchNorm statistics once
    assert int(model.state_dict()["stem.1.num_batches_tracked"]) == int(data[f"{name}@f64/final_num_batches_tracked"][0])


def _trainer(over, n, seed=5):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    cfg = compose(list(over) + ["data.pixels=16", "impl.validate_every_nth_step=1000"])
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(n, 16)
    return cfg, model, FullBatchTrainer(model, (x, y), (x[:32], y[:32]), SETUP, cfg)


def test_wolfe_step_wiring_on_snapshots(searches):
    """Two steps with the three engine calls wrapped: one direction per step on the CLIPPED gradient (the clip is applied in place in front of
    it), one trial + one phi' per evaluation with step = lr alpha; the arenas after each call are within tests/wolfe_ref's bounds of the float64
    restatement of the arenas before it; the momentum has the bits ``fb_mt_clip_sgd`` writes; the p / theta0 arenas appear with the first step;
    the parameters end at the LAST EVALUATED trial point; the scalars the search saw are the ones in the device buffer; one statistics record
    per evaluation, whose train_loss is the loss the search compared."""
    cfg, model, trainer = _trainer(SMALL + ["hyp.steps=2", "hyp.grad_clip=0.25"], 64)
    eng, o = trainer.engine, cfg.hyp.optim
    assert getattr(eng, "wolfe_p", None) is None
    calls, orig = [], {k: getattr(eng, k) for k in ("wolfe_direction", "wolfe_trial", "wolfe_phi_grad")}

    def direction(wd, mu, damp, nesterov):
        before = dict(theta=eng.theta.clone(), avg=eng.avg.clone(), mom=eng.mom.clone(), first=eng.first_step, norm2=float(eng.norms2[0]))
        orig["wolfe_direction"](wd, mu, damp, nesterov)
        torch.cuda.synchronize()
        calls.append(("direction", (wd, mu, damp, nesterov), before, dict(mom=eng.mom.clone(), p=eng.wolfe_p.clone(), theta0=eng.wolfe_theta0.clone(),
                                                                         out=eng.wolfe_out.clone())))

    def trial(lr, alpha):
        orig["wolfe_trial"](lr, alpha)
        torch.cuda.synchronize()
        calls.append(("trial", (lr, alpha), None, dict(theta=eng.theta.clone())))

    def phi_grad(wd):
        orig["wolfe_phi_grad"](wd)
        torch.cuda.synchronize()
        calls.append(("phi_grad", (wd,), dict(theta=eng.theta.clone(), avg=eng.avg.clone()), dict(out=eng.wolfe_out.clone())))

    eng.wolfe_direction, eng.wolfe_trial, eng.wolfe_phi_grad = direction, trial, phi_grad
    lrs = []
    for _ in range(2):
        lrs.append(trainer.optimizer.param_groups[0]["lr"])
        trainer.step()
    stats = trainer.stats
    assert len(searches) == 2 and [c[0] for c in calls].count("direction") == 2
    n_evals = sum(len(s[0]) for s in searches)
    assert [c[0] for c in calls].count("trial") == [c[0] for c in calls].count("phi_grad") == n_evals >= 2
    assert len(stats["train_loss"]) == 2 + n_evals == len(stats["preclip_gradnorm"])
    P, it, rec = eng.plan.P, iter(calls), 0
    for s, (evaluated, returned, (loss0, dphi0)) in enumerate(searches):
        kind, args, b, a = next(it)
        assert kind == "direction" and args == (o.weight_decay, o.momentum, o.dampening, o.nesterov) and b["first"] == (s == 0)
        assert b["norm2"] ** 0.5 > 0.25 and abs(float(b["avg"].double().pow(2).sum()) ** 0.5 - 0.25) < 1e-4     # the clip was hit and applied in place
        ref = wolfe_ref.direction_f64(b["theta"], b["avg"], b["mom"], *args, b["first"])
        for key in ("mom", "p"):
            assert bool(((a[key].double() - ref[key][0]).abs() <= ref[key][1]).all()), (s, key)
        assert torch.equal(a["theta0"], b["theta"])
        sgd = {k: b[k].clone() for k in ("theta", "avg", "mom")}
        from fullbatchtraining_amd import lib
        lib.call("fb_mt_clip_sgd", sgd["theta"].data_ptr(), sgd["avg"].data_ptr(), sgd["mom"].data_ptr(), P, None, -1.0, 0.1, o.weight_decay, o.momentum,
                 o.dampening, 1 if o.nesterov else 0, 1 if b["first"] else 0)
        assert torch.equal(sgd["mom"].view(torch.int32), a["mom"].view(torch.int32)), "momentum bits differ from fb_mt_clip_sgd's"
        c = wolfe_ref.phi_c(P, True, ref["mode"])
        assert abs(float(a["out"][0]) - ref["dphi"][0]) <= c * wolfe_ref.U32 * wolfe_ref.SLACK * ref["dphi"][1]
        assert dphi0 == float(a["out"][0]) and loss0 == stats["train_loss"][rec] and dphi0 < 0
        rec += 1
        theta0, p = a["theta0"], a["p"]
        for alpha in evaluated:
            kind, args, _, at = next(it)
            assert kind == "trial" and args == (lrs[s], alpha)
            t64, bound = wolfe_ref.trial_f64(theta0, p, lrs[s], alpha)
            assert bool(((at["theta"].double() - t64).abs() <= bound).all()), (s, alpha)
            kind, args, bp, ap = next(it)
            assert kind == "phi_grad" and args == (o.weight_decay,) and torch.equal(bp["theta"], at["theta"])
            want, mag = wolfe_ref.phi_grad_f64(bp["theta"], bp["avg"], p, o.weight_decay)
            assert abs(float(ap["out"][1]) - want) <= wolfe_ref.phi_c(P, False) * wolfe_ref.U32 * wolfe_ref.SLACK * mag
            rec += 1
    assert trainer.optimizer.state["alpha"] == searches[-1][1]
    assert next(it, None) is None and rec == len(stats["train_loss"])
    assert torch.equal(eng.theta, [c for c in calls if c[0] == "trial"][-1][3]["theta"])          # no final step
    assert stats["clipped_step"][0] == 1 and len(stats["clipped_step"]) == rec


def test_gradient_descent_without_a_line_search_allocates_nothing_for_it():
    cfg, model, trainer = _trainer(["hyp=fbclip", "model=resnet20", "hyp.steps=1", "data.batch_size=32", "hyp.sub_batch=32"], 64)
    trainer.step()
    assert getattr(trainer.engine, "wolfe_p", None) is None and getattr(trainer.engine, "wolfe_theta0", None) is None
    assert len(trainer.stats["train_loss"]) == 1


def test_wolfe_checkpoint_resumes_bit_for_bit_and_has_the_reference_layout(searches, tmp_path):
    """1 step, save, resume in a fresh trainer, 1 step = 2 uninterrupted steps: parameters, buffers, momentum and alpha, bit for bit.  The saved
    optimizer state has the key structure of the reference's own checkpoint (meta_wolfe.json).  cosine-4000: the lr of a step does not depend on
    hyp.steps."""
    with open(os.path.join(HERE, "golden", "meta_wolfe.json")) as handle:
        want = json.load(handle)["checkpoint"]
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    run = lambda ck, steps: _train(SMALL, 64, 16, 7, "wolfe_ck", [f"impl.checkpoint.name={ck}", f"hyp.steps={steps}"], tmp_path)      # noqa: E731
    run("ck.pth", 1)
    first = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    assert first[4] == 1 and first[0]["state"]["alpha"] == searches[0][1]
    _, _, stats_r = run("ck.pth", 2)
    n_resumed = len(searches)
    _, _, stats_s = run("straight.pth", 2)
    assert n_resumed == 2 and len(searches) == 4 and searches[1][:2] == searches[3][:2] and searches[0][:2] == searches[2][:2]
    assert len(stats_r["train_loss"]) == 1 + len(searches[1][0]) and stats_r["train_loss"] == stats_s["train_loss"][-len(stats_r["train_loss"]):]
    resumed = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    straight = torch.load(tmp_path / "checkpoints" / "straight.pth", weights_only=False)
    assert resumed[4] == straight[4] == 2
    for (k, a), b in zip(resumed[1].items(), straight[1].values()):
        assert torch.equal(a, b), k
    n_params = want["n_state"] - 1
    assert len(resumed[0]["state"]) == len(straight[0]["state"]) == want["n_state"]
    assert resumed[0]["state"]["alpha"] == straight[0]["state"]["alpha"] == searches[3][1]
    for i in range(n_params):
        a, b = resumed[0]["state"][i], straight[0]["state"][i]
        assert list(a) == ["momentum_buffer"] and torch.equal(a["momentum_buffer"], b["momentum_buffer"]), i
    assert describe(resumed[0]["state"][0]) == want["state0"] and describe(resumed[0]["state"][n_params - 1]) == want["state_last"]
    mine = describe(resumed[0]["param_groups"])
    assert want["optimizer"] == "WolfeGradientDescent" and len(mine) == len(want["param_groups"]) == 1
    assert list(mine[0]) == list(want["param_groups"][0]) and mine[0]["params"] == want["param_groups"][0]["params"]
    assert resumed[0]["param_groups"] == straight[0]["param_groups"] and resumed[2] == straight[2]
