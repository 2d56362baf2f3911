"""``hyp/optim=fista`` end to end on the GPU: ``train()`` against runs of the REAL reference with its FISTA optimizer
(tests/golden/scenarios_fista.npz, written by tests/golden/make_golden_fista.py) in both branches; the wiring of the update -- arguments, state,
the modifiers in front of it -- against ``tests/fista_ref.fista_ref`` on snapshots, bit for bit; checkpoints; bf16, EMA; and that
gradient-descent runs allocate nothing for FISTA."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import fista_ref
from tests.adam_ref import describe
from tests.helpers import make_data, rel_err, shuffling_loaders, summarise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STAT_KEYS = ("train_loss", "train_acc", "param_norm", "full_loss", "clipped_step")
NORM_KEYS = ("grad_norm", "preclip_gradnorm")
SETUP = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)


@pytest.fixture(scope="module")
def golden_fista():
    with open(os.path.join(HERE, "golden", "meta_fista.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "golden", "scenarios_fista.npz"))), meta


def _run(meta, name, extra=(), tmp_path=None):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import train

    sc = meta["scenarios"][name]
    cfg = compose(sc["overrides"] + [f"data.pixels={sc['pixels']}", "impl.validate_every_nth_step=1000"] + list(extra),
                  original_cwd=str(tmp_path) if tmp_path else os.getcwd(), name=name)
    torch.manual_seed(sc["model_seed"])
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(sc["n"], sc["pixels"])
    if sc["shuffling_loader"]:                 # the loaders the reference run was given (RandomSampler, shared generator): its sample order
        tl, vl = shuffling_loaders(x, y, cfg.data.batch_size)
        return cfg, model, train(model, tl, vl, SETUP, cfg)
    return cfg, model, train(model, (x, y), (x[:64], y[:64]), SETUP, cfg)


@pytest.mark.parametrize("name", ["fista_plain", "fista_clip_warm", "fista_reg_r18", "fista_sgd_mode"])
def test_fista_train_matches_reference_run_f32(golden_fista, name, tmp_path):
    """Every statistic of every step within ``max(tol |r64|, 5 |r32 - r64|)`` of the reference's float64 run, tol = the scenario's ``judged_at``
    (``max(tol, 1e-3)`` for gradient norms), admissible because the reference's own fp32 run is within half of it (tests/test_cpu_fista.py); the
    final state in relative l2 against the float64 run, within ``max(5 x noise, meta bound)``."""
    data, meta = golden_fista
    tol = meta["judged_at"][name]
    cfg, model, stats = _run(meta, name, (), tmp_path)
    assert cfg.hyp.optim.name == "FISTA" and bool(cfg.hyp.train_stochastic) == (name == "fista_sgd_mode")
    for key in STAT_KEYS + NORM_KEYS:
        if f"{name}@f64/stat/{key}" not in data:
            assert key not in stats
            continue
        r64, r32 = data[f"{name}@f64/stat/{key}"], data[f"{name}/stat/{key}"]
        print(f"{name} {key}: engine {np.array(stats[key])} ref32 {r32} ref64 {r64}")
        t = max(tol, 1e-3) if key in NORM_KEYS else tol
        bound = np.maximum(t * np.abs(r64) + 1e-6, 5 * np.abs(r32 - r64))
        if key == "train_acc":       # one prediction may flip on the fp32 noise floor
            bound = np.maximum(bound, 1.0 / meta["scenarios"][name]["n"] + 1e-9)
        assert len(stats[key]) == len(r64) and np.all(np.abs(np.array(stats[key]) - r64) <= bound), (key, stats[key], r32, r64)
    n_chunks = len([k for k in stats if k.startswith("grad_norm_train_")])
    assert n_chunks == meta["scenarios"][name]["n"] // (cfg.data.batch_size if cfg.hyp.train_stochastic else min(cfg.data.batch_size, cfg.hyp.sub_batch))
    for k in range(n_chunks):
        r64, r32 = data[f"{name}@f64/stat/grad_norm_train_{k}"], data[f"{name}/stat/grad_norm_train_{k}"]
        bound = np.maximum(max(tol, 1e-3) * np.abs(r64), 5 * np.abs(r32 - r64))
        print(f"{name} grad_norm_train_{k}: engine {np.array(stats[f'grad_norm_train_{k}'])} ref32 {r32} ref64 {r64}")
        assert np.all(np.abs(np.array(stats[f"grad_norm_train_{k}"]) - r64) <= bound), (k, stats[f"grad_norm_train_{k}"], r32, r64)
    err = rel_err(summarise([v.double() for v in model.state_dict().values()])[1], data[f"{name}@f64/final_sample"])
    noise = rel_err(data[f"{name}/final_sample"], data[f"{name}@f64/final_sample"])
    print(f"{name}: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e}, bound {meta['final_rel_l2_bound'][name]:.2e})")
    # (the value in meta: 5x the LARGEST distance among the reference's fp32 runs at 8, 2 and 1 threads -- one run is one sample of its own noise)
    assert abs(noise - meta["spread"][name]["final_rel_l2"]) <= 1e-12
    assert err < max(5 * noise, meta["final_rel_l2_bound"][name])
    assert int(model.state_dict()["stem.1.num_batches_tracked"]) == int(data[f"{name}@f64/final_num_batches_tracked"][0])
    assert len(stats["valid_loss"]) >= 1 and np.isfinite(stats["valid_loss"][-1])
    if name == "fista_clip_warm":    # warm-up from lr 0 with ak = 0: the first update moves nothing -- equal records here iff equal in the reference's
        for key in ("train_loss", "param_norm"):
            ref_equal = bool(data[f"{name}/stat/{key}"][0] == data[f"{name}/stat/{key}"][1])
            assert (stats[key][0] == stats[key][1]) == ref_equal, (key, stats[key][:2], data[f"{name}/stat/{key}"][:2])
        assert data[f"{name}/stat/train_loss"][0] == data[f"{name}/stat/train_loss"][1]


# ------------------------------------------------------------------------------------------------------------------- wiring --
def _trainer(over, n, seed=5):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    cfg = compose(list(over) + ["data.pixels=16", "impl.validate_every_nth_step=1000"])
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(n, 16)
    return cfg, model, FullBatchTrainer(model, (x, y), (x[:32], y[:32]), SETUP, cfg)


def _padding_mask(eng):
    mask = torch.ones(eng.plan.P, dtype=torch.bool, device=eng.theta.device)
    for name in eng.plan.param_names:
        mask[eng.plan.offsets[name]:eng.plan.offsets[name] + math.prod(eng.plan.param_shapes[name])] = False
    return mask


def _same_bits(got, want):
    return int(np.count_nonzero(got.cpu().numpy().view(np.int32) != np.asarray(want, dtype=np.float32).view(np.int32)))


@pytest.mark.parametrize("modifiers", [False, True], ids=["clip", "clip-noise-norm-bias"])
def test_update_wiring_on_snapshots(modifiers):
    """Three full-batch steps (warm-up 1, clip 0.25 hit) with ``Engine.fista_step`` wrapped: at every call the arguments are the scheduler's lr
    and the configured ``fista_mod``, ``fista_tk`` advances through the host's sequence for steps 1-3, and the arenas after the call are
    ``fista_ref`` of the arenas before it with that step's (ak, 1 + ak), BIT FOR BIT.  With gradient noise and the norm bias on, the clip is
    applied in place in front of the noise (no clip argument) and the gradient the update consumed is not the closure's: the modifiers reach
    FISTA."""
    from fullbatchtraining_amd.engine import fista_coefficients
    from fullbatchtraining_amd.training import optim_interface
    mod = [0.02, 0.1, 4.0]
    over = ["hyp=fbclip", "model=resnet20", "hyp/optim=fista", "hyp.optim.lr=0.01", "hyp.optim.fista_mod=[0.02,0.1,4.0]", "hyp.steps=3",
            "hyp.warmup=1", "hyp.scheduler=cosine-decay", "data.batch_size=32", "hyp.sub_batch=32"]
    if modifiers:
        over += ["hyp.grad_noise.additive=0.01", "hyp.norm_bias.strength=0.1"]
    cfg, model, trainer = _trainer(over, 64)
    eng = trainer.engine
    assert getattr(eng, "x_minus", None) is None                                   # allocated on first use
    pad = _padding_mask(eng)
    assert int(pad.sum()) > 0
    snaps, orig = [], eng.fista_step

    def wrapped(lr, fista_mod, grad_clip=None, torch_clip=False):
        eng._fista_arena()
        before = dict(theta=eng.theta.clone(), avg=eng.avg.clone(), xm=eng.x_minus.clone(), norms2=eng.norms2.clone(), tk=eng.fista_tk)
        orig(lr, fista_mod, grad_clip, torch_clip)
        torch.cuda.synchronize()
        snaps.append(dict(before=before, args=(lr, list(fista_mod), grad_clip, torch_clip), tk=eng.fista_tk,
                          after=dict(theta=eng.theta.clone(), avg=eng.avg.clone(), xm=eng.x_minus.clone())))

    eng.fista_step = wrapped
    raw = []
    for _ in range(3):
        trainer.step()
        raw.append(float(trainer.stats["grad_norm"][-1]))
    ref_opt, ref_sched = optim_interface(torch.nn.Linear(2, 2), cfg.hyp)
    assert len(snaps) == 3
    tk = np.float32(1)
    for i, s in enumerate(snaps):
        lr, fista_mod, clip, torch_clip = s["args"]
        assert lr == ref_opt.param_groups[0]["lr"] and (i > 0 or lr == 0.0) and (i == 0 or lr > 0)
        ref_sched.step()
        assert fista_mod == mod and torch_clip is False and clip == (None if modifiers else 0.25)
        b, a = s["before"], s["after"]
        assert type(s["tk"]) is np.float32 and b["tk"].tobytes() == tk.tobytes()
        ieee = fista_ref.coefficients_ref(tk, mod)
        tk, ak, opak = fista_coefficients(tk, mod)                  # the host's coefficients: the reference's expression on this host's torch,
        for got, want, ulps in zip((tk, ak, opak), ieee, (1, 2, 2)):    # within a faithfully rounded sqrt of the IEEE ones (tests/test_cpu_fista.py)
            assert abs(np.float64(got) - np.float64(want)) <= ulps * np.float64(np.spacing(want)), (i, got, want)
        assert s["tk"].tobytes() == tk.tobytes() and (ak == 0) == (i == 0)
        norm2 = float(b["norms2"][0])
        coef, hit = fista_ref.clip_coef_f32(norm2, clip, False)
        assert hit == (not modifiers) and (modifiers or norm2 ** 0.5 > 1.0)
        theta, g, xm = fista_ref.fista_ref(b["theta"].cpu().numpy(), b["avg"].cpu().numpy(), b["xm"].cpu().numpy(), coef, lr, ak, opak)
        for key, got, want in (("theta", a["theta"], theta), ("grad", a["avg"], g), ("x_minus", a["xm"], xm)):
            diff = _same_bits(got, want)
            print(f"[wiring modifiers={modifiers} step {i + 1}] {key}: {diff} of {got.numel()} elements differ in their bits")
            assert diff == 0, (i, key, diff)
        if i == 0:                       # x- starts as a clone of the parameters; lr 0 and ak 0: the parameters keep their values
            assert torch.equal(b["xm"], b["theta"]) and torch.equal(a["theta"], b["theta"]) and torch.equal(a["xm"], b["theta"])
        else:
            assert torch.equal(b["xm"], snaps[i - 1]["after"]["xm"])
            assert not torch.equal(a["theta"], b["theta"]) and not torch.equal(a["theta"], a["xm"])
        for t in a.values():             # the arena's alignment padding stays exactly 0
            assert not bool(t[pad].any())
        if modifiers:
            # the norm bias (+0.1 on every element where |theta|^2 > 0) is in the norm the clip saw; what reached the update is that gradient clipped
            # to 0.25 plus N(0, 0.01^2) noise per element: |avg|^2 = 0.25^2 + 1e-4 n to a few per cent (the cross term is 2 * 0.25 * 0.01)
            n_real = int((~pad).sum())
            assert trainer.stats["preclip_gradnorm"][i] > 2 * raw[i] and abs(norm2 ** 0.5 - trainer.stats["preclip_gradnorm"][i]) < 1e-3 * norm2 ** 0.5
            assert abs(float(b["avg"].double().pow(2).sum()) / (0.25 ** 2 + 1e-4 * n_real) - 1) < 0.05
            assert torch.equal(a["avg"], b["avg"])
    assert trainer.stats["clipped_step"] == [1, 1, 1]


# --------------------------------------------------------------------------------------------------------------- checkpoints --
def test_fista_checkpoint_resumes_bit_for_bit_and_has_the_reference_layout(golden_fista, tmp_path):
    """2 steps, save, resume in a fresh trainer, 1 step = 3 uninterrupted steps: parameters, buffers, x+, x-, tk, bit for bit.  The saved optimizer
    state has the key structure of the reference's own checkpoint (meta_fista.json).  cosine-4000: the lr of a step does not depend on
    hyp.steps."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import fista_coefficients
    from fullbatchtraining_amd.models import construct_model
    data, meta = golden_fista
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    extra = ["hyp.scheduler=cosine-4000", "hyp.warmup=2", "hyp.optim.lr=0.01"]
    _run(meta, "fista_plain", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=2"], tmp_path)
    assert torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)[4] == 2
    _, _, stats_r = _run(meta, "fista_plain", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=3"], tmp_path)
    _, _, stats_s = _run(meta, "fista_plain", extra + ["impl.checkpoint.name=straight.pth", "hyp.steps=3"], tmp_path)
    assert len(stats_r["train_loss"]) == 1 and len(stats_s["train_loss"]) == 3 and stats_r["train_loss"][-1] == stats_s["train_loss"][-1]
    resumed = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    straight = torch.load(tmp_path / "checkpoints" / "straight.pth", weights_only=False)
    assert resumed[4] == straight[4] == 3 and resumed[3] is None
    for (k, a), b in zip(resumed[1].items(), straight[1].values()):
        assert torch.equal(a, b), k
    n_params = len(list(construct_model(compose(meta["scenarios"]["fista_plain"]["overrides"]).model, 3, 10).parameters()))
    assert len(resumed[0]["state"]) == len(straight[0]["state"]) == n_params
    tk3 = np.float32(1)
    for _ in range(3):
        tk3 = fista_coefficients(tk3, (1.0, 1.0, 4.0))[0]
    for i in range(n_params):
        a, b = resumed[0]["state"][i], straight[0]["state"][i]
        assert list(a) == ["x+", "x-", "tk"] and a["tk"].numpy().tobytes() == b["tk"].numpy().tobytes() == tk3.tobytes()
        assert torch.equal(a["x-"], b["x-"]) and torch.equal(a["x+"], b["x+"]) and torch.equal(a["x+"], a["x-"]), i
    first = list(resumed[1].values())[0]
    assert first.shape == resumed[0]["state"][0]["x-"].shape and not torch.equal(first, resumed[0]["state"][0]["x-"])    # ak != 0: the parameters are ahead of x-
    assert resumed[0]["param_groups"] == straight[0]["param_groups"]
    # the reference's own checkpoint (ResNet-20, one step): same keys, same shapes and dtypes
    want = meta["checkpoint"]
    assert want["optimizer"] == "FISTA" and want["n_state"] == n_params
    assert describe(resumed[0]["state"][0]) == want["state0"] and describe(resumed[0]["state"][n_params - 1]) == want["state_last"]
    mine = describe(resumed[0]["param_groups"])
    assert len(mine) == len(want["param_groups"]) == 1 and list(mine[0]) == list(want["param_groups"][0])
    assert mine[0]["params"] == want["param_groups"][0]["params"] and mine[0]["fista_mod"] == want["param_groups"][0]["fista_mod"]
    assert mine[0]["projection"] is None and sorted(resumed[2]) == want["scheduler_keys"]


# --------------------------------------------------------------------------------------------------------------- other paths --
def test_fista_bf16_runs_and_tracks_the_f32_engine_on_the_first_step(golden_fista, tmp_path):
    """impl.mixed_precision=True: three finite steps; the first record (taken at the initial parameters) within the looseness the project gives
    bf16 against fp32 -- 2e-2 on losses and the parameter norm, 0.1 on the gradient norm -- of the f32 ENGINE run."""
    data, meta = golden_fista
    _, _, f32 = _run(meta, "fista_plain", (), tmp_path)
    cfg, _, bf16 = _run(meta, "fista_plain", ["impl.mixed_precision=True"], tmp_path)
    assert cfg.impl.mixed_precision is True
    for key in ("train_loss", "full_loss", "param_norm", "grad_norm"):
        print(f"bf16 {key}: {np.array(bf16[key])} f32 engine {np.array(f32[key])}")
        assert len(bf16[key]) == 3 and np.all(np.isfinite(bf16[key]))
        assert abs(bf16[key][0] - f32[key][0]) <= (0.1 if key == "grad_norm" else 2e-2) * abs(f32[key][0]), key
    assert bf16["train_loss"][2] < bf16["train_loss"][0]


def test_fista_bf16_refreshes_the_compute_dtype_copies_after_the_update():
    """bf16 storage in the mini-batch branch, whose update section ends with the weight copies: after an epoch the compute-dtype copies are those
    of the updated parameters (regenerating them from ``theta`` changes nothing)."""
    over = ["hyp=base_sgd", "hyp.grad_clip=0.5", "model=resnet20", "hyp/optim=fista", "hyp.optim.lr=0.01", "hyp.steps=2", "hyp.warmup=0", "data.batch_size=32", "impl.mixed_precision=True"]
    cfg, model, trainer = _trainer(over, 64)
    eng = trainer.engine
    theta0 = eng.theta.clone()
    trainer.step()
    trainer.step()
    trainer.flush_stats()
    assert eng.w_fwd[0].dtype == torch.bfloat16 and not torch.equal(eng.theta, theta0) and bool(torch.isfinite(eng.theta).all())
    assert not torch.equal(eng.theta, eng.x_minus)                   # the second update has ak != 0
    fwd, dgrad = eng.w_fwd[0].clone(), eng.w_dgrad[0].clone()
    eng.w_fwd[0].zero_()
    eng.prep_weights(eng.theta, 1)
    torch.cuda.synchronize()
    assert torch.equal(eng.w_fwd[0].view(torch.int16), fwd.view(torch.int16)) and torch.equal(eng.w_dgrad[0].view(torch.int16), dgrad.view(torch.int16))
    assert bool(fwd.any()) and np.all(np.isfinite(trainer.stats["train_loss"]))


def test_fista_with_ema_and_test_time_flips_evaluates(golden_fista, tmp_path):
    data, meta = golden_fista
    _, model, stats = _run(meta, "fista_plain", ["hyp.evaluate_ema=True", "hyp.test_time_flips=True", "impl.validate_every_nth_step=1"], tmp_path)
    assert len(stats["valid_loss"]) == 3 and np.all(np.isfinite(stats["valid_loss"])) and all(0.0 <= a <= 1.0 for a in stats["valid_acc"])
    assert len(stats["train_loss"]) == 3 and np.all(np.isfinite(stats["train_loss"]))


def test_gradient_descent_runs_allocate_nothing_for_fista():
    for over, n in ((["hyp=fb1", "model=resnet20", "hyp.steps=2", "hyp.warmup=0", "data.batch_size=32", "hyp.sub_batch=32"], 64),
                    (["hyp=base_sgd", "model=resnet20", "hyp.steps=2", "hyp.warmup=0", "data.batch_size=32"], 64)):
        cfg, model, trainer = _trainer(over, n)
        assert type(trainer.optimizer) is torch.optim.SGD
        trainer.step()
        trainer.flush_stats()
        eng = trainer.engine
        assert getattr(eng, "x_minus", None) is None and not hasattr(eng, "fista_tk")
        assert not eng.first_step and bool(eng.mom.any())
