"""``hyp/optim=gd_agc`` end to end on the GPU: ``train()`` against runs of the REAL reference with its ``SGD_AGC`` (tests/golden/scenarios_agc.npz,
written by tests/golden/make_golden_agc.py) in both branches; the wiring of the update -- arguments, state, the unit table, the modifiers in
front of it -- against ``tests/agc_ref.agc_ref`` on snapshots (no trajectory); checkpoints; bf16; EMA; and that the averaged gradient keeps the
global clip only."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import adam_ref, agc_ref
from tests.helpers import clip_coef_ref, make_data, rel_err, shuffling_loaders, summarise, within_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STAT_KEYS = ("train_loss", "train_acc", "param_norm", "full_loss", "clipped_step")
NORM_KEYS = ("grad_norm", "preclip_gradnorm")
SETUP = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
PRESET = dict(weight_decay=2e-5, momentum=0.9, dampening=0.0, nesterov=True, clipping=0.01, eps=1e-3)


@pytest.fixture(scope="module")
def golden_agc():
    with open(os.path.join(HERE, "golden", "meta_agc.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "golden", "scenarios_agc.npz"))), meta


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


@pytest.mark.parametrize("name", ["agc_plain", "agc_clip_warm", "agc_reg_r18", "agc_sgd_mode"])
def test_gd_agc_train_matches_reference_run_f32(golden_agc, name, tmp_path):
    """Every statistic of every step within ``max(tol |r64|, 5 |r32 - r64|)`` of the reference's float64 run, tol = the scenario's ``judged_at``
    (``max(tol, 1e-3)`` for gradient norms), admissible because the reference's own fp32 run is within half of it (tests/test_cpu_agc.py); the
    final state in relative l2 against the float64 run, within 5x what the reference's own fp32 runs get.  On every trajectory some units' clip
    triggered and some did not (meta_agc.json: triggered_units)."""
    data, meta = golden_agc
    tol = meta["judged_at"][name]
    cfg, model, stats = _run(meta, name, (), tmp_path)
    assert cfg.hyp.optim.name == "GD-AGC" and bool(cfg.hyp.train_stochastic) == (name == "agc_sgd_mode")
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
    print(f"{name}: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e})")
    assert abs(noise - meta["spread"][name]["final_rel_l2"]) <= 1e-12
    assert err < max(5 * noise, meta["final_rel_l2_bound"][name])
    assert int(model.state_dict()["stem.1.num_batches_tracked"]) == int(data[f"{name}@f64/final_num_batches_tracked"][0])
    assert len(stats["valid_loss"]) >= 1 and np.isfinite(stats["valid_loss"][-1])
    if name == "agc_clip_warm":      # warm-up from lr 0: the first update leaves the parameters where they were, so records 1 and 2 are equal
        assert stats["train_loss"][0] == stats["train_loss"][1] and stats["param_norm"][0] == stats["param_norm"][1]


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


def _wrap(eng, snaps):
    orig = eng.agc_sgd_step

    def wrapped(lr, weight_decay, momentum, dampening, nesterov, clipping, eps, grad_clip=None, torch_clip=False):
        before = dict(theta=eng.theta.clone(), avg=eng.avg.clone(), mom=eng.mom.clone(), norms2=eng.norms2.clone(), first=eng.first_step)
        orig(lr, weight_decay, momentum, dampening, nesterov, clipping, eps, grad_clip, torch_clip)
        torch.cuda.synchronize()
        snaps.append(dict(before=before, args=(lr, grad_clip, torch_clip), hyp=dict(weight_decay=weight_decay, momentum=momentum, dampening=dampening,
                                                                                   nesterov=nesterov, clipping=clipping, eps=eps),
                          after=dict(theta=eng.theta.clone(), avg=eng.avg.clone(), mom=eng.mom.clone())))
    eng.agc_sgd_step = wrapped


def _judge(eng, s, label):
    lr, clip, torch_clip = s["args"]
    b, a = s["before"], s["after"]
    norm2 = float(b["norms2"][0])
    coef, hit = (adam_ref.torch_clip_coef_ref if torch_clip else clip_coef_ref)(norm2, clip)
    rows = eng.agc_unit_table().tolist()
    ref = agc_ref.agc_ref(b["theta"], b["avg"], b["mom"], rows, coef, hit, dict(s["hyp"], lr=lr, torch_clip=torch_clip), b["first"])
    for key, got in (("param", a["theta"]), ("grad", a["avg"]), ("mom", a["mom"])):
        worst, where = within_bound(got, *ref[key])
        print(f"[wiring {label}] {key}: worst error / bound {worst:.3f} at {where}; units triggered {int(ref['triggered'].sum())} of {int(ref['clipped'].sum())}")
        assert worst <= 1.0, (label, key, worst, where)
    return ref, coef, hit


@pytest.mark.parametrize("modifiers", [False, True], ids=["clip", "clip-noise-norm-bias"])
def test_update_wiring_on_snapshots(modifiers):
    """Three full-batch steps (warm-up 1, clip 0.25 hit) with ``Engine.agc_sgd_step`` wrapped: at every call the arguments are the scheduler's lr
    and the preset's values, ``first_step`` is set for the first call only, and the arenas after the call are within ``agc_ref``'s bounds of the
    arenas before it, with the engine's own unit table.  ``avg`` after the step is the GLOBALLY clipped gradient: units triggered, and none of
    their clip is in it.  With gradient noise and the norm bias on, the clip is applied in place in front of the noise (no clip argument) and
    the gradient the update consumed is not the closure's: the modifiers reach GD-AGC."""
    from fullbatchtraining_amd.training import optim_interface
    over = ["hyp=fbclip", "model=resnet20", "hyp/optim=gd_agc", "hyp.optim.lr=0.03", "hyp.steps=3", "hyp.warmup=1", "hyp.scheduler=cosine-decay",
            "data.batch_size=32", "hyp.sub_batch=32"]
    if modifiers:
        over += ["hyp.grad_noise.additive=0.01", "hyp.norm_bias.strength=0.1"]
    cfg, model, trainer = _trainer(over, 64)
    eng = trainer.engine
    pad = _padding_mask(eng)
    assert int(pad.sum()) > 0
    rows = eng.agc_unit_table().tolist()
    assert sum(r[2] for r in rows) == 3189 and all(r[3] == 1 for r in rows) and eng.agc_unit_table() is eng.agc_unit_table()
    snaps = []
    _wrap(eng, snaps)
    for _ in range(3):
        trainer.step()
    ref_opt, ref_sched = optim_interface(model, cfg.hyp)
    assert len(snaps) == 3
    for i, s in enumerate(snaps):
        lr, clip, torch_clip = s["args"]
        assert lr == ref_opt.param_groups[0]["lr"] and (i > 0 or lr == 0.0) and (i == 0 or lr > 0)
        ref_sched.step()
        assert s["hyp"] == PRESET and torch_clip is False and s["before"]["first"] == (i == 0)
        assert clip == (None if modifiers else 0.25)
        ref, coef, hit = _judge(eng, s, f"modifiers={modifiers} step {i + 1}")
        assert hit == (not modifiers)
        b, a = s["before"], s["after"]
        trig = int(ref["triggered"].sum())
        assert trig > 0 and (modifiers or trig < 3189)       # (per-element noise of 0.01 is above most units' 1 % of the parameter norm)
        if i == 0:                       # lr 0: the parameters keep their bits, the momentum leaves zero
            assert torch.equal(a["theta"].view(torch.int32), b["theta"].view(torch.int32)) and not bool(b["mom"].any()) and bool(a["mom"].any())
        else:
            assert torch.equal(b["mom"], snaps[i - 1]["after"]["mom"]) and not torch.equal(a["theta"], b["theta"])
        for t in a.values():             # the arena's alignment padding stays exactly 0
            assert not bool(t[pad].any())
        if modifiers:
            assert torch.equal(a["avg"], b["avg"])
        else:                            # avg = coef * avg: the global clip, in triggered units too
            assert not torch.equal(a["avg"], b["avg"])
            assert float((a["avg"].double() - coef * b["avg"].double()).abs().max()) <= 8 * 2.0 ** -24 * float(b["avg"].abs().max())
    assert trainer.stats["clipped_step"] == [1, 1, 1]


def test_update_wiring_in_the_stochastic_branch():
    """One epoch of two mini-batch updates: the torch clip form, ``avg`` read only, the weight copies of the next block made from the new parameters
    (the second update's gradient differs from the first's)."""
    over = ["hyp=base_sgd", "model=resnet20", "hyp/optim=gd_agc", "hyp.optim.lr=0.03", "hyp.steps=1", "hyp.warmup=0", "hyp.grad_clip=0.5", "data.batch_size=32"]
    cfg, model, trainer = _trainer(over, 64)
    eng = trainer.engine
    snaps = []
    _wrap(eng, snaps)
    trainer.step()
    trainer.flush_stats()
    assert len(snaps) == 2
    for i, s in enumerate(snaps):
        lr, clip, torch_clip = s["args"]
        assert (clip, torch_clip) == (0.5, True) and s["hyp"] == PRESET and s["before"]["first"] == (i == 0) and lr > 0
        _judge(eng, s, f"stochastic update {i + 1}")
        assert torch.equal(s["after"]["avg"].view(torch.int32), s["before"]["avg"].view(torch.int32))
    assert not torch.equal(snaps[0]["before"]["avg"], snaps[1]["before"]["avg"])


# --------------------------------------------------------------------------------------------------------------- checkpoints --
def test_gd_agc_checkpoint_resumes_bit_for_bit_and_has_the_reference_layout(golden_agc, tmp_path):
    """2 steps, save, resume in a fresh trainer, 1 step = 3 uninterrupted steps: parameters, buffers and momentum, bit for bit.  The saved
    optimizer state has the key structure of the reference's own checkpoint (meta_agc.json): one group per tensor with its name, clipping and
    eps; ``momentum_buffer`` state.  cosine-4000: the lr of a step does not depend on hyp.steps."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    data, meta = golden_agc
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    extra = ["hyp.scheduler=cosine-4000", "hyp.warmup=2"]
    _run(meta, "agc_plain", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=2"], tmp_path)
    assert torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)[4] == 2
    _, _, stats_r = _run(meta, "agc_plain", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=3"], tmp_path)
    _, _, stats_s = _run(meta, "agc_plain", extra + ["impl.checkpoint.name=straight.pth", "hyp.steps=3"], tmp_path)
    assert len(stats_r["train_loss"]) == 1 and len(stats_s["train_loss"]) == 3 and stats_r["train_loss"][-1] == stats_s["train_loss"][-1]
    resumed = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    straight = torch.load(tmp_path / "checkpoints" / "straight.pth", weights_only=False)
    assert resumed[4] == straight[4] == 3 and resumed[3] is None
    for (k, a), b in zip(resumed[1].items(), straight[1].values()):
        assert torch.equal(a, b), k
    model = construct_model(compose(meta["scenarios"]["agc_plain"]["overrides"]).model, 3, 10)
    names = [n for n, _ in model.named_parameters()]
    assert len(resumed[0]["state"]) == len(straight[0]["state"]) == len(names)
    for i in range(len(names)):
        a, b = resumed[0]["state"][i], straight[0]["state"][i]
        assert set(a) == {"momentum_buffer"} and torch.equal(a["momentum_buffer"], b["momentum_buffer"]) and bool(a["momentum_buffer"].any()), i
    assert resumed[0]["param_groups"] == straight[0]["param_groups"]
    # the reference's own checkpoint (ResNet-20, one step): same groups, same keys, same shapes and dtypes
    want = meta["checkpoint"]
    groups = resumed[0]["param_groups"]
    assert want["optimizer"] == "SGD_AGC" and want["n_state"] == want["n_groups"] == len(names) == len(groups)
    assert [g["name"] for g in groups] == want["group_names"] == names
    assert adam_ref.describe(resumed[0]["state"][0]) == want["state0"] and adam_ref.describe(resumed[0]["state"][len(names) - 1]) == want["state_last"]
    for mine, theirs in ((adam_ref.describe(groups[0]), want["group0"]), (adam_ref.describe(groups[-1]), want["group_last"])):
        assert set(mine) == set(theirs)
        for key in ("name", "params", "momentum", "dampening", "weight_decay", "nesterov", "clipping", "eps"):
            assert mine[key] == theirs[key], key
    assert sorted(resumed[2]) == want["scheduler_keys"]


# --------------------------------------------------------------------------------------------------------------- other paths --
def test_gd_agc_bf16_runs_and_tracks_the_f32_engine_on_the_first_step(golden_agc, tmp_path):
    """impl.mixed_precision=True: three finite steps; the first record (taken at the initial parameters) within the looseness the project gives
    bf16 against fp32 -- 2e-2 on losses and the parameter norm, 0.1 on the gradient norm -- of the f32 ENGINE run."""
    data, meta = golden_agc
    _, _, f32 = _run(meta, "agc_plain", (), tmp_path)
    cfg, _, bf16 = _run(meta, "agc_plain", ["impl.mixed_precision=True"], tmp_path)
    assert cfg.impl.mixed_precision is True
    for key in ("train_loss", "full_loss", "param_norm", "grad_norm"):
        print(f"bf16 {key}: {np.array(bf16[key])} f32 engine {np.array(f32[key])}")
        assert len(bf16[key]) == 3 and np.all(np.isfinite(bf16[key]))
        assert abs(bf16[key][0] - f32[key][0]) <= (0.1 if key == "grad_norm" else 2e-2) * abs(f32[key][0]), key
    assert bf16["param_norm"][2] != bf16["param_norm"][0]          # (the updates did move the parameters)


def test_gd_agc_with_ema_and_test_time_flips_evaluates(golden_agc, tmp_path):
    data, meta = golden_agc
    _, model, stats = _run(meta, "agc_plain", ["hyp.evaluate_ema=True", "hyp.test_time_flips=True", "impl.validate_every_nth_step=1"], tmp_path)
    assert len(stats["valid_loss"]) == 3 and np.all(np.isfinite(stats["valid_loss"])) and all(0.0 <= a <= 1.0 for a in stats["valid_acc"])
    assert len(stats["train_loss"]) == 3 and np.all(np.isfinite(stats["train_loss"]))
