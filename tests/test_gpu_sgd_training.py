"""Mini-batch SGD mode (``hyp.train_stochastic``) end to end on the GPU: ``train()`` against runs of the REAL reference's stochastic branch
(tests/golden/scenarios_sgd.npz) and against the float64 restatement (tests/sgd_ref.py); the fused update against the composition bit for
bit in fresh processes; the recorded launch lists, checkpoints, bf16 and a learnable dataset."""
import os
import subprocess
import sys

import json
import numpy as np
import pytest
import torch

from tests import sgd_ref
from tests.helpers import err_cos, hyp_from_cfg, make_data, oracle_device, rel_err, shuffling_loaders, summarise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
STAT_KEYS = ("train_loss", "train_acc", "param_norm", "grad_norm", "full_loss")
SETUP = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)


@pytest.fixture(scope="module")
def golden_sgd():
    with open(os.path.join(HERE, "golden", "meta_sgd.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "golden", "scenarios_sgd.npz"))), meta


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
    if "shuffle" in name:                      # the loaders the reference run was given (RandomSampler, shared generator)
        tl, vl = shuffling_loaders(x, y, cfg.data.batch_size)
        return cfg, model, train(model, tl, vl, SETUP, cfg)
    return cfg, model, train(model, (x, y), (x[:64], y[:64]), SETUP, cfg)


# tol: the values of test_train_matches_reference_run_f32's table -- 2e-4 plain, 3e-3 with the regulariser
@pytest.mark.parametrize("name,tol", [("sgd_plain", 2e-4), ("sgd_ragged", 2e-4), ("sgd_smooth", 2e-4), ("sgd_shuffle_reg", 3e-3)])
def test_sgd_train_matches_reference_run_f32(golden_sgd, name, tol, tmp_path):
    """The bound form of test_train_matches_reference_run_f32: every statistic within ``tol`` of the reference's float64 run, or within 5x the
    reference's own fp32-vs-float64 spread (admissible scenarios only: that spread is below 1e-3 on the losses and the parameter norm)."""
    data, meta = golden_sgd
    assert meta["judged_at"][name] == tol
    cfg, model, stats = _run(meta, name, (), tmp_path)
    assert cfg.hyp.train_stochastic is True
    for key in STAT_KEYS:
        r64, r32 = data[f"{name}@f64/stat/{key}"], data[f"{name}/stat/{key}"]
        print(f"{name} {key}: engine {np.array(stats[key])} ref32 {r32} ref64 {r64}")
        bound = np.maximum(tol * np.abs(r64) + 1e-6, 5 * np.abs(r32 - r64))
        if key == "train_acc":       # one prediction may flip on the fp32 noise floor
            bound = np.maximum(bound, 1.0 / meta["scenarios"][name]["n"] + 1e-9)
        assert len(stats[key]) == len(r64) and np.all(np.abs(np.array(stats[key]) - r64) <= bound), (key, stats[key], r32, r64)
    assert "preclip_gradnorm" not in stats and "clipped_step" not in stats          # _modify_gradient_params is not part of the branch
    n_blocks = len([k for k in stats if k.startswith("grad_norm_train_")])
    assert n_blocks == meta["scenarios"][name]["n"] // cfg.data.batch_size
    for k in range(n_blocks):
        r64, r32 = data[f"{name}@f64/stat/grad_norm_train_{k}"], data[f"{name}/stat/grad_norm_train_{k}"]
        bound = np.maximum(max(tol, 1e-3) * np.abs(r64), 5 * np.abs(r32 - r64))
        print(f"{name} grad_norm_train_{k}: engine {np.array(stats[f'grad_norm_train_{k}'])} ref32 {r32} ref64 {r64}")
        assert np.all(np.abs(np.array(stats[f"grad_norm_train_{k}"]) - r64) <= bound), (k, stats[f"grad_norm_train_{k}"], r32, r64)
    err = rel_err(summarise([v.double() for v in model.state_dict().values()])[1], data[f"{name}@f64/final_sample"])
    noise = rel_err(data[f"{name}/final_sample"], data[f"{name}@f64/final_sample"])
    print(f"{name}: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e})")
    assert err < max(10 * noise, 1e-5)
    rm_err = rel_err(model.state_dict()["stem.1.running_mean"].double().numpy(), data[f"{name}@f64/final_stem_running_mean"])
    rm_noise = rel_err(data[f"{name}/final_stem_running_mean"], data[f"{name}@f64/final_stem_running_mean"])
    print(f"{name}: stem running_mean engine-vs-ref64 {rm_err:.2e} (reference fp32-vs-f64 {rm_noise:.2e})")
    assert rm_err < max(10 * rm_noise, 2e-3)
    assert int(model.state_dict()["stem.1.num_batches_tracked"]) == int(data[f"{name}@f64/final_num_batches_tracked"][0])
    assert len(stats["valid_loss"]) >= 1 and np.isfinite(stats["valid_loss"][-1])
    # the branch ends every update with optimizer.zero_grad() (reference training.py:282): what that leaves under the installed torch
    p = torch.nn.Parameter(torch.zeros(2))
    p.grad = torch.ones(2)
    torch.optim.SGD([p], lr=0.1).zero_grad()
    assert all((q.grad is None) if p.grad is None else (q.grad is not None and not q.grad.any()) for q in model.parameters())


def _trainer(over, n_blocks, seed=5):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    cfg = compose(list(over) + ["impl.validate_every_nth_step=1000"])
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(n_blocks * cfg.data.batch_size, cfg.data.pixels)
    return cfg, model, x, y, FullBatchTrainer(model, (x, y), None, SETUP, cfg)


@pytest.mark.parametrize("reg", [False, True], ids=["clip", "clip-regulariser"])
def test_one_sgd_epoch_from_a_given_state_against_float64(reg):
    """One epoch of 4 blocks of 32 (ResNet-18, 16 px, clip + Nesterov momentum, lr 0.005) against tests/sgd_ref.py in float64: parameters,
    momentum, running statistics.

    A mini-batch trajectory amplifies fp32 noise: the gradient of block k is taken at parameters that carry the noise of blocks < k (tiny
    BatchNorm batches, ReLU masks), so after four updates the plain fp32 evaluation of the restatement itself -- torch's own kernels, no
    engine code -- sits 2e-2 (displacement) and 3e-2 (momentum) from its float64 twin at this lr, and 0.15 / 0.25 at lr 0.05.  The engine is
    therefore held to the rule tests/test_gpu_running_stats.py uses for such quantities: within 5x what that fp32 evaluation gets, but not
    below a floor -- 1e-2, the bound of ONE chunk gradient in tests/test_gpu_engine.py, for the relative L2 error of the momentum and for the
    parameter error relative to the DISPLACEMENT |theta'_64 - theta_0| (the update is linear in the gradients); 1e-5 for the running statistics
    (per layer, max over channels of |d mean| / std and |d var| / var).  num_batches_tracked exactly; the losses to 1e-3."""
    over = ["hyp=base_sgd", "model=resnet18", "data.pixels=16", "data.batch_size=32", "hyp.steps=3", "hyp.warmup=0", "hyp.optim.lr=0.005",
            "hyp.grad_clip=2.0"] + (["hyp.grad_reg.block_strength=0.5"] if reg else [])
    cfg, model, x, y, trainer = _trainer(over, 4)
    eng = trainer.engine
    theta0 = eng.theta.double().clone()
    trainer.step()
    trainer.flush_stats()
    dev = oracle_device()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        state = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()).to(dev) for k, v in model.state_dict().items()}
        net = sgd_ref.Net(cfg.model, model)
        st = sgd_ref.train_sgd(net, state, x.to(dev, dtype), y.to(dev), hyp_from_cfg(cfg), 1, 32, cfg.hyp.scheduler, cfg.hyp.warmup)
        runs[dtype] = (state, st)
    state, st = runs[torch.float64]
    names = [k for k, _ in model.named_parameters()]

    def flat(tensors):
        return torch.cat([t.detach().reshape(-1).double().cpu() for t in tensors])

    theta64, mom64 = flat([state[k] for k in names]), flat(st["_momentum"])
    theta0 = flat(eng.unflatten_list(theta0))
    disp = float((theta64 - theta0).norm())
    y_theta = float((flat([runs[torch.float32][0][k] for k in names]) - theta64).norm()) / disp
    y_mom, _ = err_cos(flat(runs[torch.float32][1]["_momentum"]), mom64)
    e_theta = float((flat(eng.unflatten_list(eng.theta)) - theta64).norm()) / disp
    e_mom, cos = err_cos(flat(eng.unflatten_list(eng.mom)), mom64)
    print(f"[reg={reg}] parameters: error / displacement {e_theta:.2e} (fp32 restatement {y_theta:.2e}; |displacement| {disp:.3e}); "
          f"momentum: rel {e_mom:.2e} (fp32 restatement {y_mom:.2e}), 1 - cos {1 - cos:.1e}")
    assert e_theta <= max(5 * y_theta, 1e-2) and e_mom <= max(5 * y_mom, 1e-2)
    assert eng.num_batches_tracked == int(state["stem.1.num_batches_tracked"]) == 4 * (2 if reg else 1)
    fails = []
    yard = runs[torch.float32][0]
    for L in eng.plan.layers:
        r_m, r_v = state[f"{L.bn_name}.running_mean"].double().cuda(), state[f"{L.bn_name}.running_var"].double().cuda()
        std, var = (r_v + 1e-5).sqrt(), r_v + 1e-5
        e_m = float(((eng.running_mean[L.ch_off:L.ch_off + L.cout].double() - r_m).abs() / std).max())
        e_v = float(((eng.running_var[L.ch_off:L.ch_off + L.cout].double() - r_v).abs() / var).max())
        y_m = float(((yard[f"{L.bn_name}.running_mean"].double().cuda() - r_m).abs() / std).max())
        y_v = float(((yard[f"{L.bn_name}.running_var"].double().cuda() - r_v).abs() / var).max())
        print(f"  {L.bn_name:28s} mean {e_m:.2e} | {y_m:.2e}   var {e_v:.2e} | {y_v:.2e}")
        if not (e_m <= max(5 * y_m, 1e-5) and e_v <= max(5 * y_v, 1e-5)):
            fails.append((L.bn_name, e_m, y_m, e_v, y_v))
    assert not fails, fails
    for key in ("train_loss", "param_norm", "full_loss"):
        assert abs(trainer.stats[key][0] - st[key][0]) <= 1e-3 * abs(st[key][0]), (key, trainer.stats[key], st[key])


def _child(out, over, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "FB_SGD_FUSED"}
    env.update(env_extra)
    res = subprocess.run([sys.executable, "-m", "tests.sgd_child", str(out)] + list(over), cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("over", [
    ["hyp.grad_clip=2.0", "hyp.grad_reg.block_strength=0.5"],                       # fp32 copies, a second recorded list for the perturbed pass
    ["hyp.grad_clip=2.0", "impl.mixed_precision=True"],                             # bf16 copies
], ids=["f32-clip-regulariser", "bf16-clip"])
def test_fused_update_and_composition_give_the_same_bits_over_two_epochs(over, tmp_path):
    """FB_SGD_FUSED=0 (fb_mt_sgd_torch + fb_weight_prep per layer) and the default (one fb_mt_sgd_prep launch), each in a fresh process under its
    own time limit: parameters, momentum, running statistics and every statistic of two epochs of 4 blocks carry the same bits."""
    base = ["hyp=base_sgd", "model=resnet20", "data.pixels=16", "data.batch_size=32", "hyp.steps=2", "hyp.warmup=0", "hyp.optim.lr=0.05"] + over
    fused = _child(tmp_path / "fused.npz", base, {})
    comp = _child(tmp_path / "comp.npz", base, {"FB_SGD_FUSED": "0"})
    assert int(comp["fused"][0]) == 0
    assert int(fused["fused"][0]) == 1, "the fused update is not the default: compare FB_EXPERIMENTAL"
    assert set(fused) == set(comp) and any(k.startswith("stat/grad_norm_train_3") for k in fused)
    for key in fused:
        if key in ("fused", "cmdlists", "replays"):
            continue
        assert np.array_equal(fused[key].view(np.uint8), comp[key].view(np.uint8)), key
    assert len(fused["stat/train_loss"]) == 2 and np.all(np.isfinite(fused["stat/train_loss"])) and float(np.abs(fused["mom"]).max()) > 0


def test_recorded_lists_do_not_grow_with_the_number_of_blocks():
    """One fixed staging buffer: an epoch of 8 blocks leaves as many recorded launch lists as an epoch of 2, and later blocks replay them."""
    over = ["hyp=base_sgd", "model=resnet20", "data.pixels=16", "data.batch_size=32", "hyp.steps=4", "hyp.warmup=0", "hyp.optim.lr=0.05",
            "hyp.grad_reg.block_strength=0.5"]
    counts = {}
    for n_blocks in (2, 8):
        _, _, _, _, trainer = _trainer(over, n_blocks)
        eng = trainer.engine
        trainer.step()
        first = (len(eng.cmdlists), eng.replays)
        trainer.step()
        trainer.flush_stats()
        counts[n_blocks] = (first, (len(eng.cmdlists), eng.replays))
        assert eng.unrecorded_runs == 0 and eng.cmd_evictions == 0
        assert len(trainer.stats["grad_norm_train_%d" % (n_blocks - 1)]) == 2
    print(counts)
    assert counts[8][0][0] == counts[2][0][0] == counts[8][1][0] == counts[2][1][0] <= 6
    assert counts[8][0][1] > counts[2][0][1] > 0 and counts[8][1][1] > counts[8][0][1]


def test_sgd_checkpoint_after_epoch_1_resumes_epoch_2_bit_for_bit(golden_sgd, tmp_path):
    """5-list checkpoint written after epoch 1, resumed in a new trainer: epoch 2 has the bits of the uninterrupted run (parameters, momentum
    buffers, running statistics, statistics).  cosine-4000: the lr of an epoch does not depend on hyp.steps."""
    data, meta = golden_sgd
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    extra = ["hyp.scheduler=cosine-4000", "hyp.warmup=0", "hyp.optim.lr=0.02"]
    _, first, _ = _run(meta, "sgd_ragged", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=1"], tmp_path)
    optim_state, model_state, sched_state, scaler_state, step = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    assert step == 1 and scaler_state is None and len(optim_state["state"]) == len(list(first.parameters()))
    assert all(tuple(optim_state["state"][i]["momentum_buffer"].shape) == tuple(p.shape) for i, p in enumerate(first.parameters()))
    _, resumed, stats_r = _run(meta, "sgd_ragged", extra + ["impl.checkpoint.name=ck.pth", "hyp.steps=2"], tmp_path)
    _, straight, stats_s = _run(meta, "sgd_ragged", extra + ["hyp.steps=2"], tmp_path)
    assert len(stats_r["train_loss"]) == 1 and len(stats_s["train_loss"]) == 2
    for key in STAT_KEYS + tuple(f"grad_norm_train_{k}" for k in range(4)):
        assert stats_r[key][-1] == stats_s[key][-1], (key, stats_r[key], stats_s[key])
    for (k, a), b in zip(resumed.state_dict().items(), straight.state_dict().values()):
        assert torch.equal(a, b), k


def test_sgd_bf16_tracks_fp32_statistics(golden_sgd, tmp_path):
    """impl.mixed_precision=True with the tolerances of test_train_bf16_tracks_fp32_statistics: 2e-2 on losses / parameter norm, 0.1 on the
    gradient norm, against the reference's float64 run."""
    data, meta = golden_sgd
    cfg, model, stats = _run(meta, "sgd_plain", ["impl.mixed_precision=True"], tmp_path)
    for key in ("train_loss", "full_loss", "param_norm", "grad_norm"):
        r64 = data[f"sgd_plain@f64/stat/{key}"]
        print(f"bf16 {key}: engine {np.array(stats[key])} ref64 {r64}")
        assert np.allclose(stats[key], r64, rtol=2e-2 if key != "grad_norm" else 0.1), key
    assert abs(stats["train_acc"][0] - data["sgd_plain@f64/stat/train_acc"][0]) < 0.02


@pytest.mark.parametrize("mixed", [False, True])
def test_sgd_fits_a_learnable_dataset(mixed, tmp_path):
    """The recipe of test_full_batch_descent_fits_a_learnable_dataset (512 images whose labels are a function of the inputs, 25 "steps", clip
    + warm-up + Nesterov momentum, lr 0.1) under mini-batch SGD -- 4 updates per epoch -- reaches the same thresholds."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import train

    gen = torch.Generator().manual_seed(7)
    n, pixels = 512, 16
    protos = torch.randn(10, 3, pixels, pixels, generator=gen)
    y = torch.randint(0, 10, (n,), generator=gen)
    x = protos[y] + 0.5 * torch.randn(n, 3, pixels, pixels, generator=gen)
    cfg = compose(["hyp=base_sgd", "hyp.steps=25", "hyp.warmup=5", "hyp.optim.lr=0.1", "hyp.grad_clip=1.0", "data.batch_size=128",
                   f"data.pixels={pixels}", "impl.validate_every_nth_step=1000", f"impl.mixed_precision={mixed}"], original_cwd=str(tmp_path), name="fit")
    assert cfg.hyp.train_stochastic is True
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, 10)
    stats = train(model, (x, y), (x, y), SETUP, cfg)
    loss, acc = np.array(stats["train_loss"]), np.array(stats["train_acc"])
    print(f"mixed={mixed}: loss {loss[[0, 5, 10, 15, 20, 24]]}, acc {acc[[0, 5, 10, 15, 20, 24]]}, valid_acc {stats['valid_acc']}")
    assert np.all(np.isfinite(loss)) and loss[-1] < 0.25 * loss[0] and acc[-1] > 0.95
    assert stats["valid_acc"][-1] > 0.9
    assert len(loss) == 25 and len(stats["grad_norm_train_3"]) == 25


def test_default_configuration_trains_an_epoch(tmp_path):
    """``compose([])`` -- hyp=base_sgd, ResNet-18, blocks of 128 -- is no longer refused: one epoch over 256 images at 32 px."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import train

    cfg = compose(["hyp.steps=1"], original_cwd=str(tmp_path), name="default")
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(256, cfg.data.pixels)
    stats = train(model, (x, y), (x[:64], y[:64]), SETUP, cfg)
    assert len(stats["train_loss"]) == 1 and np.isfinite(stats["train_loss"][0]) and "grad_norm_train_1" in stats and "grad_norm_train_2" not in stats
