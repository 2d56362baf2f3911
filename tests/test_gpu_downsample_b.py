"""The strided 1x1 shortcut (``model.downsample=B``, reference resnets.py:142-146) on the GPU: the two subsample kernels against torch
slicing, ResNet-20/B and ResNet-50/B chunk gradients against float64 autograd through the parameter container's own ``forward`` (the oracle
of ``oracle/`` knows the 'C' shortcut only), the schedules (replayed command lists, two streams, host callback, finite-difference weight
sets) bit for bit, and ``train()`` against runs of the REAL reference (tests/golden/make_golden_dsb.py).

Bounds are those of the tests these follow in tests/test_gpu_engine.py and tests/test_gpu_training.py.  The bf16 yardstick -- torch's own
``autocast(bfloat16)`` run of the same net -- means something at this shape: on the host it has cosine 0.954 .. 0.963 to the float64 truth
for ResNet-20/B at 16 px with chunks of 32 (relative distance 0.27 .. 0.30), well above the 0.9 below which the comparison would be noise.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import confined, err_cos, flat64, make_data, oracle_device, rel_err, summarise, torch_bf16_chunk_grads

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAT_KEYS = ("train_loss", "train_acc", "param_norm", "grad_norm", "full_loss", "preclip_gradnorm", "clipped_step")
R20 = ("model=resnet20",)
R50 = ("model=resnet50", "model.stem=standard", "model.downsample=B")


@pytest.fixture(scope="module")
def dsb():
    with open(os.path.join(HERE, "meta_dsb.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "scenarios_dsb.npz"))), meta


# ------------------------------------------------------------------------------------------------------------------ kernels --
@pytest.mark.parametrize("shape", [(3, 8, 8, 64), (2, 7, 7, 256), (5, 16, 16, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_subsample_kernels_against_torch_slicing(dtype, shape):
    """Through tests/helpers.py ``confined``: guard bands on both sides of every operand stay untouched, the inputs keep their bytes, and the results do not
    depend on what surrounds the operands (nor, for the copy, on what the output held before)."""
    from fullbatchtraining_amd import lib

    n, H, W, C = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dtc = lib.dtype_code(dtype)
    gen = torch.Generator().manual_seed(17 + H + C)
    x = torch.randn(n, H, W, C, generator=gen).to(dtype)
    y = confined(lambda o: lib.call("fb_subsample2_fwd", o["x"].data_ptr(), o["y"].data_ptr(), n, H, W, C, dtc), {"x": x}, {"y": ((n, Ho, Wo, C), dtype)})["y"]
    assert torch.equal(y.cpu(), x[:, ::2, ::2])                                      # a copy: bit-exact
    # in-place scatter-add: fp32 sum, one rounding to the storage type (dx is an accumulator: it keeps its content, its surroundings are filled)
    dx = torch.randn(n, H, W, C, generator=gen).to(dtype)
    dy = (torch.randn(n, Ho, Wo, C, generator=gen) * 1.7).to(dtype)
    want = dx.clone()
    want[:, ::2, ::2] = (dx.float()[:, ::2, ::2] + dy.float()).to(dtype)
    got = confined(lambda o: lib.call("fb_subsample2_bwd_add", o["dx"].data_ptr(), o["dy"].data_ptr(), n, H, W, C, dtc), {"dy": dy}, {}, inout={"dx": dx})["dx"].cpu()
    assert torch.equal(got[:, ::2, ::2], want[:, ::2, ::2])
    rest = torch.ones(H, W, dtype=torch.bool)
    rest[::2, ::2] = False
    assert torch.equal(got[:, rest], dx[:, rest])                                    # every other position: the bits from before
    assert not torch.equal(got, dx)


@pytest.mark.parametrize("dtype,C", [(torch.float32, 66), (torch.bfloat16, 68)], ids=["f32-66", "bf16-68"])
def test_subsample_kernels_refuse_channels_that_do_not_form_16_byte_vectors(dtype, C):
    from fullbatchtraining_amd import lib

    n, H = 2, 8
    x = torch.zeros(n, H, H, C, dtype=dtype, device="cuda")
    y = torch.zeros(n, H // 2, H // 2, C, dtype=dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for name in ("fb_subsample2_fwd", "fb_subsample2_bwd_add"):
        assert getattr(lib.load(), name)(x.data_ptr(), y.data_ptr(), n, H, H, C, lib.dtype_code(dtype), st) == -1       # FB_ERR_ARG
        with pytest.raises(lib.EngineError, match="16-byte vectors"):
            lib.call(name, x.data_ptr(), y.data_ptr(), n, H, H, C, lib.dtype_code(dtype))
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0 and float(y.abs().max()) == 0


# ------------------------------------------------------------------------------------------------------- chunk gradients --
def _build(over=R20, pixels=16, chunk=32, G=3, dtype=torch.float32, seed=0, fd_sets=0, f32_split=None):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.models import construct_model

    cfg = compose(list(over))
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    eng = Engine(model, pixels, chunk, G, compute_dtype=dtype, fd_sets=fd_sets, f32_split=f32_split)
    assert any(b.kind == "B" and b.pooled is not None for b in eng.plan.blocks)
    return cfg, model, eng, stem_patches


_TRUTH = {}


def _truth(over, model, x, y, chunk):
    """[(gradient list on the host, loss, #correct) per chunk]: float64 autograd through the container's own plain-torch ``forward`` in
    train mode -- computed once per configuration (the models are seeded: same parameters in every test) and shared."""
    key = (tuple(over), tuple(x.shape), chunk)
    if key not in _TRUTH:
        dev = oracle_device()
        m = copy.deepcopy(model).double().to(dev).train()
        params = list(m.parameters())
        out = []
        for k in range(x.shape[0] // chunk):
            xb, yb = x[k * chunk:(k + 1) * chunk].double().to(dev), y[k * chunk:(k + 1) * chunk].to(dev)
            logits = m(xb)
            loss = torch.nn.functional.cross_entropy(logits, yb)
            grads = torch.autograd.grad(loss, params)
            out.append(([g.detach().cpu() for g in grads], float(loss.detach()), float((logits.argmax(-1) == yb).sum())))
        _TRUTH[key] = out
    return _TRUTH[key]


def _engine_grads_as_lists(eng, G):
    flat = eng.g[:G].cpu()
    return [[eng._unflatten(flat[g], name) for name in eng.plan.param_names] for g in range(G)]


def _group_gradient(eng, stem_patches, x, y, G, dtype):
    patches = stem_patches(x.cuda(), eng.plan.stem, dtype)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    torch.cuda.synchronize()
    return _engine_grads_as_lists(eng, G)


@pytest.mark.parametrize("split", ["bf16x6", "f16x2"])
def test_resnet20b_chunk_gradients_f32_vs_float64_autograd(split):
    """The bounds of test_resnet18_chunk_gradients_vs_oracle.  ``f16x2``: the opt-in fp32 arithmetic (22-bit operands) that tracks max|.| of
    the tensors it writes -- the in-place ``fb_subsample2_bwd_add`` drops whatever was recorded for the input gradient it completes, so a
    later consumer measures the completed tensor; held to the gradient bounds test_f32_split_modes_regularised_mean_gradient_vs_oracle
    holds that mode to (the same 1e-2 / 0.99999)."""
    pixels, chunk, G = 16, 32, 3
    cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, torch.float32, f32_split=split)
    assert eng.f32_split == split
    x, y = make_data(chunk * G, pixels)
    truth = _truth(R20, model, x, y, chunk)
    got = _group_gradient(eng, stem_patches, x, y, G, torch.float32)
    for g in range(G):
        a, t = flat64(got[g]), flat64(truth[g][0])
        err, cos = err_cos(a, t)
        fc = rel_err(got[g][-2].numpy(), truth[g][0][-2].numpy())
        print(f"[resnet20/B f32 {split}] chunk {g}: engine-vs-f64 {err:.3e} cos {cos:.7f} fc {fc:.2e}; loss {float(eng.loss[g]):.7f} vs {truth[g][1]:.7f}")
        assert err < 1e-2 and cos > 0.99999, (g, err, cos)
        if split == "bf16x6":                                  # exact fp32 products: loss, predictions and the well-conditioned classifier gradient are sharp
            assert abs(float(eng.loss[g]) - truth[g][1]) < 1e-5 * max(1.0, abs(truth[g][1]))
            assert float(eng.correct[g]) == truth[g][2]
            assert fc < 1e-4, (g, fc)


def test_resnet20b_chunk_gradients_bf16_vs_torch_autocast_yardstick():
    pixels, chunk, G = 16, 32, 3
    cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, torch.bfloat16)
    x, y = make_data(chunk * G, pixels)
    truth = _truth(R20, model, x, y, chunk)
    got = _group_gradient(eng, stem_patches, x, y, G, torch.bfloat16)
    yard = torch_bf16_chunk_grads(model, x, y, chunk)
    for g in range(G):
        t = flat64(truth[g][0])
        e_eng, c_eng = err_cos(flat64(got[g]), t)
        e_tch, c_tch = err_cos(flat64(yard[g][0]), t)
        print(f"[resnet20/B bf16] chunk {g}: engine {e_eng:.3f} / cos {c_eng:.4f}; torch autocast(bf16) {e_tch:.3f} / cos {c_tch:.4f}; "
              f"loss {float(eng.loss[g]):.5f} vs {yard[g][1]:.5f} (truth {truth[g][1]:.5f})")
        assert c_tch > 0.9                                     # the yardstick itself is above the noise at this shape
        assert e_eng <= 1.15 * e_tch, (g, e_eng, e_tch)
        assert c_eng >= c_tch - 0.01, (g, c_eng, c_tch)
        assert abs(float(eng.loss[g]) - yard[g][1]) < 2e-2 * max(1.0, abs(yard[g][1]))


def test_resnet50b_standard_stem_chunk_gradients_vs_float64_autograd():
    """Bottleneck blocks: a stride-1 'B' shortcut (first stage: the 'C' schedule under other key names) and three stride-2 ones, at the shape
    and with the bounds of test_bottleneck_standard_stem_chunk_gradients_vs_oracle."""
    pixels, chunk, G = 64, 32, 2
    cfg, model, eng, stem_patches = _build(R50, pixels, chunk, G, torch.float32)
    kinds = [(b.kind, b.stride, b.pooled is not None) for b in eng.plan.blocks if b.shortcut is not None]
    assert kinds == [("B", 1, False), ("B", 2, True), ("B", 2, True), ("B", 2, True)]
    x, y = make_data(chunk * G, pixels)
    truth = _truth(R50, model, x, y, chunk)
    got = _group_gradient(eng, stem_patches, x, y, G, torch.float32)
    for g in range(G):
        err, cos = err_cos(flat64(got[g]), flat64(truth[g][0]))
        fc = rel_err(got[g][-2].numpy(), truth[g][0][-2].numpy())
        print(f"[resnet50/B standard stem] chunk {g}: engine-vs-f64 {err:.3e} cos {cos:.6f} fc {fc:.2e}; loss {float(eng.loss[g]):.7f} vs {truth[g][1]:.7f}")
        assert abs(float(eng.loss[g]) - truth[g][1]) < 1e-5 * abs(truth[g][1])
        assert err < 5e-2, err
        assert fc < 1e-4, fc


# -------------------------------------------------------------------------------------------------------------- schedules --
@pytest.mark.parametrize("dtype,fd", [(torch.bfloat16, 0), (torch.float32, 1)], ids=["bf16", "f32-fd"])
def test_replayed_command_lists_equal_interpreted_launches_for_the_b_plan(dtype, fd, monkeypatch):
    """test_replayed_command_lists_equal_interpreted_launches on the ResNet-20/B plan: the recording takes the two subsample calls (a call the
    native executor does not know raises while recording), nothing runs unrecorded, and three steps of replayed lists equal three steps of
    interpreted launches bit for bit -- plain bf16 and the fp32 finite-difference passes (per-chunk weight sets), ragged last group."""
    pixels, chunk, G, n_chunks = 16, 32, 3, 5
    x, y = make_data(chunk * n_chunks, pixels)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("FB_REPLAY", mode)
        cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, dtype, fd_sets=fd)
        assert eng.use_replay == (mode == "1")
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
        trace = []
        for step in range(3):
            loss, correct, sq = eng.full_gradient(patches, yd, 0.1, block_strength=0.5 if fd else 0.0)
            eng.grad_and_param_sqnorm()
            eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True, grad_clip=0.25)
            trace.append((loss.clone(), correct.clone(), sq.clone()))
        torch.cuda.synchronize()
        if mode == "1":
            per_step = 2 * (1 + fd) + 1 + 2 * fd          # group passes + weight preparations, as in the test this follows
            assert eng.replays == 2 * per_step and len(eng.cmdlists) == per_step and eng.unrecorded_runs == 0
        out[mode] = (eng.theta.clone(), eng.mom.clone(), eng.running_mean.clone(), eng.running_var.clone(), trace, eng.num_batches_tracked)
    a, b = out["0"], out["1"]
    assert all(bool(torch.isfinite(t).all()) for t in a[:4]) and not torch.equal(a[1], torch.zeros_like(a[1]))
    for i in range(4):
        assert torch.equal(a[i], b[i]), i
    for ta, tb in zip(a[4], b[4]):
        for u, v in zip(ta, tb):
            assert torch.equal(u, v)
    assert a[5] == b[5]


@pytest.mark.parametrize("dtype,fd", [(torch.bfloat16, 0), (torch.float32, 1)], ids=["bf16", "f32-fd"])
def test_two_stream_schedule_is_bit_identical_to_one_stream_for_the_b_plan(dtype, fd, monkeypatch):
    """test_two_stream_schedule_is_bit_identical_to_one_stream on the ResNet-20/B plan: the shortcut's weight gradient reads the subsampled
    copy on the second stream, and the in-place add sits between the input-gradient convolution and the hand-back of its operand."""
    pixels, chunk, G, n_chunks = 16, 32, 2, 5
    x, y = make_data(chunk * n_chunks, pixels)

    def run():
        cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, dtype, fd_sets=fd)
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
        trace = []
        for lr in (0.0, 0.4, 0.4):
            loss, correct, sq = eng.full_gradient(patches, yd, lr, block_strength=0.5 if fd else 0.0)
            trace += [loss.clone(), correct.clone(), sq.clone(), eng.avg.clone()]
            eng.grad_and_param_sqnorm()
            eng.sgd_step(lr, 5e-4, 0.9, 0.0, True, grad_clip=0.25)
            trace.append(eng.theta.clone())
        torch.cuda.synchronize()
        return eng, trace + [eng.running_mean.clone(), eng.running_var.clone()]

    monkeypatch.setenv("FB_WGRAD_STREAM", "0")
    monkeypatch.setenv("FB_ACC_OVERLAP", "0")
    eng, ref = run()
    assert eng.wstream is None and all(bool(torch.isfinite(t).all()) for t in ref)
    monkeypatch.setenv("FB_WGRAD_STREAM", "1")
    monkeypatch.delenv("FB_ACC_OVERLAP")
    for rep in range(3):
        eng, got = run()
        assert eng.wstream is not None and eng.use_replay and eng.replays > 0
        for k, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (rep, k, float((a - b).abs().max()))


@pytest.mark.parametrize("dtype,wsets", [(torch.bfloat16, 1), (torch.float32, 2)], ids=["bf16", "f32-wsets"])
def test_on_block_done_path_gives_the_bits_of_the_replayed_path_for_the_b_plan(dtype, wsets):
    """``group_gradient(on_block_done=...)`` (launch by launch, the multi-GPU late bucket) against the recorded and the replayed list; the
    callback fires once per block, last block first."""
    pixels, chunk, G = 16, 32, 3
    cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, dtype, fd_sets=1 if wsets > 1 else 0)
    x, y = make_data(chunk * G, pixels)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
    theta, gout, pidx = eng.theta, eng.g, 0
    if wsets > 1:
        eng.theta_k.copy_(eng.theta[None, :] * (1 + 1e-3 * torch.arange(1, G + 1, device="cuda", dtype=torch.float32)[:, None]))
        theta, gout, pidx = eng.theta_k, eng.g_fd[0], 1
    prep = (lambda: eng.prep_weights(theta, G, per_chunk=True)) if wsets > 1 else (lambda: eng.prep_weights(theta, 1))
    out = []
    for rep in range(2):
        prep()
        eng.group_gradient(patches, yd, G, gout, wsets, theta, pidx)
        torch.cuda.synchronize()
        out.append((gout[:G].clone(), eng.loss[:G].clone(), eng.mean_tab[pidx].clone()))
    assert eng.replays > 0
    seen = []
    prep()
    eng.group_gradient(patches, yd, G, gout, wsets, theta, pidx, on_block_done=seen.append)
    torch.cuda.synchronize()
    assert seen == list(range(len(eng.plan.blocks) - 1, -1, -1)) and eng.plan.late_block == 6
    for ref in out:
        assert torch.equal(ref[0], gout[:G]) and torch.equal(ref[1], eng.loss[:G]) and torch.equal(ref[2], eng.mean_tab[pidx])
    assert bool(torch.isfinite(gout[:G]).all()) and float(gout[:G].abs().max()) > 0


def test_evaluation_of_the_b_plan_vs_float64_eval_mode():
    """``evaluate_batch`` (BatchNorm on running statistics, no statistics pass) after one training step has moved them, against the
    container's float64 ``forward`` in eval mode on the stored state: the loss to 1e-5 (fp32 forward), every prediction but at most one."""
    pixels, chunk, G = 16, 32, 2
    cfg, model, eng, stem_patches = _build(R20, pixels, chunk, G, torch.float32)
    x, y = make_data(chunk * G, pixels)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.float32), y.cuda()
    eng.full_gradient(patches, yd, 0.1)
    eng.grad_and_param_sqnorm()
    eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True)
    loss, correct = eng.evaluate_batch(patches, yd)
    eng.store_to_model(model)
    m = copy.deepcopy(model).double().eval()
    with torch.no_grad():
        logits = m(x.double())
        want = float(torch.nn.functional.cross_entropy(logits, y))
        want_correct = float((logits.argmax(-1) == y).sum())
    print(f"[resnet20/B eval] loss {loss:.7f} vs float64 {want:.7f}; correct {correct} vs {want_correct}")
    assert float(m.layers[1][0].downsample[1].running_mean.abs().max()) > 0
    assert abs(loss - want) < 1e-5 * max(1.0, abs(want)) and abs(correct - want_correct) <= 1


# ----------------------------------------------------------------------------------------------------- train() vs reference --
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
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    stats = train(model, (x, y), (x[:64], y[:64]), setup, cfg)
    return cfg, model, stats


def _judge(data, meta, name, tol, cfg, model, stats, tag=""):
    """The rules of test_train_matches_reference_run_f32, plus the validation pass on the first 64 images."""
    for key in STAT_KEYS:
        if f"{name}@f64/stat/{key}" not in data:
            continue
        r64, r32 = data[f"{name}@f64/stat/{key}"], data[f"{name}/stat/{key}"]
        print(f"{name}{tag} {key}: engine {np.array(stats[key])} ref32 {r32} ref64 {r64}")
        bound = np.maximum(tol * np.abs(r64) + 1e-6, 5 * np.abs(r32 - r64))
        if key == "train_acc":       # one prediction may flip on the fp32 noise floor
            bound = np.maximum(bound, 1.0 / meta["scenarios"][name]["n"] + 1e-9)
        assert np.all(np.abs(np.array(stats[key]) - r64) <= bound), (key, stats[key], r32, r64)
    n_chunks = len([k for k in stats if k.startswith("grad_norm_train_")])
    assert n_chunks == meta["scenarios"][name]["n"] // min(cfg.data.batch_size, cfg.hyp.sub_batch)
    for k in range(n_chunks):
        r64, r32 = data[f"{name}@f64/stat/grad_norm_train_{k}"], data[f"{name}/stat/grad_norm_train_{k}"]
        bound = np.maximum(max(tol, 1e-3) * np.abs(r64), 5 * np.abs(r32 - r64))
        assert np.all(np.abs(np.array(stats[f"grad_norm_train_{k}"]) - r64) <= bound), (k, stats[f"grad_norm_train_{k}"], r32, r64)
    ordered = [v.double() for v in model.state_dict().values()]
    err = rel_err(summarise(ordered)[1], data[f"{name}@f64/final_sample"])
    noise = rel_err(data[f"{name}/final_sample"], data[f"{name}@f64/final_sample"])
    print(f"{name}{tag}: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e})")
    assert err < max(10 * noise, 1e-5)
    rm_err = rel_err(model.state_dict()["stem.1.running_mean"].double().numpy(), data[f"{name}@f64/final_stem_running_mean"])
    rm_noise = rel_err(data[f"{name}/final_stem_running_mean"], data[f"{name}@f64/final_stem_running_mean"])
    print(f"{name}{tag}: stem running_mean engine-vs-ref64 {rm_err:.2e} (reference fp32-vs-f64 {rm_noise:.2e})")
    assert rm_err < max(10 * rm_noise, 2e-3)
    assert int(model.state_dict()["stem.1.num_batches_tracked"]) == int(data[f"{name}@f64/final_num_batches_tracked"][0])
    # evaluation of the final model on the first 64 images: the loss by the rule of the statistics, the accuracy within one prediction
    (l64, a64), (l32, a32) = data[f"{name}@f64/valid64"], data[f"{name}/valid64"]
    print(f"{name}{tag}: valid loss {stats['valid_loss'][-1]:.7f} acc {stats['valid_acc'][-1]:.4f}; ref32 {l32:.7f} {a32:.4f} ref64 {l64:.7f} {a64:.4f}")
    assert abs(stats["valid_loss"][-1] - l64) <= max(tol * abs(l64) + 1e-6, 5 * abs(l32 - l64))
    assert abs(stats["valid_acc"][-1] - a64) <= 1.0 / 64 + 1e-9
    assert all(p.grad is not None and p.grad.shape == p.shape for p in model.parameters())


@pytest.mark.parametrize("name,tol,group", [("dsb_plain", 2e-4, 3), ("dsb_gradreg", 3e-3, 2)])     # (the project's values for fb_plain / fb_gradreg)
def test_train_matches_reference_run_f32_downsample_b(dsb, name, tol, group, tmp_path):
    data, meta = dsb
    cfg, model, stats = _run(meta, name, [f"impl.engine.chunk_group={group}"], tmp_path)
    assert cfg.model.downsample == "B" and "layers.1.0.downsample.0.weight" in model.state_dict()
    _judge(data, meta, name, tol, cfg, model, stats)


def test_train_f16x2_opt_in_matches_reference_run_downsample_b(dsb, tmp_path):
    """``impl.engine.fd_arithmetic=f16x2`` together with 'B' shortcuts (test_train_f16x2_opt_in_matches_reference_run: the statistics and the
    final state by the same rules, the tolerance of fb_gradreg)."""
    data, meta = dsb
    name, tol = "dsb_gradreg", 3e-3
    cfg, model, stats = _run(meta, name, ["impl.engine.chunk_group=2", "impl.engine.fd_arithmetic=f16x2"], tmp_path)
    for key in STAT_KEYS:
        if f"{name}@f64/stat/{key}" not in data:
            continue
        r64, r32 = data[f"{name}@f64/stat/{key}"], data[f"{name}/stat/{key}"]
        print(f"{name} [f16x2] {key}: engine {np.array(stats[key])} ref32 {r32} ref64 {r64}")
        bound = np.maximum(tol * np.abs(r64) + 1e-6, 5 * np.abs(r32 - r64))
        if key == "train_acc":
            bound = np.maximum(bound, 1.0 / meta["scenarios"][name]["n"] + 1e-9)
        assert np.all(np.abs(np.array(stats[key]) - r64) <= bound), (key, stats[key], r32, r64)
    err = rel_err(summarise([v.double() for v in model.state_dict().values()])[1], data[f"{name}@f64/final_sample"])
    noise = rel_err(data[f"{name}/final_sample"], data[f"{name}@f64/final_sample"])
    print(f"{name} [f16x2]: final state engine-vs-ref64 {err:.2e} (reference fp32-vs-f64 {noise:.2e})")
    assert err < max(10 * noise, 1e-5)


def test_checkpoint_roundtrip_and_reference_layout_downsample_b(dsb, tmp_path):
    """The 5-list checkpoint of a 'B' run carries the reference's ResNet-20 key layout (``downsample.0`` / ``.1``), resumes to the
    uninterrupted run of the engine, and loads into a fresh container whose evaluation repeats the run's last validation pass."""
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import evaluate

    data, meta = dsb
    os.makedirs(tmp_path / "checkpoints", exist_ok=True)
    # (cosine-4000: the learning rate of a step does not depend on hyp.steps, so a run cut at two steps is the head of the three-step run)
    sched = "hyp.scheduler=cosine-4000"
    cfg, model, stats = _run(meta, "dsb_plain", [sched, "impl.checkpoint.name=ck.pth", "hyp.steps=2"], tmp_path)
    optim_state, model_state, sched_state, scaler_state, step = torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)
    assert step == 2 and scaler_state is None
    assert {k: [list(v.shape), str(v.dtype)] for k, v in model_state.items()} == meta["resnet20b_keys"]
    assert list(model_state) == list(meta["resnet20b_keys"])
    assert len(optim_state["state"]) == len(list(model.parameters()))
    assert all(tuple(optim_state["state"][i]["momentum_buffer"].shape) == tuple(p.shape) for i, p in enumerate(model.parameters()))
    # resume for the third step: must reproduce the uninterrupted 3-step run (the state travels through the file exactly, the engine is deterministic)
    cfg2, model2, stats2 = _run(meta, "dsb_plain", [sched, "impl.checkpoint.name=ck.pth", "hyp.steps=3"], tmp_path)
    cfg3, model3, stats3 = _run(meta, "dsb_plain", [sched, "hyp.steps=3"], tmp_path)
    assert len(stats3["train_loss"]) == 3 and stats3["train_loss"][:2] == stats["train_loss"]
    assert np.allclose(stats2["train_loss"][-1], stats3["train_loss"][-1], rtol=1e-6), (stats2["train_loss"], stats3["train_loss"])
    assert rel_err(summarise(list(model2.state_dict().values()))[1], summarise(list(model3.state_dict().values()))[1]) < 1e-6
    fresh = construct_model(cfg2.model, 3, 10)
    fresh.load_state_dict(torch.load(tmp_path / "checkpoints" / "ck.pth", weights_only=False)[1])
    sc = meta["scenarios"]["dsb_plain"]
    x, y = make_data(sc["n"], sc["pixels"])
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    ev = evaluate(fresh, (x[:64], y[:64]), None, setup, cfg2.impl, cfg2.hyp)
    assert np.allclose(ev["valid_loss"][-1], stats2["valid_loss"][-1], rtol=1e-5) and ev["valid_acc"][-1] == stats2["valid_acc"][-1]
