"""End-to-end GPU parity of the engine (forward + hand-scheduled backward through the whole ResNet) vs the CPU oracle and
the committed reference vectors.

Tolerances.  The per-chunk gradient of a freshly initialised ResNet-18 is an ill-conditioned (heavily cancelling) sum:
the reference's own fp32 CPU result differs from its float64 run by ~3e-3 relative L2 (tests/test_oracle_golden.py).
  f32 engine  vs float64 oracle : gradient 1e-2 (same class as the reference's fp32), loss 1e-5, BN statistics 1e-5
  bf16 engine: every activation / activation-gradient is stored with 2^-9 relative rounding, which flips ~0.4 % of the
    ReLU masks of near-zero pre-activations; at random init with random labels (the hardest case: the chunk gradient is
    the small residual of a cancelling sum) that alone moves the chunk gradient by ~30 % (the float64 oracle that merely
    *rounds at the same storage points* is 0.30 from the truth).  So bf16 is held to: loss 2e-3, classifier gradient
    5e-2, cosine > 0.9 and relative distance < 0.45 to the rounding-emulating oracle -- and to multi-step training
    statistics (test_gpu_training.py), where the noise averages out over chunks.
"""
import numpy as np
import pytest
import torch

from tests.helpers import make_data, oracle_device, oracle_state, rel_err, summarise, to_oracle

pytestmark = pytest.mark.gpu


def _build(depth=18, pixels=16, chunk=32, G=3, dtype=torch.float32, seed=0, fd_sets=0, stem="CIFAR", classes=10):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.models import construct_model

    cfg = compose([f"model=resnet{depth}", f"model.stem={stem}"])
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, classes)
    eng = Engine(model, pixels, chunk, G, compute_dtype=dtype, fd_sets=fd_sets)
    return cfg, model, eng, stem_patches


_TRUTH = {}


def _oracle_chunk_grads(model, x, y, chunk, depth=18, stem="CIFAR", classes=10, dtype=torch.float64, emulate_bf16=False):
    """[(gradient list on the HOST, loss, #correct) per chunk], params, buffers -- evaluated on the oracle's device (tests/helpers.py)."""
    from oracle import fb_oracle as orc

    q = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if emulate_bf16 else orc.identity
    spec = orc.Spec(depth, stem=stem, classes=classes)
    params, buffers = oracle_state(model, dtype)
    xo, yo = to_oracle(x, y, dtype=dtype)
    out = []
    for k in range(x.shape[0] // chunk):
        g, loss, correct = orc.chunk_gradient(spec, params, buffers, xo[k * chunk:(k + 1) * chunk], yo[k * chunk:(k + 1) * chunk], q)
        out.append(([t.cpu() for t in g], float(loss), float(correct)))
    return out, {k: v.cpu() for k, v in params.items()}, {k: v.cpu() for k, v in buffers.items()}


def _engine_grads_as_lists(eng, G):
    flat = eng.g[:G].cpu()
    return [[eng._unflatten(flat[g], name) for name in eng.plan.param_names] for g in range(G)]


@pytest.mark.parametrize("dtype,gtol,ltol", [(torch.float32, 1e-2, 1e-5), (torch.bfloat16, 0.45, 2e-3)])
def test_resnet18_chunk_gradients_vs_oracle(dtype, gtol, ltol):
    """f32 engine vs float64 oracle; bf16 engine vs the float64 oracle that rounds to bf16 at the engine's storage points
    (same rounding points, exact arithmetic in between), plus the distance of both to the un-rounded truth for the record."""
    pixels, chunk, G = 16, 32, 3
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, dtype)
    x, y = make_data(chunk * G, pixels)
    truth, _, _ = _oracle_chunk_grads(model, x, y, chunk)
    ref, params, buffers = _oracle_chunk_grads(model, x, y, chunk, emulate_bf16=dtype == torch.bfloat16)
    patches = stem_patches(x.cuda(), eng.plan.stem, dtype)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    torch.cuda.synchronize()
    got = _engine_grads_as_lists(eng, G)
    for g in range(G):
        assert abs(float(eng.loss[g]) - ref[g][1]) < ltol * max(1.0, abs(ref[g][1])), (g, float(eng.loss[g]), ref[g][1])
        if dtype == torch.float32:
            assert float(eng.correct[g]) == ref[g][2]
        a = torch.cat([t.reshape(-1).double() for t in got[g]])
        b = torch.cat([t.reshape(-1).double() for t in ref[g][0]])
        err = float((a - b).norm() / b.norm())
        t = torch.cat([r.reshape(-1).double() for r in truth[g][0]])
        print(f"[{dtype}] chunk {g}: engine-vs-oracle {err:.3e}; engine-vs-f64-truth {float((a - t).norm() / t.norm()):.3e}; "
              f"oracle-vs-truth {float((b - t).norm() / t.norm()):.3e}; loss {float(eng.loss[g]):.6f} vs {ref[g][1]:.6f} (truth {truth[g][1]:.6f})")
        assert err < gtol, (g, err)
        cos = float((a * t).sum() / (a.norm() * t.norm()))
        assert cos > (0.99999 if dtype == torch.float32 else 0.9), cos
        # the classifier gradient is well conditioned: tight in fp32, bf16 activation rounding (2^-9) in bf16
        assert rel_err(got[g][-2].numpy(), truth[g][0][-2].numpy()) < (1e-4 if dtype == torch.float32 else 5e-2)
    if dtype == torch.bfloat16:
        # the independent yardstick: torch's own bf16 autocast of the same model on the same chunks (plain torch -- neither libfbengine nor
        # oracle/; the reference's impl.mixed_precision path, training.py:76-83).  The engine may be no noisier than that: distance to the
        # float64 truth <= 1.15 x torch-bf16's, cosine no more than 0.01 below it, chunk by chunk.
        from tests.helpers import err_cos, flat64, torch_bf16_chunk_grads
        yard = torch_bf16_chunk_grads(model, x, y, chunk)
        for g in range(G):
            t = flat64(truth[g][0])
            e_eng, c_eng = err_cos(flat64(got[g]), t)
            e_tch, c_tch = err_cos(flat64(yard[g][0]), t)
            print(f"[bf16 yardstick] chunk {g}: engine {e_eng:.3f} / cos {c_eng:.4f}; torch autocast(bf16) {e_tch:.3f} / cos {c_tch:.4f}")
            assert e_eng <= 1.15 * e_tch, (g, e_eng, e_tch)
            assert c_eng >= c_tch - 0.01, (g, c_eng, c_tch)
            assert abs(float(eng.loss[g]) - yard[g][1]) < 2e-2 * max(1.0, abs(yard[g][1]))
    # batch statistics of the first and last BN layers (chunk 0) against torch
    L = eng.plan.stem
    mean0 = eng.mean_tab[0, 0, L.ch_off:L.ch_off + 64].cpu()
    xs = torch.nn.functional.conv2d(x[:chunk].double(), params["stem.0.weight"], None, 1, 1)
    assert rel_err(mean0.numpy(), xs.mean((0, 2, 3)).numpy()) < (1e-4 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("split", ["bf16x6", "f16x2"])
def test_f32_split_modes_regularised_mean_gradient_vs_oracle(split, monkeypatch):
    """Both arithmetic modes of the fp32 convolutions (three bf16 pieces / six MFMAs, two scaled fp16 pieces / three MFMAs)
    through the whole engine: raw chunk gradients and the finite-difference regularised MEAN gradient of three chunks (both passes in the
    same arithmetic, per-chunk scales) against the float64 oracle.  The regulariser's own truncation error (a few 1e-2 even in fp32)
    hides the 2^-22 operand rounding of f16x2; a raw chunk gradient of the freshly initialised net is a cancelling sum on the fp32 noise
    floor in either mode (the reference's own fp32 run: 3e-3 from its float64 run)."""
    from oracle import fb_oracle as orc
    monkeypatch.setenv("FB_F32_SPLIT", split)
    pixels, chunk, G = 16, 32, 3
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, torch.float32, fd_sets=1)
    assert eng.f32_split == split
    x, y = make_data(chunk * G, pixels)
    truth, _, _ = _oracle_chunk_grads(model, x, y, chunk)
    patches = stem_patches(x.cuda(), eng.plan.stem, torch.float32)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    got = _engine_grads_as_lists(eng, G)
    for g in range(G):
        a = torch.cat([t.reshape(-1).double() for t in got[g]])
        t = torch.cat([r.reshape(-1).double() for r in truth[g][0]])
        err = float((a - t).norm() / t.norm())
        print(f"[{split}] raw chunk {g}: engine-vs-f64 {err:.3e}")
        assert err < 1e-2 and float((a * t).sum() / (a.norm() * t.norm())) > 0.99999      # (the reference's own fp32 run: 3e-3)
    # regularised mean gradient (forward differences, block_strength 0.5, lr 0.1)
    spec = orc.Spec(18)
    params, buffers = oracle_state(model)
    xo, yo = to_oracle(x, y)
    mean = None
    for k in range(G):
        xk, yk = xo[k * chunk:(k + 1) * chunk], yo[k * chunk:(k + 1) * chunk]
        raw, _, _ = orc.chunk_gradient(spec, params, buffers, xk, yk)
        reg = orc.gradreg(spec, params, buffers, [g.clone() for g in raw], xk, yk, 0.1, 0.5, 1e-2, "forward-differences")
        flat = torch.cat([t.reshape(-1) for t in reg]).cpu()
        mean = flat / G if mean is None else mean + flat / G
    eng.full_gradient(patches, y.cuda(), 0.1, block_strength=0.5, eps=1e-2, implementation="forward-differences")
    torch.cuda.synchronize()
    names = eng.plan.param_names
    avg = torch.cat([eng._unflatten(eng.avg.cpu(), n).reshape(-1).double() for n in names])
    err = float((avg - mean).norm() / mean.norm())
    print(f"[{split}] regularised mean gradient of {G} chunks: engine-vs-f64 oracle {err:.3e}")
    assert err < 5e-2


def test_oracle_on_the_device_equals_the_oracle_on_the_host():
    """The float64 oracle of the GPU tests runs with its tensors on the device (tests/helpers.oracle_device: 60x faster than the host cores):
    same restatement, torch's GPU kernels instead of its CPU kernels -- raw and regularised chunk gradients agree with the host run to 1e-11."""
    from oracle import fb_oracle as orc
    if oracle_device().type != "cuda":
        pytest.skip("FB_ORACLE_DEVICE=cpu: the oracle already runs on the host")
    pixels, chunk = 16, 32
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, 1, torch.float32)
    x, y = make_data(chunk, pixels)
    spec = orc.Spec(18)
    out = {}
    for dev in (torch.device("cpu"), oracle_device()):
        params, buffers = oracle_state(model, device=dev)
        xd, yd = x.double().to(dev), y.to(dev)
        raw, loss, correct = orc.chunk_gradient(spec, params, buffers, xd, yd)
        reg = orc.gradreg(spec, params, buffers, [g.clone() for g in raw], xd, yd, 0.1, 0.5, 1e-2, "forward-differences")
        out[dev.type] = (torch.cat([t.reshape(-1).cpu() for t in raw]), torch.cat([t.reshape(-1).cpu() for t in reg]), float(loss), float(correct),
                         buffers["stem.1.running_mean"].cpu())
    a, b = out["cpu"], out["cuda"]
    assert float((a[0] - b[0]).norm() / a[0].norm()) < 1e-11 and float((a[1] - b[1]).norm() / a[1].norm()) < 1e-11
    assert abs(a[2] - b[2]) < 1e-12 and a[3] == b[3] and torch.allclose(a[4], b[4], rtol=1e-12, atol=1e-14)


def test_golden_reference_chunk_gradient_f32(golden):
    """Engine (f32) vs vectors of the REAL reference: fb_plain chunk 0 (128 images, 32x32) raw gradient sample + scalars."""
    data, meta = golden
    sc = meta["scenarios"]["fb_plain"]
    cfg, model, eng, stem_patches = _build(18, 32, 128, 2, torch.float32, seed=sc["model_seed"])
    x, y = make_data(sc["n"], 32)
    patches = stem_patches(x[:256].cuda(), eng.plan.stem, torch.float32)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y[:256].cuda(), 2, eng.g)
    got = _engine_grads_as_lists(eng, 2)
    for k in range(2):
        loss_ref, correct_ref, sq_ref = data[f"fb_plain@f64/chunk{k}_scalars"]
        assert abs(float(eng.loss[k]) - loss_ref) < 1e-5 * abs(loss_ref)
        assert float(eng.correct[k]) == correct_ref
        per, samp = summarise(got[k])
        e64 = rel_err(samp, data[f"fb_plain@f64/chunk{k}_raw_sample"])
        e32 = rel_err(samp, data[f"fb_plain/chunk{k}_raw_sample"])
        ref_noise = rel_err(data[f"fb_plain/chunk{k}_raw_sample"], data[f"fb_plain@f64/chunk{k}_raw_sample"])
        print(f"chunk {k}: engine-vs-ref64 {e64:.2e}, engine-vs-ref32 {e32:.2e}, ref32-vs-ref64 {ref_noise:.2e}")
        assert e64 < 1e-2 and e32 < 1.5e-2
        assert abs(float(sum(t.double().pow(2).sum() for t in got[k])) - sq_ref) < 5e-3 * sq_ref


def test_bottleneck_standard_stem_chunk_gradients_vs_oracle():
    """ResNet-50 (Bottleneck blocks, 7x7/s2 'standard' stem + MaxPool, stride-1 and stride-2 shortcuts) -- the block types of the
    ResNet-152 configuration -- at 64x64 input: f32 engine vs float64 oracle."""
    pixels, chunk, G = 64, 32, 2
    cfg, model, eng, stem_patches = _build(50, pixels, chunk, G, torch.float32, stem="standard")
    x, y = make_data(chunk * G, pixels)
    truth, params, buffers = _oracle_chunk_grads(model, x, y, chunk, depth=50, stem="standard")
    patches = stem_patches(x.cuda(), eng.plan.stem, torch.float32)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    torch.cuda.synchronize()
    got = _engine_grads_as_lists(eng, G)
    for g in range(G):
        assert abs(float(eng.loss[g]) - truth[g][1]) < 1e-5 * abs(truth[g][1])
        a = torch.cat([t.reshape(-1).double() for t in got[g]])
        t = torch.cat([r.reshape(-1).double() for r in truth[g][0]])
        err = float((a - t).norm() / t.norm())
        print(f"resnet50/standard chunk {g}: engine-vs-f64-truth {err:.3e}")
        assert err < 5e-2, err      # 53 conv layers: fp32 conditioning of the chunk gradient is ~5x that of ResNet-18
        assert rel_err(got[g][-2].numpy(), truth[g][0][-2].numpy()) < 1e-4


@pytest.mark.parametrize("c1g,bn3_gamma", [(None, None), ("1", None), (None, 0.25), ("1", 0.25)])
def test_bottleneck_standard_stem_bf16_chunk_gradients_vs_oracle(c1g, bn3_gamma, monkeypatch):
    """The bf16 Bottleneck path -- the arithmetic of bench.py's ResNet-152 lines (reference resnets.py:296-316 under impl.mixed_precision, training.py:76-83) --
    against the float64 oracle with the yardsticks of the ResNet-18 bf16 case: ResNet-50, 'standard' stem (7x7/s2 on pre-gathered patches, MaxPool with a
    remembered argmax), 64 px, three chunks of 32 in ONE group so that the identity blocks take their residual gradient through the ReLU bitmask inside the
    streaming 1x1 input gradients (asserted: the engine reports masked addends for them) -- with the shipped dispatch, and with FB_C1G=1 (every 1x1 forward
    call the 256 x 256 GEMM kernel can take goes there: the dispatch of the large groups of the ResNet-152 bench).  Held to: per chunk, distance to the float64 truth <= 1.15 x torch's own
    autocast(bf16) (and the rounding-emulating oracle's) and cosine >= torch's - 0.01, classifier gradient <= 1.15 x torch's; at the better-conditioned point (``bn3_gamma``)
    also loss 2e-3 from the rounding-emulating oracle, classifier gradient 5e-2, cosine > 0.88; the stem's batch statistics and the MaxPool output against torch."""
    from oracle import fb_oracle as orc
    from tests.helpers import err_cos, flat64, torch_bf16_chunk_grads
    if c1g is not None:
        monkeypatch.setenv("FB_C1G", c1g)
    pixels, chunk, G = 64, 32, 3
    dt = torch.bfloat16
    cfg, model, eng, stem_patches = _build(50, pixels, chunk, G, dt, stem="standard")
    if bn3_gamma is not None:
        # a better-conditioned point of the same net: the last BatchNorm of every block scaled down (towards the zero-init-residual start of reference
        # resnets.py:120-126), so that the residual branches perturb the identity path instead of doubling its variance sixteen times -- ReLU-mask flips of rounded
        # pre-activations then move the gradient by tens of per cent instead of replacing it, and an error of a few per cent in one kernel becomes visible end to end
        with torch.no_grad():
            for name, p_ in model.named_parameters():
                if name.endswith("bn3.weight"):
                    p_.fill_(bn3_gamma)
        eng.load_from_model(model)
    x, y = make_data(chunk * G, pixels)
    truth, _, _ = _oracle_chunk_grads(model, x, y, chunk, depth=50, stem="standard")
    ref, params, buffers = _oracle_chunk_grads(model, x, y, chunk, depth=50, stem="standard", emulate_bf16=True)
    # which blocks hand their residual gradient to the 1x1 input gradient as (d, ReLU bitmask of the block output): every identity block (conv1 with up to 256 output
    # channels: the streaming kernels; the two 512-channel blocks of the last stage: the implicit GEMM's epilogue, round 6)
    lazy = [b.shortcut is None and eng._masked_addend_ok(b.convs[0], G, 1) for b in eng.plan.blocks]
    assert lazy == [b.shortcut is None for b in eng.plan.blocks] and sum(lazy) == 12, lazy
    patches = stem_patches(x.cuda(), eng.plan.stem, dt)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    torch.cuda.synchronize()
    got = _engine_grads_as_lists(eng, G)
    yard = torch_bf16_chunk_grads(model, x, y, chunk)
    rows = []
    for g in range(G):
        t = flat64(truth[g][0])
        rows.append((err_cos(flat64(got[g]), t), err_cos(flat64(ref[g][0]), t), err_cos(flat64(yard[g][0]), t)))
        (e_eng, c_eng), (e_orc, c_orc), (e_tch, c_tch) = rows[-1]
        print(f"[resnet50 bf16, FB_C1G={c1g}, bn3 gamma {bn3_gamma}] chunk {g}: engine {e_eng:.3f} / cos {c_eng:.4f}; rounding-emulating oracle {e_orc:.3f} / {c_orc:.4f}; "
              f"torch autocast(bf16) {e_tch:.3f} / {c_tch:.4f}; loss {float(eng.loss[g]):.5f} vs {ref[g][1]:.5f} (truth {truth[g][1]:.5f}, torch {yard[g][1]:.5f}); "
              f"classifier gradient {rel_err(got[g][-2].numpy(), truth[g][0][-2].numpy()):.2e} (torch {rel_err(yard[g][0][-2].numpy(), truth[g][0][-2].numpy()):.2e})")
    # Measured (MI355X): at random initialisation a 32-image bf16 chunk gradient of this 53-layer net is mostly ReLU-mask noise in EVERY bf16 evaluation -- engine 1.25-1.29
    # from the float64 truth (cosine 0.17-0.22), the float64 oracle that only rounds at the engine's storage points 1.26-1.27 (0.19-0.21), torch's own autocast 1.24-1.28
    # (0.18-0.21); losses scatter by 0.2-1.3 % around the truth in all three, the classifier gradient is 0.21-0.23 off in engine and torch alike.  So the assertions are
    # the yardstick ones (no noisier than torch's bf16, chunk by chunk) plus sanity bounds; what pins the kernels is tests/test_gpu_bf16_structural.py (2 ulp per tensor).
    for g in range(G):
        (e_eng, c_eng), (e_orc, c_orc), (e_tch, c_tch) = rows[g]
        assert abs(float(eng.loss[g]) - truth[g][1]) < 3e-2 * abs(truth[g][1]), (g, float(eng.loss[g]), truth[g][1])
        assert abs(float(eng.loss[g]) - ref[g][1]) < 1e-2 * abs(ref[g][1]) and abs(float(eng.loss[g]) - yard[g][1]) < 2e-2 * abs(yard[g][1])
        assert e_eng <= 1.15 * e_tch and e_eng <= 1.15 * e_orc, (g, e_eng, e_tch, e_orc)
        assert c_eng >= c_tch - 0.01, (g, c_eng, c_tch)
        cls_eng, cls_tch = (rel_err(t[g][-2].numpy() if t is got else t[g][0][-2].numpy(), truth[g][0][-2].numpy()) for t in (got, yard))
        assert cls_eng <= 1.15 * cls_tch, (g, cls_eng, cls_tch)                       # classifier gradient: as close as torch's
        if bn3_gamma is not None:
            # the better-conditioned point (measured: engine 0.415-0.428 / cosine 0.909-0.914, the rounding-emulating oracle 0.416-0.426 / 0.909-0.913, torch autocast
            # 0.416-0.430 / 0.907-0.914; loss 5e-4 from the emulating oracle; classifier gradient 2.4e-2 - 3.0e-2, torch 2.5e-2 - 3.2e-2): the ResNet-18 bounds hold
            assert abs(float(eng.loss[g]) - ref[g][1]) < 2e-3 * abs(ref[g][1]) and cls_eng < 5e-2 and c_eng > 0.88 and e_eng < 0.5, (g, e_eng, c_eng, cls_eng)
    # the stem: batch statistics of chunk 0 and the MaxPool output of the whole group against torch on the oracle's (bf16-rounded) tensors
    L = eng.plan.stem
    q = lambda t: t.to(torch.bfloat16).to(t.dtype)          # noqa: E731
    w0 = q(params["stem.0.weight"].double())
    raw = torch.nn.functional.conv2d(q(x[:chunk].double()), w0.cpu(), None, 2, 3)
    assert rel_err(eng.mean_tab[0, 0, L.ch_off:L.ch_off + 64].cpu().numpy(), raw.mean((0, 2, 3)).numpy()) < 1e-3
    assert rel_err(eng.var_tab[0, 0, L.ch_off:L.ch_off + 64].cpu().numpy(), raw.var((0, 2, 3), unbiased=False).numpy()) < 1e-3
    pooled = torch.nn.functional.max_pool2d(eng.stem_out.float().permute(0, 3, 1, 2), 3, 2, 1)
    assert torch.equal(pooled.permute(0, 2, 3, 1).contiguous(), eng.stem_pooled.float())
    # the remembered argmax addresses a maximum of its window (ties: any maximal element gives the same gradient VALUE only if it is the first -- fb_maxpool3s2_bwd_idx
    # against the recomputing form is a bit-identity test in test_gpu_ops.py; here: the byte of every pooled element points at an element equal to the pooled value)
    if eng.stem_pool_idx is not None:
        so = eng.stem_out.float()
        n_, hp = so.shape[0], eng.stem_pooled.shape[1]
        idx = eng.stem_pool_idx.long()
        dy_, dx_ = idx // 3, idx % 3
        oy = torch.arange(hp, device=so.device)[None, :, None, None] * 2 - 1 + dy_
        ox = torch.arange(hp, device=so.device)[None, None, :, None] * 2 - 1 + dx_
        assert int(oy.min()) >= 0 and int(ox.min()) >= 0 and int(oy.max()) < so.shape[1] and int(ox.max()) < so.shape[2]
        ni = torch.arange(n_, device=so.device)[:, None, None, None].expand_as(idx)
        ci = torch.arange(64, device=so.device)[None, None, None, :].expand_as(idx)
        assert torch.equal(so[ni, oy, ox, ci], eng.stem_pooled.float())


@pytest.mark.parametrize("dtype,wsets", [(torch.bfloat16, 1), (torch.float32, 1), (torch.float32, 2)])
def test_on_block_done_path_gives_the_bits_of_the_replayed_path_on_a_bottleneck_plan(dtype, wsets):
    """A rank's LAST chunk group of a multi-GPU step is issued launch by launch (``group_gradient(on_block_done=...)`` bypasses the command lists: the callback that
    starts the late bucket's exchange sits inside the backward pass, reference training/utils.py:31-41 for resnets.py:271-316) -- every other group is a replayed
    list.  Both must give the same bits on a Bottleneck plan (masked addends of the identity blocks, remembered MaxPool argmax, per-chunk weight sets of the
    finite-difference pass), and the callback fires once per block, last block first, the late block among them."""
    pixels, chunk, G = 64, 32, 3
    cfg, model, eng, stem_patches = _build(50, pixels, chunk, G, dtype, stem="standard", fd_sets=1 if wsets > 1 else 0)
    x, y = make_data(chunk * G, pixels)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
    theta, gout, pidx = eng.theta, eng.g, 0
    if wsets > 1:                                     # the finite-difference pass: one perturbed parameter set per chunk
        eng.theta_k.copy_(eng.theta[None, :] * (1 + 1e-3 * torch.arange(1, G + 1, device="cuda", dtype=torch.float32)[:, None]))
        theta, gout, pidx = eng.theta_k, eng.g_fd[0], 1
    prep = (lambda: eng.prep_weights(theta, G, per_chunk=True)) if wsets > 1 else (lambda: eng.prep_weights(theta, 1))
    out = []
    for rep in range(2):                              # (recorded, then replayed)
        prep()
        eng.group_gradient(patches, yd, G, gout, wsets, theta, pidx)
        torch.cuda.synchronize()
        out.append((gout[:G].clone(), eng.loss[:G].clone(), eng.mean_tab[pidx].clone()))
    assert eng.replays > 0
    seen = []
    prep()
    eng.group_gradient(patches, yd, G, gout, wsets, theta, pidx, on_block_done=seen.append)
    torch.cuda.synchronize()
    assert seen == list(range(len(eng.plan.blocks) - 1, -1, -1)) and eng.plan.late_block == 13 and eng.plan.late_block in seen
    for ref in out:
        assert torch.equal(ref[0], gout[:G]) and torch.equal(ref[1], eng.loss[:G]) and torch.equal(ref[2], eng.mean_tab[pidx])
    assert bool(torch.isfinite(gout[:G]).all()) and float(gout[:G].abs().max()) > 0


def test_experimental_switches_need_fb_experimental(monkeypatch):
    """The switches that turn ON a kernel form which lost its same-box A/B (fused BatchNorm-backward statistics; in the library: FB_C1G=2, FB_H4_WIDE, ...) act
    only together with FB_EXPERIMENTAL=1 -- without it the engine runs the default dispatch whatever else the environment says (DESIGN.md section 4 is then the
    whole truth)."""
    monkeypatch.setenv("FB_FUSED_BWD_STAT", "1")
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine
    from fullbatchtraining_amd.models import construct_model
    model = construct_model(compose([]).model, 3, 10)

    def build():
        return Engine(model, 32, 128, 2, compute_dtype=torch.bfloat16, nominal_group=98)

    monkeypatch.setenv("FB_EXPERIMENTAL", "0")
    eng = build()
    assert not eng.fuse_bwd_stat
    monkeypatch.setenv("FB_EXPERIMENTAL", "1")
    eng = build()
    assert eng.fuse_bwd_stat


def test_resnet152_at_224_directional_derivative():
    """BASELINE config 5 at its real shape (ResNet-152, 'standard' stem, 224x224 inputs, one chunk of 128 images, fp32 storage with the
    bf16x6 split -- the arithmetic of plain fp32 training; the regulariser's f16x2 arithmetic at this shape is covered by
    test_resnet152_at_224_regulariser_f16x2 below): too large for the CPU oracle inside a test, so a size-independent property ties the backward kernels to the
    forward ones -- the change of the chunk loss between theta + c g and theta - c g equals <g, theta+ - theta-> (the ACTUAL fp32
    difference of the two parameter vectors: |g| is ~1500 at initialisation, so a step that moves the loss by 1e-3 changes most
    weights by less than their fp32 spacing and the rounded step has to be accounted for).  Measured 1.0003; 0.989 / 1.025 at a
    4x larger / smaller step (curvature / fp32 resolution of the loss)."""
    pixels, chunk, G = 224, 128, 1
    cfg, model, eng, stem_patches = _build(152, pixels, chunk, G, torch.float32, stem="standard")
    x, y = make_data(chunk, pixels)
    patches = stem_patches(x.cuda(), eng.plan.stem, torch.float32)
    yd = y.cuda()

    def loss_and_grad():
        eng.prep_weights(eng.theta, 1)
        eng.group_gradient(patches, yd, G, eng.g)
        torch.cuda.synchronize()
        return float(eng.loss[0]), eng.g[0].clone()

    loss0, g = loss_and_grad()
    gn = float(g.double().norm())
    assert np.isfinite(loss0) and np.isfinite(gn) and gn > 0
    theta0 = eng.theta.clone()
    c = 5e-4 * max(1.0, abs(loss0)) / gn ** 2
    tp, tm = theta0 + c * g, theta0 - c * g
    predicted = float((g.double() * (tp.double() - tm.double())).sum())
    eng.theta.copy_(tp)
    lp, _ = loss_and_grad()
    eng.theta.copy_(tm)
    lm, _ = loss_and_grad()
    eng.theta.copy_(theta0)
    print(f"resnet152@224: loss {loss0:.5f}, |g| {gn:.2f}, (L+ - L-) / <g, theta+ - theta-> = {(lp - lm) / predicted:.4f}")
    assert abs((lp - lm) / predicted - 1.0) < 2e-2, (lp, lm, predicted)
    # determinism at this size: a second evaluation reproduces loss and gradient bit for bit
    loss1, g1 = loss_and_grad()
    assert loss1 == loss0 and torch.equal(g1, g)


def test_resnet152_at_224_regulariser_f16x2(monkeypatch):
    """BASELINE config 5 WITH the regulariser, in the arithmetic it runs by default (f16x2: two scaled fp16 pieces per operand, one
    power-of-two scale per chunk and tensor).  ResNet-152 needs ~310 scale slots per forward + backward; round 2 handed them out from a
    ring of 256, so the weight gradients of the first layers read another tensor's scale -> fp16 overflow -> NaN loss after one update,
    and nothing tested f16x2 at this depth.  (i) two regularised steps stay finite, (ii) the directional-derivative property of the raw
    chunk gradient holds on the f16x2 path, (iii) raw and regularised chunk gradients stay inside the measured fp32 noise floor of
    this (ill-conditioned) shape -- see the comment at the assertions and profiles/r3_fd_conditioning.md."""
    from fullbatchtraining_amd.engine import Engine

    pixels, chunk, G = 224, 128, 1
    x, y = make_data(chunk, pixels)
    yd = y.cuda()
    results = {}
    for split in ("f16x2", "bf16x6"):
        monkeypatch.setenv("FB_F32_SPLIT", split)
        cfg, model, eng, stem_patches = _build(152, pixels, chunk, G, torch.float32, stem="standard", fd_sets=1)
        assert eng.f32_split == split
        patches = stem_patches(x.cuda(), eng.plan.stem, torch.float32)
        loss, _, sq = eng.full_gradient(patches, yd, 0.1, block_strength=0.5, eps=1e-2, implementation="forward-differences")
        torch.cuda.synchronize()
        results[split] = (float(loss[0]), eng.avg.clone().cpu().double(), float(sq[0]), eng.g[0].clone().cpu().double())
        assert np.isfinite(results[split][0]) and bool(torch.isfinite(eng.avg).all()) and bool(torch.isfinite(eng.g_fd[0][0]).all())
        if split == "f16x2":
            print(f"f16x2 scale slots: {eng.amax_handouts} hand-outs in one regularised evaluation, {len(eng.amax_slots)} distinct buffers")
            assert eng.amax_handouts > 2 * 256           # (two passes) the shape that overran the old ring of 256 within ONE pass
            # (ii) directional derivative of the raw chunk gradient on this arithmetic
            def loss_and_grad():
                eng.prep_weights(eng.theta, 1)
                eng.group_gradient(patches, yd, G, eng.g)
                torch.cuda.synchronize()
                return float(eng.loss[0]), eng.g[0].clone()

            loss0, g = loss_and_grad()
            gn = float(g.double().norm())
            theta0 = eng.theta.clone()
            c = 5e-4 * max(1.0, abs(loss0)) / gn ** 2
            tp, tm = theta0 + c * g, theta0 - c * g
            predicted = float((g.double() * (tp.double() - tm.double())).sum())
            eng.theta.copy_(tp)
            lp, _ = loss_and_grad()
            eng.theta.copy_(tm)
            lm, _ = loss_and_grad()
            eng.theta.copy_(theta0)
            print(f"resnet152@224 f16x2: loss {loss0:.5f}, |g| {gn:.2f}, (L+ - L-) / <g, theta+ - theta-> = {(lp - lm) / predicted:.4f}")
            assert abs((lp - lm) / predicted - 1.0) < 2e-2, (lp, lm, predicted)
            # (i) two regularised steps: update with the clipped regularised gradient, evaluate again
            eng.full_gradient(patches, yd, 0.1, block_strength=0.5, eps=1e-2, implementation="forward-differences")
            eng.grad_and_param_sqnorm()
            eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True, grad_clip=0.25)
            loss2, _, sq2 = eng.full_gradient(patches, yd, 0.1, block_strength=0.5, eps=1e-2, implementation="forward-differences")
            torch.cuda.synchronize()
            print(f"resnet152@224 f16x2 + regulariser: loss {results[split][0]:.5f} -> {float(loss2[0]):.5f}, |g_k|^2 {results[split][2]:.4e} -> {float(sq2[0]):.4e}")
            assert np.isfinite(float(loss2[0])) and np.isfinite(float(sq2[0])) and bool(torch.isfinite(eng.avg).all())
        del eng, patches
        torch.cuda.empty_cache()
    (l16, a16, s16, _), (l6, a6, s6, _) = results["f16x2"], results["bf16x6"]
    err = float((a16 - a6).norm() / a6.norm())
    print(f"resnet152@224 regularised chunk gradient, f16x2 vs bf16x6: {err:.3e}; loss {l16:.6f} vs {l6:.6f}; |g_k|^2 {s16:.5e} vs {s6:.5e}")
    assert abs(l16 - l6) < 1e-4 * abs(l6)
    assert abs(s16 - s6) < 1e-2 * s6
    # How close can two 32-bit evaluations be here?  profiles/r3_fd_conditioning.md: at this shape the finite-difference term is 2648 x the
    # gradient (extreme curvature at random init), the exact-f32 MFMA chain -- another legitimate fp32 evaluation -- is 1.0e-1 from bf16x6 on the
    # RAW chunk gradient and 0.96 on the regularised one, and re-ordering fp32 additions alone moves the latter by 4e-2.  f16x2 must stay
    # inside that fp32 floor (measured 7.2e-2 raw, 0.916 regularised); 5e-2 on the regularised gradient is out of reach for ANY fp32 arithmetic
    raw16, raw6 = results["f16x2"][3], results["bf16x6"][3]
    raw_err = float((raw16 - raw6).norm() / raw6.norm())
    print(f"resnet152@224 raw chunk gradient, f16x2 vs bf16x6: {raw_err:.3e} (exact-f32 MFMA vs bf16x6: 1.0e-1)")
    assert raw_err < 1.0e-1, raw_err
    assert err < 0.96, err
    cos = float((a16 * a6).sum() / (a16.norm() * a6.norm()))
    assert cos > 0.5, cos


def test_f16x2_scale_slots_are_owned_by_their_buffer(monkeypatch):
    """Host-side contract of the fp16x2 scale slots: a buffer keeps ONE slot for the life of the engine, distinct live buffers never
    share one (however many there are), and the pool invalidates the cached magnitudes of a buffer it hands out again."""
    monkeypatch.setenv("FB_F32_SPLIT", "f16x2")
    cfg, model, eng, stem_patches = _build(18, 16, 32, 2, torch.float32, fd_sets=1)
    bufs = [torch.empty(64, device="cuda") for _ in range(600)]          # > 2 allocation blocks of 256
    slots = [eng._amax_slot(t, 64) for t in bufs]
    assert len(set(slots)) == len(slots)
    assert [eng._amax_slot(t, 64) for t in bufs] == slots
    t = eng.pool.get((4, 4))
    eng._amax_slot(t, 16)
    assert t.data_ptr() in eng.amax_map
    eng.pool.put(t)
    t2 = eng.pool.get((4, 4))
    assert t2.data_ptr() == t.data_ptr() and t.data_ptr() not in eng.amax_map


@pytest.mark.parametrize("dtype,fd", [(torch.bfloat16, 0), (torch.float32, 1)])
def test_replayed_command_lists_equal_interpreted_launches(dtype, fd, monkeypatch):
    """The native launch executor (csrc/cmdlist.cpp) replays exactly the launches the interpreter issued when the list was recorded: three
    full-gradient evaluations + updates with replay on (the first records, the next two replay) give bit-identical parameters, running
    statistics, losses and per-chunk norms to the same three steps with every launch going through ctypes (FB_REPLAY=0) -- plain bf16 and
    the fp32 finite-difference passes (per-chunk weight sets, fp16x2 scale slots), two chunk groups per step, ragged last group."""
    pixels, chunk, G, n_chunks = 16, 32, 3, 5
    x, y = make_data(chunk * n_chunks, pixels)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("FB_REPLAY", mode)
        cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, dtype, fd_sets=fd)
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
            per_step = 2 * (1 + fd) + 1 + 2 * fd          # group passes + weight preparations (shared set + per-chunk sets of each group)
            assert eng.replays == 2 * per_step, (eng.replays, per_step)
            assert len(eng.cmdlists) == per_step
            assert sum(len(c) for c in eng.cmdlists.values()) > 400
        out[mode] = (eng.theta.clone(), eng.mom.clone(), eng.running_mean.clone(), eng.running_var.clone(), trace, eng.num_batches_tracked)
    a, b = out["0"], out["1"]
    for i in range(4):
        assert torch.equal(a[i], b[i]), i
    for ta, tb in zip(a[4], b[4]):
        for u, v in zip(ta, tb):
            assert torch.equal(u, v)
    assert a[5] == b[5]


@pytest.mark.filterwarnings("ignore:fullbatchtraining_amd.Engine")
def test_command_list_cache_is_bounded_and_stops_recording_when_it_thrashes(monkeypatch):
    """More (group, pass) keys than the cache holds, visited cyclically -- the shape of ResNet-152 with the regulariser on one GPU (~196 keys), or
    of a feed that re-allocates its buffers every step: the least recently used list is dropped, its library events are REUSED by the next
    recording (the process-wide event table stops growing), after one cache worth of evictions the engine stops recording (misses go through
    the interpreter, hits still replay), and the arithmetic is bit-identical to the interpreted launches throughout."""
    from fullbatchtraining_amd import lib
    pixels, chunk, G, n_chunks = 16, 32, 1, 7
    x, y = make_data(chunk * n_chunks, pixels)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("FB_REPLAY", mode)
        monkeypatch.setenv("FB_MAX_CMDLISTS", "4")
        cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, torch.bfloat16)
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.bfloat16), y.cuda()
        counts = [lib.event_count()]
        for step in range(6):
            eng.full_gradient(patches, yd, 0.1)
            eng.grad_and_param_sqnorm()
            eng.sgd_step(0.1, 5e-4, 0.9, 0.0, True, grad_clip=0.25)
            counts.append(lib.event_count())
        torch.cuda.synchronize()
        if mode == "1":
            # recording was switched off at least once (misses ran through the interpreter, one warning), and hits pay the eviction count
            # back so that it can come on again (a transient thrash must not disable recording for the rest of the process)
            assert len(eng.cmdlists) <= 4 and eng.unrecorded_runs > 0 and eng._warned_record_off
            # 8 keys cycle through 4 slots: recordings reuse the ids of dropped lists; once recording has stopped the interpreted launches
            # draw from the engine's ring of 1024 eager events, and the table stops growing altogether
            from fullbatchtraining_amd.engine import _Events
            per_list = max(len(cl.events) for cl in eng.cmdlists.values())
            assert per_list > 10
            assert counts[1] - counts[0] <= 6 * per_list, (counts, per_list)        # step 1 records 8 lists into 4 slots: at most 5 of them on fresh events
            assert counts[-1] <= counts[1] + _Events.RING and len(eng.events.ring) <= _Events.RING, counts
        out[mode] = (eng.theta.clone(), eng.running_mean.clone())
        if mode == "1":
            # steady state on a working set that fits (2 chunks: prep + 2 group keys): every launch sequence is replayed again
            for step in range(6):
                eng.full_gradient(patches[: 2 * chunk], yd[: 2 * chunk], 0.1)
            torch.cuda.synchronize()
            before = eng.replays
            eng.full_gradient(patches[: 2 * chunk], yd[: 2 * chunk], 0.1)
            assert eng.record_new and eng.replays == before + 3, (eng.record_new, eng.replays - before)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])


def test_replayed_list_refuses_a_missing_stream(monkeypatch):
    """A list recorded with the weight-gradient stream holds stream INDICES; the stream pair is part of the cache key (dropping the stream
    records a new list instead of replaying the old one into the default stream), and CommandList.replay itself raises on a None stream it needs."""
    from fullbatchtraining_amd.lib import EngineError
    pixels, chunk, G = 16, 32, 2
    x, y = make_data(chunk * G, pixels)
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, torch.bfloat16)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.bfloat16), y.cuda()
    eng.full_gradient(patches, yd, 0.1)
    two = eng.avg.clone()
    n_lists = len(eng.cmdlists)
    group_list = next(cl for key, cl in eng.cmdlists.items() if key[0] == "group")
    with pytest.raises(EngineError, match="stream index that is None"):
        group_list.replay([torch.cuda.current_stream(), None])
    saved, eng.wstream = eng.wstream, None
    eng.running_mean.zero_(), eng.running_var.fill_(1.0)
    eng.full_gradient(patches, yd, 0.1)
    torch.cuda.synchronize()
    assert len(eng.cmdlists) == 2 * n_lists and torch.equal(eng.avg, two)
    eng.wstream = saved


@pytest.mark.parametrize("case", ["r18-bf16", "r18-fd-f16x2", "r18-fd-bf16x6", "r50-bf16", "r152-bf16"])
def test_two_stream_schedule_is_bit_identical_to_one_stream(case, monkeypatch):
    """The schedule bench.py runs (weight gradients and the running-mean pass on a second stream, recorded launches replayed natively) gives bit
    for bit what the same launches give in one stream, every time.  ``r18-bf16``: ResNet-18 at the benchmark's real shape (32 x 32, chunks of
    128), 8 chunks in groups of 3 / 3 / 2, three evaluations + updates, ten repetitions against the one-stream trace -- the regression test of
    the store-data hazard of the resident-filter convolution (csrc/common.h store_b128_guard): before the guard half of such runs carried a
    corrupted bf16 (~1e38, then Inf / NaN) in the 32 x 32 stage's input gradients, and only while two streams kept the CUs busy.  The other
    cases put the remaining kernel families under the same two-stream load: the fp32 finite-difference passes in both split modes (per-chunk
    weight sets, fp16x2 scale slots) and Bottleneck models with the standard stem (streaming 1x1 kernels, 1x1 / all-taps weight gradients), ResNet-152 at 224 px among them."""
    fd = case.startswith("r18-fd")
    if case == "r50-bf16":
        depth, stem, pixels, chunk, G, n_chunks, dtype, reps = 50, "standard", 64, 32, 2, 5, torch.bfloat16, 6
    elif case == "r152-bf16":            # BASELINE config 5's shape: 224 px, chunks of 128 (56 / 28 / 14 / 7 maps, MaxPool, 1x1 streaming kernels)
        depth, stem, pixels, chunk, G, n_chunks, dtype, reps = 152, "standard", 224, 128, 2, 3, torch.bfloat16, 3
    elif fd:
        depth, stem, pixels, chunk, G, n_chunks, dtype, reps = 18, "CIFAR", 32, 128, 2, 3, torch.float32, 6
        monkeypatch.setenv("FB_F32_SPLIT", case.split("-")[-1])
    else:
        depth, stem, pixels, chunk, G, n_chunks, dtype, reps = 18, "CIFAR", 32, 128, 3, 8, torch.bfloat16, 10
    x, y = make_data(chunk * n_chunks, pixels)

    def run():
        cfg, model, eng, stem_patches = _build(depth, pixels, chunk, G, dtype, fd_sets=1 if fd else 0, stem=stem)
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
    monkeypatch.setenv("FB_WGRAD_STREAM", "1")       # (unset, a wide Bottleneck net would time both schedules and keep the faster one: engine._autotune_streams)
    monkeypatch.delenv("FB_ACC_OVERLAP")
    for rep in range(reps):
        eng, got = run()
        assert eng.wstream is not None and eng.use_replay and eng.replays > 0
        for k, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (case, rep, k, float((a - b).abs().max()))


def test_stream_schedule_is_timed_once_for_wide_bottleneck_nets(monkeypatch):
    """engine._autotune_streams: with FB_WGRAD_STREAM unset, an engine whose plan has 1x1 layers with K >= 512 (ResNet-50) times one chunk group with and
    without the weight-gradient stream at its first full_gradient call and keeps the faster schedule (two streams unless one is 0.5 % faster); the timing
    passes leave nothing behind -- losses, squared norms, mean gradient and running statistics equal those of an engine pinned to either schedule bit for
    bit; a BasicBlock net (ResNet-18) never times anything; FB_WGRAD_STREAM=0 / 1 pins."""
    monkeypatch.delenv("FB_WGRAD_STREAM", raising=False)
    x, y = make_data(32 * 5, 64)

    def run(depth):
        cfg, model, eng, stem_patches = _build(depth, 64, 32, 2, torch.bfloat16, stem="standard")
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.bfloat16), y.cuda()
        auto = eng.stream_autotune
        loss, correct, sq = eng.full_gradient(patches, yd, 0.1)
        loss2, _, sq2 = eng.full_gradient(patches, yd, 0.1)              # (the second call does not time again)
        torch.cuda.synchronize()
        return eng, auto, [loss.clone(), correct.clone(), sq.clone(), eng.avg.clone(), eng.running_mean.clone(), eng.running_var.clone(), loss2.clone(), sq2.clone()]

    eng, auto, got = run(50)
    assert auto and not eng.stream_autotune and set(eng.stream_times) == {"one", "two"} and all(t > 0 for t in eng.stream_times.values())
    assert (eng.wstream is None) == (eng.stream_times["one"] < 0.995 * eng.stream_times["two"])
    assert int(eng.num_batches_tracked) == 10                             # two calls x five chunks: the timing passes are not counted
    for pin in ("0", "1"):
        monkeypatch.setenv("FB_WGRAD_STREAM", pin)
        eng_p, auto_p, ref = run(50)
        assert not auto_p and eng_p.stream_times is None and (eng_p.wstream is None) == (pin == "0")
        for a, b in zip(ref, got):
            assert torch.equal(a, b)
    monkeypatch.delenv("FB_WGRAD_STREAM")
    eng18, auto18, _ = run(18)
    assert not auto18 and eng18.stream_times is None and eng18.wstream is not None
    # choose_schedule: the same choice made by the caller ahead of its first (timed) step -- full_gradient then has nothing left to time and gives the same bits
    cfg, model, eng_c, stem_patches = _build(50, 64, 32, 2, torch.bfloat16, stem="standard")
    patches, yd = stem_patches(x.cuda(), eng_c.plan.stem, torch.bfloat16), y.cuda()
    eng_c.choose_schedule(patches, yd, 5)
    assert not eng_c.stream_autotune and set(eng_c.stream_times) == {"one", "two"}
    chosen = dict(eng_c.stream_times)
    loss, correct, sq = eng_c.full_gradient(patches, yd, 0.1)
    torch.cuda.synchronize()
    assert eng_c.stream_times == chosen and torch.equal(loss, got[0]) and torch.equal(sq, got[2]) and torch.equal(eng_c.avg, got[3])


def test_chunk_group_beyond_2g_byte_tensors_equals_smaller_groups():
    """bf16 chunk groups whose activation tensors exceed 2^31 bytes (more than 127 chunks of 128 images at 32 x 32 x 64 channels): every kernel bases
    its buffer descriptors at its own tile / K slice, so the 32-bit offsets inside stay small.  130 chunks in ONE group (the 64-channel tensors are
    2.18 GB each) give the losses and BatchNorm statistics of the same chunks in two groups of 65 bit for bit (the forward pass is the same
    arithmetic) and the same gradients up to the summation order of the BatchNorm-backward reduction, whose partial rows cover 128-1024 pixels
    depending on the launch's pixel count (fb_bn_bwd_reduce_rows; a different fp32 sum order moves a few bf16 roundings of dx): EVERY chunk's
    squared gradient norm to 1e-3 (measured 2e-4), the mean gradient to 2e-3 relative L2 (measured 5.7e-4; the bf16 path itself is 6e-3 from fp32).
    A wrong address anywhere in a 2 GB tensor would be garbage or a chunk off by per cent.  Same K-slice counts: nominal_group = 130 for both."""
    import gc

    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.models import construct_model

    pixels, chunk, n_chunks = 32, 128, 130
    x, y = make_data(chunk * 4, pixels)
    x, y = x.repeat(n_chunks // 4 + 1, 1, 1, 1)[:chunk * n_chunks], y.repeat(n_chunks // 4 + 1)[:chunk * n_chunks]
    x = x + 0.01 * torch.arange(chunk * n_chunks).view(-1, 1, 1, 1) / (chunk * n_chunks)       # (no two chunks alike)
    cfg = compose(["model=resnet18", "model.stem=CIFAR"])
    out = {}
    for G in (65, 130):
        torch.manual_seed(0)
        model = construct_model(cfg.model, 3, 10)
        eng = Engine(model, pixels, chunk, G, compute_dtype=torch.bfloat16, nominal_group=130)
        if G == 130:
            assert max(t.numel() * t.element_size() for t in (eng.stem_out, eng.plan.blocks[0].out)) > (1 << 31)
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.bfloat16), y.cuda()
        loss, correct, sq = eng.full_gradient(patches, yd, 0.1)
        torch.cuda.synchronize()
        out[G] = (loss.cpu(), correct.cpu(), sq.cpu(), eng.avg.cpu(), eng.running_mean.cpu(), eng.running_var.cpu())
        del eng, patches, model
        gc.collect(), torch.cuda.empty_cache()
    a, b = out[65], out[130]
    assert bool(torch.isfinite(b[3]).all())
    for k in (0, 1, 4, 5):
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    assert float(((a[2] - b[2]).abs() / a[2]).max()) < 1e-3
    err = float((a[3] - b[3]).norm() / a[3].norm())
    print(f"mean gradient of 130 chunks, one group vs two: rel L2 {err:.2e}")
    assert err < 2e-3


@pytest.mark.parametrize("depth,pixels,n_chunks,split", [(18, 32, 130, "bf16x6"), (18, 32, 130, "f16x2"), (50, 224, 8, "bf16x6")])
def test_f32_chunk_group_beyond_2g_byte_tensors_equals_smaller_groups(depth, pixels, n_chunks, split, monkeypatch):
    """fp32 storage with chunk groups whose activation tensors exceed 2^31 bytes (round 6 lifted the rule that held fp32 groups below that: the implicit GEMM and
    the persistent halo kernel base their descriptors at their own tile, the weight-gradient and BatchNorm kernels use 64-bit pointers): ONE group against two groups
    of half the size -- ResNet-18 @32 with 130 chunks (4.4 GB tensors) in both fp32 arithmetics, ResNet-50 / 'standard' stem @224 with 8 chunks of 128 (3.06 GiB; the
    layer shapes of BASELINE config 5) -- plain and with the regulariser (per-chunk weight sets in the second pass).  The forward pass is the same arithmetic: losses
    bit for bit; a chunk's gradient differs by the summation order of the BatchNorm-backward partial rows only (squared norms to 1e-5, measured 1e-7; mean gradient
    to 1e-4, measured 8e-7); the regularised mean gradient amplifies those last bits by 1 / eps_n (measured 9e-3 ... 4e-2 -- profiles/r3_fd_conditioning.md -- held
    to finite, cosine 0.99).  A wrong address anywhere in a 3 GB tensor would be garbage."""
    import gc

    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.models import construct_model

    monkeypatch.setenv("FB_F32_SPLIT", split)
    chunk = 128
    x, y = make_data(chunk * 4, pixels)
    reps = n_chunks // 4 + 1
    x, y = x.repeat(reps, 1, 1, 1)[:chunk * n_chunks], y.repeat(reps)[:chunk * n_chunks]
    x = x + 0.01 * torch.arange(chunk * n_chunks).view(-1, 1, 1, 1) / (chunk * n_chunks)       # (no two chunks alike)
    cfg = compose([f"model=resnet{depth}", f"model.stem={'CIFAR' if depth == 18 else 'standard'}"])
    out = {}
    for G in (n_chunks // 2, n_chunks):
        torch.manual_seed(0)
        model = construct_model(cfg.model, 3, 10)
        eng = Engine(model, pixels, chunk, G, compute_dtype=torch.float32, nominal_group=n_chunks, fd_sets=1)
        assert eng.f32_split == split
        if G == n_chunks:
            assert max(t.numel() * t.element_size() for t in (eng.stem_out, eng.plan.blocks[0].out)) > (1 << 31)
        patches, yd = stem_patches(x.cuda(), eng.plan.stem, torch.float32), y.cuda()
        res = []
        for bs in (0.0, 0.5):
            loss, correct, sq = eng.full_gradient(patches, yd, 0.1, block_strength=bs)
            torch.cuda.synchronize()
            res.append((loss.cpu(), correct.cpu(), sq.cpu(), eng.avg.cpu().double()))
        out[G] = res
        del eng, patches, model
        gc.collect(), torch.cuda.empty_cache()
    a, b = out[n_chunks // 2], out[n_chunks]
    for i in range(2):
        assert torch.equal(a[i][0], b[i][0]) and torch.equal(a[i][1], b[i][1])
        assert float(((a[i][2] - b[i][2]).abs() / a[i][2]).max()) < 1e-5
        err = float((a[i][3] - b[i][3]).norm() / a[i][3].norm())
        cos = float((a[i][3] * b[i][3]).sum() / (a[i][3].norm() * b[i][3].norm()))
        print(f"resnet{depth} fp32 ({split}), {n_chunks} chunks in one group vs two, block_strength {0.5 * i}: mean gradient rel L2 {err:.2e}, cosine {cos:.6f}")
        assert bool(torch.isfinite(b[i][3]).all()) and (err < 1e-4 if i == 0 else cos > 0.99), (i, err, cos)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, "f16x2+fd"])
def test_stem_launch_ranges_equal_one_launch(dtype, monkeypatch):
    """The pre-gathered patches of the ImageNet stem (7x7x3 -> 160 values per pixel) are the largest tensor of ResNet-152 @224 and used to cap
    the chunk group at 4; the two launches that read them are now cut into chunk ranges below 2^31 bytes (Engine._stem_ranges) and the
    group is sized by the other tensors (10 chunks).  A forced split (one chunk per range) must reproduce the single launch bit for bit:
    statistics tables, coefficients, outputs and per-chunk gradient rows are all indexed by chunk."""
    pixels, chunk, G = 64, 32, 3
    x, y = make_data(chunk * G, pixels)
    fd = dtype == "f16x2+fd"                  # the regulariser's passes: per-chunk fp16x2 scales and per-chunk weight sets in the second pass
    dtype = torch.float32 if fd else dtype
    if fd:
        monkeypatch.setenv("FB_F32_SPLIT", "f16x2")
    out = {}
    for limit in (None, 1):
        if limit is None:
            monkeypatch.delenv("FB_STEM_RANGE_BYTES", raising=False)
        else:
            monkeypatch.setenv("FB_STEM_RANGE_BYTES", str(limit))
        cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, dtype, stem="standard", fd_sets=1 if fd else 0)
        assert len(eng._stem_ranges(G)) == (1 if limit is None else G)
        patches = stem_patches(x.cuda(), eng.plan.stem, dtype)
        if fd:
            assert eng.f32_split == "f16x2"
            eng.full_gradient(patches, y.cuda(), 0.1, block_strength=0.5)
            torch.cuda.synchronize()
            out[limit] = (eng.g[:G].clone(), eng.g_fd[0][:G].clone(), eng.avg.clone(), eng.mean_tab[:, :G].clone(), eng.var_tab[:, :G].clone())
            continue
        eng.prep_weights(eng.theta, 1)
        eng.group_gradient(patches, y.cuda(), G, eng.g)
        torch.cuda.synchronize()
        out[limit] = (eng.g[:G].clone(), eng.loss[:G].clone(), eng.mean_tab[0, :G].clone(), eng.var_tab[0, :G].clone())
    for a, b in zip(out[None], out[1]):
        assert torch.equal(a, b)


def test_imagenet_shaped_maps_chunk_gradient_vs_oracle():
    """ResNet-18 with the 'standard' (ImageNet) stem on 96x96 inputs: feature maps 48 -> (MaxPool) 24, 12, 6, 3 -- non-power-of-two
    sizes like the 56/28/14/7 of the 224x224 configurations (every stride-2 transition halves an even size, as there; the
    reference's AvgPool shortcut cannot take odd ones), which go through the generic implicit-GEMM / per-tap weight-gradient
    kernels (the LDS-halo kernels cover 32/16/8/4 only).  One chunk of 128 images (3x3 maps: chunk * 9 must be a multiple of 128)."""
    pixels, chunk, G = 96, 128, 1
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, torch.float32, stem="standard")
    assert {24, 12, 6, 3} <= {L.hout for L in eng.plan.layers}
    x, y = make_data(chunk * G, pixels)
    truth, params, buffers = _oracle_chunk_grads(model, x, y, chunk, depth=18, stem="standard")
    patches = stem_patches(x.cuda(), eng.plan.stem, torch.float32)
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y.cuda(), G, eng.g)
    torch.cuda.synchronize()
    got = _engine_grads_as_lists(eng, G)
    assert abs(float(eng.loss[0]) - truth[0][1]) < 1e-5 * abs(truth[0][1])
    a = torch.cat([t.reshape(-1).double() for t in got[0]])
    t = torch.cat([r.reshape(-1).double() for r in truth[0][0]])
    err = float((a - t).norm() / t.norm())
    print(f"resnet18/standard 96x96: engine-vs-f64-truth {err:.3e}")
    assert err < 2e-2, err
    assert rel_err(got[0][-2].numpy(), truth[0][0][-2].numpy()) < 1e-4


def test_chunk_must_fill_whole_statistics_blocks():
    """BN statistics are reduced per 128-pixel block and a block must not straddle two chunks: refused with a clear message."""
    from fullbatchtraining_amd.lib import EngineError
    with pytest.raises(EngineError, match="multiple of 128"):
        _build(18, 96, 32, 1, torch.float32, stem="standard")       # 3x3 maps: 32 * 9 pixels per chunk


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32-bf16x6"])
def test_resnet18_production_chunk_group_vs_oracle(dtype, monkeypatch):
    """The headline's chunk group end to end: ONE group of 98 distinct chunks of 128 images (default dispatch, replayed command list) against the float64
    oracle's chunk gradient on sampled chunks (0, 1, the last, two seeded others) -- fp32: 3e-3 relative L2 (the reference's own fp32 noise), cosine 0.99999,
    loss 1e-5; bf16: the torch-autocast yardstick of test_resnet18_chunk_gradients_vs_oracle.  Then full_gradient over 390 chunks (groups of 98/98/98/96: the
    last one short of the nominal group): the step's mean gradient and every chunk's squared norm against float64 reductions of the engine's own per-chunk
    gradients, collected group by group (the engine is bit-deterministic)."""
    import os
    import random

    from tests.helpers import err_cos, flat64, torch_bf16_chunk_grads

    for k in list(os.environ):                   # the default dispatch
        if k.startswith("FB_") and k not in ("FB_EXPERIMENTAL", "FB_ORACLE_DEVICE", "FB_TEST_TIMEOUT_S", "FB_TEST_WATCHDOG_S", "FB_SOAK"):
            monkeypatch.delenv(k)
    pixels, chunk, G, n_chunks = 32, 128, 98, 390
    cfg, model, eng, stem_patches = _build(18, pixels, chunk, G, dtype)
    assert eng.use_replay
    x, y = make_data(chunk * n_chunks, pixels, seed=4321)
    patches, yd = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
    eng.prep_weights(eng.theta, 1)
    runs = []
    for _ in range(2):                           # recorded, then replayed: the same bits
        eng.group_gradient(patches[:G * chunk], yd[:G * chunk], G, eng.g)
        torch.cuda.synchronize()
        runs.append((eng.g[:G].clone(), eng.loss[:G].clone(), eng.correct[:G].clone()))
    assert eng.replays >= 1 and all(torch.equal(a, b) for a, b in zip(*runs))
    smp = sorted({0, 1, G - 1} | set(random.Random(0).sample(range(2, G - 1), 2)))
    xs = torch.cat([x[g * chunk:(g + 1) * chunk] for g in smp])
    ys = torch.cat([y[g * chunk:(g + 1) * chunk] for g in smp])
    truth, _, _ = _oracle_chunk_grads(model, xs, ys, chunk)
    got = _engine_grads_as_lists(eng, G)
    if dtype == torch.bfloat16:
        ref, _, _ = _oracle_chunk_grads(model, xs, ys, chunk, emulate_bf16=True)
        yard = torch_bf16_chunk_grads(model, xs, ys, chunk, device="cuda")
    for i, g in enumerate(smp):
        a, t = flat64(got[g]), flat64(truth[i][0])
        e_eng, c_eng = err_cos(a, t)
        if dtype == torch.float32:
            print(f"[fp32, group of {G}] chunk {g}: engine-vs-f64 {e_eng:.3e}, cosine {c_eng:.7f}, loss {float(eng.loss[g]):.6f} vs {truth[i][1]:.6f}")
            assert e_eng < 3e-3 and c_eng > 0.99999, (g, e_eng, c_eng)
            assert abs(float(eng.loss[g]) - truth[i][1]) < 1e-5 * max(1.0, abs(truth[i][1])), g
            assert float(eng.correct[g]) == truth[i][2], g
        else:
            e_tch, c_tch = err_cos(flat64(yard[i][0]), t)
            print(f"[bf16, group of {G}] chunk {g}: engine {e_eng:.3f} / cos {c_eng:.4f}; torch autocast(bf16) {e_tch:.3f} / cos {c_tch:.4f}")
            assert e_eng <= 1.15 * e_tch and c_eng >= c_tch - 0.01, (g, e_eng, e_tch, c_eng, c_tch)
            assert abs(float(eng.loss[g]) - ref[i][1]) < 2e-3 * max(1.0, abs(ref[i][1])), g
            assert abs(float(eng.loss[g]) - yard[i][1]) < 2e-2 * max(1.0, abs(yard[i][1])), g
    # the whole step: 390 chunks in groups of 98/98/98/96
    loss, correct, sq = eng.full_gradient(patches, yd, 0.1)
    torch.cuda.synchronize()
    avg, sq = eng.avg.double().clone(), sq.double().clone()
    total = torch.zeros(eng.plan.P, dtype=torch.float64, device="cuda")
    sq64 = torch.zeros(n_chunks, dtype=torch.float64, device="cuda")
    sizes = []
    for lo in range(0, n_chunks, G):
        g_n = min(G, n_chunks - lo)
        sizes.append(g_n)
        eng.prep_weights(eng.theta, 1)
        eng.group_gradient(patches[lo * chunk:(lo + g_n) * chunk], yd[lo * chunk:(lo + g_n) * chunk], g_n, eng.g)
        torch.cuda.synchronize()
        assert torch.equal(eng.loss[:g_n], loss[lo:lo + g_n])
        for g in range(g_n):
            row = eng.g[g].double()
            total += row
            sq64[lo + g] = row.pow(2).sum()
    assert sizes == [98, 98, 98, 96]
    mean64 = total / n_chunks
    e_mean = float((avg - mean64).norm() / mean64.norm())
    e_sq = float(((sq - sq64).abs() / sq64).max())
    print(f"[{dtype}] full_gradient over {n_chunks} chunks: mean gradient vs float64 {e_mean:.2e}, chunk squared norms (worst) {e_sq:.2e}")
    assert e_mean < 1e-5 and e_sq < 1e-5
