"""Evaluation -- ``valid_loss`` / ``valid_acc``, what a user reads from a run -- against the float64 oracle.

Evaluation runs kernel paths that training never runs: ``Engine.evaluate_batch`` is ONE "chunk" of n images (any n: training insists on whole 128-pixel
statistics blocks), every convolution runs its no-statistics branch (the resident-filter 64-channel kernel refuses a forward call without statistics, so the
64 -> 64 layers on 32 x 32 maps take the persistent halo kernel instead), MaxPool runs without its index buffer and the head kernels run with chunk = n.

1. ``test_eval_walk_*``: the forward walk of tests/test_gpu_bf16_structural.py in evaluation mode.  BN coefficients from ``fb_bn_eval_coeffs`` on given running
   statistics, G = 1, chunk = n, no statistics workspace; every launch is fed the oracle's own tensor of that point (``orc.forward(..., train=False)``, bf16-rounded at
   the storage points for bf16) and EVERY image is compared, with the walk's constants unchanged (REL_L2, ULP2, FLOOR, BAD_FRACTION; fp32: REL_L2_F32, HEAD_F32).
   The launches (class, shape, kernel) must contain everything a plain ``evaluate_batch`` at the same n launches; the kernel names are printed per case.
2. ``evaluate_batch`` and the evaluation loops end to end: logits against the oracle (fp32: elementwise within 5 x plain torch fp32's own distance from float64;
   bf16: relative L2 within 1.15 x torch autocast(bfloat16)'s), loss and #correct against float64 functions of the engine's own logits (``fb_head_loss`` at chunk = n),
   the head kernels at the sizes evaluation really launches, fp32 #correct against the oracle's, ``training.evaluate`` / ``FullBatchTrainer.evaluate`` over a set
   that is not a multiple of the batch (plain, mirrored, EMA copies), and state isolation (an evaluation between two gradient evaluations changes nothing).

Parameters and running statistics: ``helpers.eval_state`` (gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1), running statistics from the data, two epsilon-path channels per
layer) -- at the init state evaluation is degenerate.

Measured (MI355X).  Walk: tensors bf16 <= 1.71e-4 (limit 1e-3), fp32 <= 2.2e-7 (2e-6), head <= 1.4e-7 (fp32 4e-6, bf16 1e-5), coefficients error / bound <= 0.903.
evaluate_batch logits, engine | yardstick: fp32 max |d| ResNet-18 n=100 1.28e-6 | torch fp32 1.91e-6, n=1037 1.59e-6 | 2.66e-6, ResNet-50 n=36 3.57e-5 | 6.32e-5; bf16 relative L2
1.79e-2 | torch autocast 8.39e-2, 1.79e-2 | 1.09e-1, 2.92e-1 | 4.39e-1.  Loss of the engine's own logits: |d| / bound <= 0.032.  Head kernels at evaluation sizes, error / bound:
features 0.081, logits 0.038, loss 0.008, dlogits 0.515.  No image had to be left out of the #correct comparison; the evaluation loops matched the oracle's loss to 5e-7 relative
and its accuracy exactly.  Convolution kernels evaluation reached: ResNet-18 bf16 conv1x1_k32, conv1x1_pipe, conv1x1_stream, conv3x3s1_halo4, conv_igemm_v3; fp32 conv3x3s1_halo4,
conv_igemm_v3; ResNet-50 @64 bf16 conv1x1_pipe, conv1x1_stream, conv3x3s1_halo4, conv_igemm_v3 (fp32: the last two); @224 bf16 conv1x1_pipe, conv1x1_stream, conv_igemm_v3.
"""
import numpy as np
import pytest
import torch

from tests.helpers import (U32, bn_eval_coeffs_ref, eval_state, make_data, mean_loss_bound, oracle_device, oracle_state, to_oracle, within_bound)
from tests.test_gpu_bf16_structural import HEAD_F32, REL_L2, REL_L2_F32, _Checks, _launch_set, _to_dev

pytestmark = pytest.mark.gpu


def _stored_chunk(model, pixels):
    """the smallest chunk an engine can be built with (whole 128-pixel statistics blocks on every map): evaluation itself takes any n"""
    from fullbatchtraining_amd.engine import Plan, padded_chunk
    return padded_chunk(Plan(model, pixels), 32)


_SETUPS = {}


def _setup(depth, stem, pixels, n, classes=10):
    """model in the evaluation state, data, the float64 oracle's evaluation logits (shared by the tests of one shape: computed once, never modified)"""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from oracle import fb_oracle as orc

    key = (depth, stem, pixels, n)
    if key not in _SETUPS:
        cfg = compose([f"model=resnet{depth}", f"model.stem={stem}"])
        torch.manual_seed(0)
        model = construct_model(cfg.model, 3, classes)
        x, y = make_data(n, pixels, classes)
        spec = orc.Spec(depth, stem=stem, classes=classes)
        eps_ch = eval_state(model, spec, x)
        params, buffers = oracle_state(model)
        with torch.no_grad():
            logits64, _ = orc.forward(spec, params, buffers, to_oracle(x), update_bn=False, train=False)
        _SETUPS[key] = dict(model=model, x=x, y=y, spec=spec, eps_ch=eps_ch, logits64=logits64.cpu())
    return _SETUPS[key]


def _engine(s, pixels, n, dtype, split=None, **kw):
    from fullbatchtraining_amd.engine import Engine
    chunk = _stored_chunk(s["model"], pixels)
    return Engine(s["model"], pixels, chunk, -(-n // chunk), compute_dtype=dtype, f32_split=split, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _run_eval_walk(depth, stem, pixels, n, dtype, split=None, monkeypatch=None):
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.engine import BN_EPS, stem_patches
    from fullbatchtraining_amd.lib import call
    from oracle import fb_oracle as orc

    if monkeypatch is not None:                  # the default dispatch: no kernel switch, no override of the arithmetic
        import os
        for k in list(os.environ):
            if k.startswith("FB_") and k not in ("FB_EXPERIMENTAL", "FB_ORACLE_DEVICE", "FB_TEST_TIMEOUT_S", "FB_TEST_WATCHDOG_S", "FB_SOAK"):
                monkeypatch.delenv(k)
    fp32 = dtype == torch.float32
    s = _setup(depth, stem, pixels, n)
    eng = _engine(s, pixels, n, dtype, split)
    assert eng.f32_split == split
    eng.use_replay = False
    plan, dt = eng.plan, eng.dt
    x, y = s["x"], s["y"]
    y_dev = y.cuda()
    q = (lambda t: t.to(torch.float32).to(t.dtype)) if fp32 else (lambda t: t.to(torch.bfloat16).to(t.dtype))
    params, buffers = oracle_state(s["model"])
    with torch.no_grad():
        logits_o, tape = orc.forward(s["spec"], params, buffers, to_oracle(x), q, update_bn=False, train=False)
    loss_o, correct_o, _ = orc.cross_entropy_fwd_bwd(logits_o, to_oracle(y))
    ck = _Checks(fp32)
    patches = stem_patches(x.cuda(), plan.stem, dt)
    hw = plan.h_final * plan.h_final

    def fwd_conv(L, src, rec, tag):
        eng._conv_bn_fwd(L, src, 1, 1, eng.theta, 0)
        raw = q(orc.conv_fwd(rec["x"], rec["w"], rec["stride"], rec["pad"]))
        ck.close(L.x[:n], raw, f"{tag} conv output")
        L.x[:n].copy_(_to_dev(raw, dt))

    def act_check(t, val, tag):
        ck.close(t[:n], val, tag)
        t[:n].copy_(_to_dev(val, dt))

    lib.profile_enable(True, 1 << 16)
    saved = (eng.chunk, eng.valid)
    try:
        eng.prep_weights(eng.theta, 1)
        worst_c = 0.0
        for L in plan.layers:
            call("fb_bn_eval_coeffs", eng.theta.data_ptr() + 4 * L.g_off, eng.theta.data_ptr() + 4 * L.b_off, eng.running_mean.data_ptr() + 4 * L.ch_off,
                 eng.running_var.data_ptr() + 4 * L.ch_off, BN_EPS, L.scale.data_ptr(), L.shift.data_ptr(), L.cout)
            # (the float64 side starts from the fp32 values the kernel reads)
            sc, sh, bsc, bsh = bn_eval_coeffs_ref(eng.theta[L.g_off:L.g_off + L.cout], eng.theta[L.b_off:L.b_off + L.cout],
                                                  eng.running_mean[L.ch_off:L.ch_off + L.cout], eng.running_var[L.ch_off:L.ch_off + L.cout])
            c0, c1 = s["eps_ch"][L.bn_name]
            assert float(eng.running_var[L.ch_off + c0]) == 0.0 and float(eng.running_var[L.ch_off + c1]) == float(np.float32(1e-6))
            worst_c = max(worst_c, within_bound(L.scale[0], sc, bsc)[0], within_bound(L.shift[0], sh, bsh)[0])
        ck.worst("evaluation coefficients (scale, shift) of all layers, error / arithmetic bound", worst_c, 0, 1.0)
        eng.chunk, eng.valid, eng._eval = n, n, True
        eng.amax_map.clear()
        fwd_conv(plan.stem, patches, tape[0]["rec"], "stem")
        eng._bn_apply(plan.stem, eng.stem_out, 1)
        act_check(eng.stem_out, tape[0]["relu_out"] if plan.stem_pool else tape[0]["out"], "stem BN+ReLU")
        a_prev = eng.stem_out
        if plan.stem_pool:                       # evaluation: MaxPool without the index buffer
            s_ = plan.stem
            call("fb_maxpool3s2_fwd", eng.stem_out.data_ptr(), eng.stem_pooled.data_ptr(), n, s_.hout, s_.wout, 64, eng.dtc)
            ck.close(eng.stem_pooled[:n], tape[0]["out"], "stem MaxPool2d(3,2,1)")
            assert torch.equal(eng.stem_pooled[:n], _to_dev(tape[0]["out"], dt))           # (a selection: no rounding at all)
            a_prev = eng.stem_pooled
        for bi, b in enumerate(plan.blocks):
            tag, E = f"block {bi}", tape[1 + bi]
            nxt = plan.blocks[bi + 1] if bi + 1 < len(plan.blocks) else None
            cur = a_prev
            for i, L in enumerate(b.convs[:-1]):
                fwd_conv(L, cur, E["recs"][i], f"{tag} conv{i + 1}")
                eng._bn_apply(L, b.mids[i], 1)
                act_check(b.mids[i], E["mids"][i], f"{tag} BN{i + 1}+ReLU")
                cur = b.mids[i]
            last = b.convs[-1]
            fwd_conv(last, cur, E["recs"][-1], f"{tag} conv{len(b.convs)}")
            next_pool = nxt.pooled if nxt is not None else None
            if b.shortcut is not None:
                src = a_prev
                if b.pooled is not None:
                    call("fb_avgpool2_fwd", a_prev.data_ptr(), b.pooled.data_ptr(), n, b.hin, b.win, b.cin, eng.dtc)
                    act_check(b.pooled, E["rd"]["x"], f"{tag} AvgPool2d(2,2)")
                    src = b.pooled
                fwd_conv(b.shortcut, src, E["rd"], f"{tag} shortcut conv")
                fused = eng._bn_apply(last, b.out, 1, res=b.shortcut.x, resL=b.shortcut, pool=next_pool)
            else:
                fused = eng._bn_apply(last, b.out, 1, res=a_prev, pool=next_pool)
            if fused:
                ck.close(nxt.pooled[:n], q(orc.avgpool2_fwd(E["out"])), f"{tag} fused pooled output")
            act_check(b.out, E["out"], f"{tag} last BN + residual + ReLU")
            a_prev = b.out
        call("fb_head_pool", a_prev.data_ptr(), eng.feat.data_ptr(), n, hw, plan.feat, eng.dtc)
        call("fb_head_loss", eng.feat.data_ptr(), eng.theta.data_ptr() + 4 * plan.fcw_off, eng.theta.data_ptr() + 4 * plan.fcb_off, 0, y_dev.data_ptr(),
             eng.logits.data_ptr(), eng.dlogits.data_ptr(), eng.loss.data_ptr(), eng.correct.data_ptr(), 1, n, plan.feat, plan.classes, 0.0, 0)
        hb = HEAD_F32 if fp32 else 1e-5          # (the training walk's head bounds)
        ck.close_vec(eng.feat[:n], tape[-1]["feat"], "head pooled features", hb)
        ck.close_vec(eng.logits[:n], logits_o, "logits", hb)
        # an image whose two largest logits are closer than the logits' own tolerance may be counted either way
        top2 = logits_o.topk(2, dim=1).values
        unsure = int(((top2[:, 0] - top2[:, 1]) < 2 * hb * float(logits_o.abs().max())).sum())
        if not (abs(float(eng.loss[0]) - float(loss_o)) < 1e-5 * float(loss_o) and abs(float(eng.correct[0]) - float(correct_o)) <= unsure):
            ck.fails.append(f"loss / #correct: {float(eng.loss[0])} / {float(eng.correct[0])} vs {float(loss_o)} / {float(correct_o)} ({unsure} images undecided)")
        torch.cuda.synchronize()
        ck.launches = _launch_set(lib.profile_read_launches())
        lib.profile_read()
        (eng.chunk, eng.valid), eng._eval = saved, False
        eng.evaluate_batch(patches, y_dev)       # what a plain evaluation of the same batch launches: the walk must have launched all of it
        torch.cuda.synchronize()
        want = _launch_set(lib.profile_read_launches())
        lib.profile_read()
    finally:
        (eng.chunk, eng.valid), eng._eval = saved, False
        lib.profile_enable(False)
    missing = want - ck.launches
    kernels = sorted({lib.PROF_KERNELS.get(w[-1], str(w[-1])) for c, w in ck.launches if c == "igemm_fwd"})
    print(f"resnet{depth} / {stem} stem / {pixels} px / n = {n} / {'fp32 ' + split if fp32 else 'bf16'}: {len(ck.report)} tensors compared (every image); largest relative L2:")
    for what, rel, bad in sorted(ck.report, key=lambda r: -r[1])[:5]:
        print(f"  {what}: {rel:.3e} ({bad:.1e} of the elements beyond 2 ulp)")
    print(f"  tensors {ck.worst_tensor:.3e} (limit {REL_L2_F32 if fp32 else REL_L2:.0e}), head {ck.worst_sum:.3e} (limit {hb:.0e}), coefficients error / bound {worst_c:.3f}")
    print(f"  {len(ck.launches)} distinct launches; evaluation's convolution kernels: {kernels}; of evaluate_batch's {len(want)} launches {len(missing)} not walked")
    if missing:
        ck.fails.append(f"launches of evaluate_batch the walk did not make: {sorted(missing)[:8]}")
    assert want, "the profile recorded nothing"
    return ck, kernels


def _eval_walk(*args, **kw):
    import gc
    ck, kernels = _run_eval_walk(*args, **kw)
    gc.collect()
    torch.cuda.empty_cache()
    ck.check()
    return ck, kernels


@pytest.mark.parametrize("n", [1, 6, 100, 528, 1037])
@pytest.mark.parametrize("dtype,split", [(torch.bfloat16, None), (torch.float32, "bf16x6")], ids=["bf16", "fp32-bf16x6"])
def test_eval_walk_resnet18(n, dtype, split, monkeypatch):
    """n = 6 breaks n % 4 (8 x 8 maps), 100 breaks n % 16 only (4 x 4 maps), 528 gives the persistent workgroups several tiles each, 1037 is ragged in every layer."""
    ck, kernels = _eval_walk(18, "CIFAR", 32, n, dtype, split, monkeypatch=monkeypatch)
    assert len(ck.report) > 40
    assert "conv3x3s1_c64_halo5_kernel" not in kernels          # (it needs the statistics workspace: evaluation's 64 -> 64 layers go elsewhere)


def test_eval_walk_resnet18_fp32_f16x2(monkeypatch):
    """fp16x2 operand split with ONE scale group of n images (``amax_imgs = n``)"""
    _eval_walk(18, "CIFAR", 32, 100, torch.float32, "f16x2", monkeypatch=monkeypatch)


@pytest.mark.parametrize("n", [1, 5, 36])
@pytest.mark.parametrize("dtype,split", [(torch.bfloat16, None), (torch.float32, "bf16x6")], ids=["bf16", "fp32-bf16x6"])
def test_eval_walk_resnet50_standard_stem(n, dtype, split, monkeypatch):
    """``fb_maxpool3s2_fwd`` without the index buffer, the 160-value stem patches, the Bottleneck 1 x 1 routes"""
    ck, _ = _eval_walk(50, "standard", 64, n, dtype, split, monkeypatch=monkeypatch)
    assert any("MaxPool" in r[0] for r in ck.report) and len(ck.report) > 100


def test_eval_walk_resnet50_at_224(monkeypatch):
    """56 / 28 / 14 / 7 maps with ragged pixel counts (n = 3)"""
    _eval_walk(50, "standard", 224, 3, torch.bfloat16, monkeypatch=monkeypatch)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _torch_logits(s, autocast):
    """the project's own parameter container in .eval(): plain torch (fp32, or autocast(bfloat16)) -- the yardstick"""
    import copy
    m = copy.deepcopy(s["model"]).cuda().float().eval()
    with torch.no_grad():
        if autocast:
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                return m(s["x"].cuda()).float().double().cpu()
        return m(s["x"].cuda()).double().cpu()


@pytest.mark.parametrize("depth,stem,pixels,n", [(18, "CIFAR", 32, 100), (18, "CIFAR", 32, 1037), (50, "standard", 64, 36)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_evaluate_batch_logits_loss_and_correct(depth, stem, pixels, n, dtype):
    """Logits of ``evaluate_batch`` against the oracle's evaluation forward; loss and #correct against float64 functions of the engine's OWN logits (isolates
    ``fb_head_loss`` at chunk = n: the bound is fp32 rounding of a mean over n, ``helpers.mean_loss_bound``); fp32: #correct against the oracle's, leaving out the
    images whose float64 top-two margin is below twice the logit bound (each of the two logits may be off by the bound) -- at most 1 % of a batch, none at
    n <= 100 (checked: with the data seed of helpers.make_data the oracle's smallest margins are 1.1e-2 at n = 100 and 1.1e-3 for ResNet-50 at n = 36)."""
    from fullbatchtraining_amd.engine import stem_patches
    from oracle import fb_oracle as orc

    s = _setup(depth, stem, pixels, n)
    eng = _engine(s, pixels, n, dtype)
    y_dev = s["y"].cuda()
    loss, correct = eng.evaluate_batch(stem_patches(s["x"].cuda(), eng.plan.stem, dtype), y_dev)
    got = eng.logits[:n].double().cpu()
    ref = s["logits64"]
    if dtype == torch.float32:
        yard = float((_torch_logits(s, False) - ref).abs().max())
        err = float((got - ref).abs().max())
        bound = 5 * yard
        print(f"resnet{depth} n={n} fp32: logits max |engine - float64| {err:.3e}; torch fp32 {yard:.3e} (limit 5 x = {bound:.3e}); max |logit| {float(ref.abs().max()):.3f}")
        assert err <= bound
        top2 = ref.topk(2, dim=1).values
        keep = (top2[:, 0] - top2[:, 1]) >= 2 * bound
        left_out = n - int(keep.sum())
        print(f"  #correct: {left_out} of {n} images left out (float64 margin below {2 * bound:.2e})")
        assert left_out <= n // 100 and (n > 100 or left_out == 0)
        assert torch.equal(got.argmax(1)[keep], ref.argmax(1)[keep])
        correct64 = float((ref.argmax(1) == s["y"]).sum())
        assert abs(correct - correct64) <= left_out
    else:
        rel = lambda a: float((a - ref).norm() / ref.norm())                   # noqa: E731
        e_eng, e_tch = rel(got), rel(_torch_logits(s, True))
        print(f"resnet{depth} n={n} bf16: logits relative L2 to float64: engine {e_eng:.3e}; torch autocast(bfloat16) {e_tch:.3e} (limit 1.15 x)")
        assert e_eng <= 1.15 * e_tch
    # fb_head_loss at chunk = n on the engine's own logits
    loss64, correct_own, _ = orc.cross_entropy_fwd_bwd(eng.logits[:n].double(), y_dev)
    lb = mean_loss_bound(n, eng.plan.classes, eng.logits[:n], y_dev)
    print(f"  loss {loss:.7f} vs float64 of the same logits {float(loss64):.7f}: |d| / bound {abs(loss - float(loss64)) / lb:.3f} (bound {lb:.2e}); #correct {correct}")
    assert abs(loss - float(loss64)) <= lb
    assert correct == float(correct_own)


@pytest.mark.parametrize("n,classes", [(10000, 10), (12544, 10), (1024, 1000), (784, 10)])
def test_head_kernels_at_evaluation_sizes(n, classes):
    """``fb_head_pool`` + ``fb_head_loss`` with G = 1 and chunk = n at the sizes evaluation launches (10 000 validation images as one chunk, the 98 x 128 cap, the
    1024-image batches of ``training.evaluate`` and their tail of 784; training never goes above 200) on synthetic bf16 features, against float64 with bounds from
    the arithmetic: features a sequential sum of hw terms; logits 64 lanes x C / 64 products, six shuffle adds, the bias; loss ``mean_loss_bound``; #correct exact;
    dlogits (softmax - onehot) / n with the loss's per-image terms."""
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.lib import call

    lib.load()
    C, hw = 512, 16
    gen = torch.Generator(device="cuda").manual_seed(n + classes)
    a = (torch.randn(n, hw, C, device="cuda", generator=gen).abs() * (1 + torch.arange(C, device="cuda") % 7)).to(torch.bfloat16)
    W = torch.randn(classes, C, device="cuda", generator=gen) * 0.02
    b = torch.randn(classes, device="cuda", generator=gen) * 0.1
    y = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    f32 = dict(device="cuda", dtype=torch.float32)
    feat, logits, dlogits = torch.empty(n, C, **f32), torch.empty(n, classes, **f32), torch.empty(n, classes, **f32)
    loss, correct = torch.full((1,), -1.0, **f32), torch.full((1,), -1.0, **f32)
    call("fb_head_pool", a.data_ptr(), feat.data_ptr(), n, hw, C, lib.dtype_code(torch.bfloat16))
    call("fb_head_loss", feat.data_ptr(), W.data_ptr(), b.data_ptr(), 0, y.data_ptr(), logits.data_ptr(), dlogits.data_ptr(), loss.data_ptr(), correct.data_ptr(),
         1, n, C, classes, 0.0, 0)
    torch.cuda.synchronize()
    a64 = a.double()
    r_feat = within_bound(feat, a64.mean(1), U32 * ((hw + 1) * a64.abs().mean(1)))[0]
    f64 = feat.double()
    lg64 = f64 @ W.double().t() + b.double()
    r_log = within_bound(logits, lg64, U32 * ((C // 64 + 8) * (f64.abs() @ W.double().abs().t()) + b.double().abs() + lg64.abs()))[0]
    z = logits.double()                                   # the loss of the engine's own logits
    zm = z - z.max(1, keepdim=True).values
    lse = zm.exp().sum(1, keepdim=True).log()
    p = (zm - lse).exp()
    onehot = torch.nn.functional.one_hot(y, classes).double()
    loss64 = float((lse[:, 0] - zm[torch.arange(n, device="cuda"), y]).mean())
    lb = mean_loss_bound(n, classes, z, y)
    dlogp = U32 * (2 * zm.abs() + (classes + 2) + 3 * lse)
    r_dl = within_bound(dlogits, (p - onehot) / n, (p * (dlogp + 2 * U32) + 3 * U32 * (p + onehot)) / n)[0]
    r_loss = abs(float(loss) - loss64) / lb
    print(f"head at n = {n}, {classes} classes: error / bound features {r_feat:.3f}, logits {r_log:.3f}, loss {r_loss:.3f} (loss {float(loss):.6f}), dlogits {r_dl:.3f}")
    assert r_feat <= 1.0 and r_log <= 1.0 and r_loss <= 1.0 and r_dl <= 1.0
    assert float(correct) == float((logits.argmax(1) == y).sum())


# ------------------------------------------------------------------------------------------------------------------------------------------------------
def _undecided(out64, tol):
    top2 = out64.topk(2, dim=1).values
    return int(((top2[:, 0] - top2[:, 1]) < tol).sum())


def _oracle_eval(s, batch, flips):
    """``orc.evaluate`` with the same batching, and the number of images whose decision is closer than 1e-5 (fp32 noise of the decided quantity)"""
    from oracle import fb_oracle as orc
    params, buffers = oracle_state(s["model"])
    xo, yo = to_oracle(s["x"], s["y"])
    with torch.no_grad():
        vl, va = orc.evaluate(s["spec"], params, buffers, xo, yo, batch=batch, test_time_flips=flips)
        out = s["logits64"].to(oracle_device())
        if flips:
            out = out.softmax(1) + orc.forward(s["spec"], params, buffers, torch.flip(xo, [3]), update_bn=False, train=False)[0].softmax(1)
    return vl, va, _undecided(out, 1e-5)


@pytest.mark.parametrize("flips", [False, True], ids=["plain", "test_time_flips"])
def test_training_evaluate_over_a_set_that_is_no_multiple_of_the_batch(flips):
    """``training.evaluate`` (1024-image batches) over 2 x 1024 + 37 images: the l * n weighting and the tail; with ``test_time_flips`` the mirrored gather in
    ``fb_stem_patches``, ``fb_head_tta`` and the sum of softmaxes.  fp32: loss to 1e-5 relative (the engine tests' fp32 loss tolerance), accuracy to the images
    whose decision is closer than 1e-5."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.training import evaluate

    n = 2 * 1024 + 37
    s = _setup(18, "CIFAR", 16, n)
    cfg = compose(["impl.mixed_precision=False", f"hyp.test_time_flips={flips}"])
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    stats = evaluate(s["model"], (s["x"], s["y"]), None, setup, cfg.impl, cfg.hyp)
    vl, va, unsure = _oracle_eval(s, 1024, flips)
    print(f"training.evaluate, {n} images, flips {flips}: loss {stats['valid_loss'][-1]:.7f} vs {vl:.7f}, acc {stats['valid_acc'][-1]:.5f} vs {va:.5f} ({unsure} undecided)")
    assert abs(stats["valid_loss"][-1] - vl) <= 1e-5 * abs(vl)
    assert abs(stats["valid_acc"][-1] - va) * n <= unsure + 1e-6


@pytest.mark.parametrize("mode", ["plain", "test_time_flips", "evaluate_ema"])
def test_trainer_evaluate_over_a_set_that_is_no_multiple_of_the_cap(mode, tmp_path):
    """``FullBatchTrainer.evaluate`` with an engine cap of 2 chunks x 32 images over 2 x 64 + 37 validation images.  ``evaluate_ema``: the numbers come from the EMA
    copies (the live parameters and running statistics are moved away first) and theta / running_mean / running_var, live and EMA, are bit-identical afterwards."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.training import FullBatchTrainer

    cap = 64
    n = 2 * cap + 37
    s = _setup(18, "CIFAR", 32, n)
    cfg = compose(["hyp=fb1", "data.batch_size=32", "hyp.sub_batch=32", "impl.engine.chunk_group=2", "impl.mixed_precision=False",
                   f"hyp.test_time_flips={mode == 'test_time_flips'}", f"hyp.evaluate_ema={mode == 'evaluate_ema'}"], original_cwd=str(tmp_path), name="eval")
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    tr = FullBatchTrainer(s["model"], (s["x"][:cap], s["y"][:cap]), (s["x"], s["y"]), setup, cfg)
    eng = tr.engine
    assert eng.G * eng.chunk == cap
    vl, va, unsure = _oracle_eval(s, cap, mode == "test_time_flips")
    if mode == "evaluate_ema":
        eng.ema_init()
        eng.theta.mul_(1.05)
        eng.running_mean.add_(0.1)
        eng.running_var.mul_(1.2)
        names = ("theta", "running_mean", "running_var", "theta_ema", "running_mean_ema", "running_var_ema")
        before = {k: getattr(eng, k).clone() for k in names}
    stats = tr.evaluate()
    print(f"FullBatchTrainer.evaluate, {n} images, {mode}: loss {stats['valid_loss'][-1]:.7f} vs {vl:.7f}, acc {stats['valid_acc'][-1]:.5f} vs {va:.5f} ({unsure} undecided)")
    assert abs(stats["valid_loss"][-1] - vl) <= 1e-5 * abs(vl)
    assert abs(stats["valid_acc"][-1] - va) * n <= unsure + 1e-6
    if mode == "evaluate_ema":
        assert all(torch.equal(getattr(eng, k), before[k]) for k in names)
        tr.cfg.hyp.evaluate_ema = False                     # the live (moved) state evaluates to something else
        live = tr.evaluate()["valid_loss"][-1]
        assert abs(live - vl) > 1e-3 * abs(vl)


@pytest.mark.parametrize("dtype,split,fd", [(torch.bfloat16, None, False), (torch.float32, "f16x2", True)], ids=["bf16-replay", "fp32-f16x2-gradreg"])
def test_an_evaluation_between_two_gradient_evaluations_changes_nothing(dtype, split, fd):
    """full_gradient -> evaluate -> full_gradient leaves loss, per-chunk norms, ``avg`` and the running statistics bit-identical to full_gradient -> full_gradient
    (evaluation overwrites L.scale / L.shift, chunk, valid and the f16x2 scale slots)."""
    from fullbatchtraining_amd.engine import Engine, stem_patches

    s = _setup(18, "CIFAR", 32, 100)
    x, y = make_data(4 * 32, 32, seed=77)
    kw = dict(block_strength=0.5, eps=1e-2, implementation="forward-differences") if fd else {}
    out = []
    for with_eval in (False, True):
        eng = Engine(s["model"], 32, 32, 2, compute_dtype=dtype, fd_sets=1 if fd else 0, f32_split=split)
        assert eng.use_replay
        patches, labels = stem_patches(x.cuda(), eng.plan.stem, dtype), y.cuda()
        eng.full_gradient(patches, labels, 0.1, **kw)
        if with_eval:
            for n in (37, 64):
                eng.evaluate_batch(stem_patches(s["x"][:n].cuda(), eng.plan.stem, dtype), s["y"][:n].cuda())
            assert (eng.chunk, eng.valid) == (32, 32) and not eng._eval
        loss_k, correct_k, sq_k = eng.full_gradient(patches, labels, 0.1, **kw)
        torch.cuda.synchronize()
        out.append([t.clone() for t in (loss_k, correct_k, sq_k, eng.avg, eng.running_mean, eng.running_var)] + [eng.num_batches_tracked, eng.replays])
    for a, b in zip(out[0][:6], out[1][:6]):
        assert torch.equal(a, b)
    assert out[0][6] == out[1][6] and out[1][7] > 0 and bool(torch.isfinite(out[0][3]).all()) and float(out[0][3].abs().max()) > 0
