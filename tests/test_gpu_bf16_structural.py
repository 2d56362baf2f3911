"""Structural parity of the bf16 path -- the arithmetic behind bench.py's headline number -- at the benchmark's REAL shapes (ResNet-18, 32x32,
one chunk of 128 images), kernel by kernel.

End-to-end a bf16 chunk gradient is 0.2 away from the fp32 one (ReLU masks of 2^-9-rounded pre-activations flip; tests/test_gpu_bf16_parity.py
shows that this is noise that averages out over chunks), which would also hide a REAL error of a few per cent in one bf16 kernel.  This test
removes the chaos instead of averaging over it: it walks the network layer by layer in the order of the reference's graph
(fullbatch/models/resnets.py:179-230 forward, autograd's backward of it) and feeds EVERY library launch the float64 oracle's own tensors of
that point -- bf16-rounded at the engine's storage points (oracle ``q = bf16_round``), ReLU masks included -- so that each kernel is compared
with exact arithmetic on identical inputs.  What remains is one bf16 rounding of the output (2^-9 relative) plus fp32 accumulation: every
tensor must agree to 1e-3 relative L2 (measured 4e-5) and element-wise to 2 ulp (plus a floor for cancelling sums).  A wrong tap, parity class, mask bit,
channel slice or coefficient in any of the production bf16 kernels (resident-filter 64-channel, persistent halo, implicit GEMM, stride-2 quad
input gradient, streaming stem, all-taps / per-tap weight gradients, BN apply with residual / pooled output, BN backward with bitmask) moves a
tensor by >= 1/9 and fails here; the suite's statistical bf16 assertions would not see it.

The same walk runs at the chunk groups the shipped configurations launch (98 x 128 and 84 x 200 in bf16, config 3's group in fp32 with both
convolution arithmetics and per-chunk weight sets, ResNet-50 @224 at 16 and 8 chunks): every launch covers the whole group of distinct chunks, the
oracle's tensors are injected into the sampled chunks' slices only, the BatchNorm statistics and the head are checked on every chunk, and the set of
launches (class, shape, kernel) must contain everything a plain ``group_gradient`` of the same engine launches.
"""
import numpy as np
import pytest
import torch

from tests.helpers import make_data, oracle_state, to_oracle

pytestmark = pytest.mark.gpu

REL_L2 = 1e-3               # bf16, per tensor (measured: <= 4.1e-5 on all 209 tensors; a wrong tap moves a tensor by >= 0.1)
ULP2 = 2.0 ** -7            # element-wise: 2 bf16 ulp of the reference value ...
FLOOR = 2.0 ** -9           # ... plus this fraction of the tensor's rms (outputs that are small differences of large terms)
BAD_FRACTION = 1e-3         # elements allowed outside the element-wise bound (1-ulp accumulator differences next to a rounding boundary)
REL_L2_F32 = 2e-6           # fp32 storage (bf16x6 and f16x2 convolutions), per tensor (measured: <= 2.3e-7)
REL_L2_F32_SUM = 1e-4       # fp32, per-channel reductions: batch statistics, dgamma / dbeta, weight gradients (measured: <= 2.5e-5, the stem's batch mean on
#                             224 px -- a near-zero vector for zero-mean input images, so fp32 accumulation error is large against its small norm)
HEAD_F32 = 4e-6             # fp32, the head of every chunk: pooled features, logits / loss, dlogits, fc gradients (measured: <= 4.6e-7; bf16: 1e-5)
# per-chunk BN statistics of EVERY chunk against float64 reductions of the engine's own conv output, max over channels of |d mean| / sqrt(var + eps) and
# |d var| / (var + eps) (measured: bf16 1.1e-3 -- the float64 side reduces the bf16-ROUNDED output, the engine its fp32 accumulators --, fp32 1.4e-6)
STAT_TOL = {torch.bfloat16: 5e-3, torch.float32: 1e-5}
N_CHUNKS_CIFAR = 390        # the headline's 50 000 images in chunks of 128


def _to_dev(t, dtype):
    """oracle NCHW float64 (values exact in ``dtype``) -> NHWC ``dtype`` on the device"""
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _nchw(t, device):
    """device NHWC -> NCHW float64 on ``device`` (the oracle's: on a GPU box the comparison never leaves the device -- a ResNet-50 walk at 224 px compares ~6 G elements)"""
    return t.to(device).double().permute(0, 3, 1, 2)


class _Checks:
    """Everything one walk compared: ``report`` [(what, relative L2, fraction beyond 2 ulp)] of the sampled chunks' tensors, ``stats`` [(what, worst, chunk)]
    of the checks that cover every chunk of the group, ``fails`` the comparisons beyond their bound.  The walk records every comparison and asserts at the
    end, so that one run reports the whole distribution."""
    def __init__(self, fp32):
        self.fp32, self.report, self.stats, self.fails, self.launches, self.samples = fp32, [], [], [], set(), []
        self.worst_tensor = self.worst_sum = 0.0

    def check(self):
        assert not self.fails, f"{len(self.fails)} comparisons beyond their bounds:\n  " + "\n  ".join(self.fails[:20])

    def close(self, got_nhwc, ref_nchw, what):
        ref = ref_nchw.double()
        got = _nchw(got_nhwc, ref.device)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        diff = (got - ref).abs()
        rms = float(ref.pow(2).mean().sqrt())
        rel = float(diff.norm() / max(float(ref.norm()), 1e-30))
        bad = float((diff > ULP2 * ref.abs() + FLOOR * rms).double().mean())
        self.report.append((what, rel, bad))
        self.worst_tensor = max(self.worst_tensor, rel)
        lim = REL_L2_F32 if self.fp32 else REL_L2
        if not (np.isfinite(rel) and rel < lim):
            self.fails.append(f"{what}: relative L2 {rel:.3e} (limit {lim:.1e})")
        if not bad < BAD_FRACTION:
            self.fails.append(f"{what}: {bad:.2e} of the elements beyond 2 ulp (+ {FLOOR:.1e} rms)")

    def close_vec(self, got, ref, what, tol):
        ref = ref.double().reshape(-1)
        got = got.double().to(ref.device).reshape(-1)
        rel = float((got - ref).norm() / max(float(ref.norm()), 1e-30))
        self.report.append((what, rel, 0.0))
        self.worst_sum = max(self.worst_sum, rel)
        lim = min(tol, REL_L2_F32_SUM) if self.fp32 else tol
        if not (np.isfinite(rel) and rel < lim):
            self.fails.append(f"{what}: relative L2 {rel:.3e} (limit {lim:.1e})")

    def worst(self, what, value, chunk, lim):
        self.stats.append((what, value, chunk))
        if not (np.isfinite(value) and value < lim):
            self.fails.append(f"{what}: {value:.3e} at chunk {chunk} (limit {lim:.1e})")


def _mask_bytes(positive_nchw, vec=8):
    """ReLU bitmask in the layout fb_bn_apply writes: one byte per 16-byte vector (``vec`` elements) of the NHWC tensor, bit k = element k > 0"""
    bits = positive_nchw.permute(0, 2, 3, 1).contiguous().reshape(-1, vec).to(torch.int32)
    weights = (2 ** torch.arange(vec, dtype=torch.int32, device=bits.device))
    return (bits * weights).sum(1).to(torch.uint8).cuda()


def _sampled_chunks(eng, G, n_random=2, seed=0):
    """0, 1 and G-1; the chunk that holds byte 2^31 (and 2^32) of every tensor that large; the first chunk of every stem range; ``n_random`` seeded others."""
    import random

    es = torch.empty((), dtype=eng.dt).element_size()
    S = eng.plan.stem
    per_chunk = {eng.chunk * S.hin * S.win * S.cin_pad * es}                   # the stem's patches
    for L in eng.plan.layers:
        per_chunk.add(eng.chunk * L.hout * L.wout * L.cout * es)
        per_chunk.add(eng.chunk * L.hin * L.win * L.cin_pad * es)
    out = {0, 1, G - 1} | {g0 for g0, _ in eng._stem_ranges(G)}
    for b in per_chunk:
        out |= {off // b for off in (1 << 31, 1 << 32) if off < G * b}
    rest = [g for g in range(G) if g not in out]
    out |= set(random.Random(seed).sample(rest, min(n_random, len(rest))))
    return sorted(g for g in out if 0 <= g < G)


def _launch_set(records):
    """(class, shape words incl. the kernel id) of every recorded launch"""
    return {(cls, words) for cls, words, _ in records}


def _walk(*args, **kwargs):
    """``_run_walk``, then its assertions -- after its engine and oracle tapes are gone (a failing test must not keep a group's tensors alive)"""
    import gc

    ck = _run_walk(*args, **kwargs)
    gc.collect()
    torch.cuda.empty_cache()
    ck.check()
    return ck


def _run_walk(depth, stem, pixels, chunk, classes=10, G=1, dtype=torch.bfloat16, split=None, passes=None, x_scale=None, monkeypatch=None, per_chunk_sets=False):
    """Forward and backward walk through ``resnet<depth>`` with the given stem: every production launch of a chunk group of ``G`` chunks, with the float64
    oracle's own tensors injected into the slices of the sampled chunks.  ``passes``: [(sampled chunks, per_chunk)] -- one walk each (the oracle tapes of a
    pass are held together); ``per_chunk``: one weight set per chunk (the regulariser's second pass: ``prep_weights(theta_k, G, per_chunk=True)``,
    distinct perturbations; needs ``per_chunk_sets``).  ``x_scale``: per-chunk factors of the input images.  Returns the ``_Checks`` (not yet asserted)."""
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.lib import call
    from fullbatchtraining_amd.models import construct_model
    from oracle import fb_oracle as orc
    from tests.helpers import oracle_device

    if monkeypatch is not None:                  # the default dispatch: no kernel switch, no override of the arithmetic
        import os
        for k in list(os.environ):
            if k.startswith("FB_") and k not in ("FB_EXPERIMENTAL", "FB_ORACLE_DEVICE", "FB_TEST_TIMEOUT_S", "FB_TEST_WATCHDOG_S", "FB_SOAK"):
                monkeypatch.delenv(k)
    fp32 = dtype == torch.float32
    any_pc = per_chunk_sets
    cfg = compose([f"model=resnet{depth}", f"model.stem={stem}"])
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, classes)
    eng = Engine(model, pixels, chunk, G, compute_dtype=dtype, fd_sets=1 if any_pc else 0, f32_split=split)
    assert eng.f32_split == split
    eng.use_replay = False                       # primitives are called one by one with injected tensors
    plan, dt = eng.plan, eng.dt
    vec = 16 // torch.empty((), dtype=dt).element_size()
    x, y = make_data(G * chunk, pixels, classes)
    if x_scale is not None:
        x = x * torch.tensor(x_scale, dtype=x.dtype).repeat_interleave(chunk).view(-1, 1, 1, 1)
    y_dev = y.cuda()
    if fp32:
        q = lambda t: t.to(torch.float32).to(t.dtype)       # noqa: E731
    else:
        q = lambda t: t.to(torch.bfloat16).to(t.dtype)      # noqa: E731  (orc.bf16_round returns float32; the walk runs in float64)
    spec = orc.Spec(depth, stem=stem, classes=classes)
    params0, buffers = oracle_state(model)
    odev = oracle_device()
    ck = _Checks(fp32)
    n, hw = G * chunk, plan.h_final * plan.h_final
    patches = stem_patches(x.cuda(), plan.stem, dt)
    if any_pc:                                   # one weight set per chunk: a distinct multiplicative perturbation of every parameter
        gen = torch.Generator(device="cuda").manual_seed(7)
        for g in range(G):
            eng.theta_k[g] = eng.theta * (1 + 0.05 * torch.randn(plan.P, generator=gen, device="cuda"))

    def sl(t, g):
        return t[g * chunk:(g + 1) * chunk]

    def sfx(g):
        return f" [chunk {g}]" if G > 1 else ""

    def one_pass(smp, per_chunk):
        wsets, pidx = (2, 1) if per_chunk else (1, 0)
        theta = eng.theta_k if per_chunk else eng.theta
        gout = eng.g_fd[0] if per_chunk else eng.g
        gout.zero_()
        eng.prep_weights(theta, G if per_chunk else 1, per_chunk=per_chunk)
        eng.amax_map.clear()
        tapes = {}
        for g in smp:
            params = params0 if not per_chunk else {k: eng._unflatten(eng.theta_k[g], k).double().to(odev) for k in params0}
            xo, yo = to_oracle(x[g * chunk:(g + 1) * chunk], y[g * chunk:(g + 1) * chunk])
            logits_o, tape = orc.forward(spec, params, buffers, xo, q, update_bn=False, train=True)
            loss_o, correct_o, dlogits_o = orc.cross_entropy_fwd_bwd(logits_o, yo)
            tapes[g] = dict(tape=tape, params=params, logits=logits_o, loss=loss_o, correct=correct_o, dlogits=dlogits_o)
        first_pass = all(pc != per_chunk for _, pc in ck.samples)          # (the checks over every chunk: once per weight mode)
        ck.samples.append((list(smp), per_chunk))

        def inject(t, g, val):
            sl(t, g).copy_(val.permute(0, 2, 3, 1).to(dt))

        def put_mask(act, g, positive):
            eng._mask_of(act).view(G, -1)[g].copy_(_mask_bytes(positive, vec))

        def grad_of(g, name):
            return eng._unflatten(gout[g], name)

        def stats_all(L, tag):
            """per-chunk BN mean / variance of EVERY chunk of the group against float64 reductions (in pieces) of the engine's own conv output"""
            C, px = L.cout, chunk * L.hout * L.wout
            step = max(1, (1 << 27) // (px * C))
            wm = wv = -1.0
            gm = gv = 0
            for g0 in range(0, G, step):
                g1 = min(G, g0 + step)
                xv = L.x[g0 * chunk:g1 * chunk].reshape(g1 - g0, px, C).double()
                m, v = xv.mean(1), xv.var(1, unbiased=False)
                del xv
                me = eng.mean_tab[pidx, g0:g1, L.ch_off:L.ch_off + C].double()
                ve = eng.var_tab[pidx, g0:g1, L.ch_off:L.ch_off + C].double()
                em = ((me - m).abs() / (v + 1e-5).sqrt()).amax(1)          # (the error of the normalised activation it causes)
                ev = ((ve - v).abs() / (v + 1e-5)).amax(1)
                i, j = int(em.argmax()), int(ev.argmax())
                if float(em[i]) > wm:
                    wm, gm = float(em[i]), g0 + i
                if float(ev[j]) > wv:
                    wv, gv = float(ev[j]), g0 + j
            ck.worst(f"{tag} batch mean (all {G} chunks, / std)", wm, gm, STAT_TOL[dt])
            ck.worst(f"{tag} batch var (all {G} chunks, relative)", wv, gv, STAT_TOL[dt])

        def fwd_conv(L, src, rec_of, tag):
            """conv + batch statistics of layer L on the full group; sampled chunks: raw output and statistics against the oracle, then the oracle's own
            rounded raw output replaces the engine's (so that everything downstream of this layer starts from identical values)"""
            eng._conv_bn_fwd(L, src, G, wsets, theta, pidx)
            if first_pass:
                stats_all(L, tag)
            for g in smp:
                rec = rec_of(tapes[g]["tape"])
                raw = orc.conv_fwd(rec["x"], rec["w"], rec["stride"], rec["pad"])
                ck.close(sl(L.x, g), q(raw), f"{tag} conv output{sfx(g)}")
                mean, var = raw.mean(dim=(0, 2, 3)), raw.var(dim=(0, 2, 3), unbiased=False)
                ck.close_vec(eng.mean_tab[pidx, g, L.ch_off:L.ch_off + L.cout], mean, f"{tag} batch mean{sfx(g)}", 1e-4)
                ck.close_vec(eng.var_tab[pidx, g, L.ch_off:L.ch_off + L.cout], var, f"{tag} batch var{sfx(g)}", 1e-4)
                ck.close_vec(L.invstd[g], rec["bn"][1], f"{tag} invstd{sfx(g)}", 1e-4)
                inject(L.x, g, q(raw))

        def act_check(t, val_of, tag, mask=True):
            for g in smp:
                v = val_of(tapes[g]["tape"])
                ck.close(sl(t, g), v, f"{tag}{sfx(g)}")
                inject(t, g, v)
                if mask:
                    put_mask(t, g, v > 0)

        # -------------------------------------------------------------------------------------------------------- forward walk --
        fwd_conv(plan.stem, patches, lambda tp: tp[0]["rec"], "stem")
        eng._bn_apply(plan.stem, eng.stem_out, G)
        act_check(eng.stem_out, lambda tp: tp[0]["relu_out"] if plan.stem_pool else tp[0]["out"], "stem BN+ReLU")
        a_prev = eng.stem_out
        if plan.stem_pool:                       # MaxPool2d(3, 2, 1) of the ImageNet stem, remembering its argmax (reference resnets.py:74-79)
            s_ = plan.stem
            assert eng.stem_pool_idx is not None
            call("fb_maxpool3s2_fwd_idx", eng.stem_out.data_ptr(), eng.stem_pooled.data_ptr(), eng.stem_pool_idx.data_ptr(), n, s_.hout, s_.wout, 64, eng.dtc)
            for g in smp:
                ref = tapes[g]["tape"][0]["out"]
                ck.close(sl(eng.stem_pooled, g), ref, f"stem MaxPool2d(3,2,1){sfx(g)}")
                assert torch.equal(sl(eng.stem_pooled, g), _to_dev(ref, dt))          # (a selection: no rounding at all)
            a_prev = eng.stem_pooled
        for bi, b in enumerate(plan.blocks):
            tag = f"block {bi}"
            nxt = plan.blocks[bi + 1] if bi + 1 < len(plan.blocks) else None
            cur = a_prev
            for i, L in enumerate(b.convs[:-1]):
                fwd_conv(L, cur, lambda tp, i=i: tp[1 + bi]["recs"][i], f"{tag} conv{i + 1}")
                eng._bn_apply(L, b.mids[i], G)
                act_check(b.mids[i], lambda tp, i=i: tp[1 + bi]["mids"][i], f"{tag} BN{i + 1}+ReLU")
                cur = b.mids[i]
            last = b.convs[-1]
            fwd_conv(last, cur, lambda tp: tp[1 + bi]["recs"][-1], f"{tag} conv{len(b.convs)}")
            next_pool = nxt.pooled if nxt is not None else None
            if b.shortcut is not None:
                src = a_prev
                if b.pooled is not None:
                    # (the previous block's output pass wrote this pooled input in production; here the stand-alone kernel on the oracle's tensor)
                    call("fb_avgpool2_fwd", a_prev.data_ptr(), b.pooled.data_ptr(), n, b.hin, b.win, b.cin, eng.dtc)
                    act_check(b.pooled, lambda tp: tp[1 + bi]["rd"]["x"], f"{tag} AvgPool2d(2,2)", mask=False)
                    src = b.pooled
                fwd_conv(b.shortcut, src, lambda tp: tp[1 + bi]["rd"], f"{tag} shortcut conv")
                fused = eng._bn_apply(last, b.out, G, res=b.shortcut.x, resL=b.shortcut, pool=next_pool)
            else:
                fused = eng._bn_apply(last, b.out, G, res=a_prev, pool=next_pool)
            if fused:                              # the pooled copy of this output for the next block's shortcut, written by the same pass
                for g in smp:
                    ck.close(sl(nxt.pooled, g), q(orc.avgpool2_fwd(tapes[g]["tape"][1 + bi]["out"])), f"{tag} fused pooled output{sfx(g)}")
            act_check(b.out, lambda tp: tp[1 + bi]["out"], f"{tag} last BN + residual + ReLU")
            a_prev = b.out
        pstride = plan.P if per_chunk else 0
        call("fb_head_pool", a_prev.data_ptr(), eng.feat.data_ptr(), n, hw, plan.feat, eng.dtc)
        call("fb_head_loss", eng.feat.data_ptr(), theta.data_ptr() + 4 * plan.fcw_off, theta.data_ptr() + 4 * plan.fcb_off, pstride, y_dev.data_ptr(),
             eng.logits.data_ptr(), eng.dlogits.data_ptr(), eng.loss.data_ptr(), eng.correct.data_ptr(), G, chunk, plan.feat, plan.classes, 0.0, 0)
        for g in smp:
            t = tapes[g]
            ck.close_vec(sl(eng.logits, g), t["logits"], f"logits{sfx(g)}", 1e-5)
            ck.close_vec(sl(eng.dlogits, g), t["dlogits"], f"dlogits{sfx(g)}", 1e-5)
            if not (abs(float(eng.loss[g]) - float(t["loss"])) < 1e-5 * float(t["loss"]) and float(eng.correct[g]) == float(t["correct"])):
                ck.fails.append(f"loss / #correct of chunk {g}: {float(eng.loss[g])} / {float(eng.correct[g])} vs {float(t['loss'])} / {float(t['correct'])}")
        # the head of EVERY chunk against float64 on the engine's own features (once per weight mode)
        fcw = [(theta[g] if per_chunk else theta)[plan.fcw_off:plan.fcw_off + plan.classes * plan.feat].view(plan.classes, plan.feat).double() for g in range(G)]
        fcb = [(theta[g] if per_chunk else theta)[plan.fcb_off:plan.fcb_off + plan.classes].double() for g in range(G)]
        feat_e, dl_e = eng.feat[:n].double(), eng.dlogits[:n].double()
        wf = wl = wd = 0.0
        cf = cl = cd = 0
        for g in range(G) if first_pass else ():
            f64 = sl(a_prev, g).reshape(chunk, hw, plan.feat).double().mean(1)
            ef = float((sl(feat_e, g) - f64).norm() / f64.norm())
            lg = sl(feat_e, g) @ fcw[g].t() + fcb[g]
            loss64, correct64, dl64 = orc.cross_entropy_fwd_bwd(lg, sl(y_dev, g))
            el = max(float((sl(eng.logits, g).double() - lg).norm() / lg.norm()), abs(float(eng.loss[g]) - float(loss64)) / float(loss64),
                     0.0 if float(eng.correct[g]) == float(correct64) else 1.0)
            ed = float((sl(dl_e, g) - dl64).norm() / dl64.norm())
            wf, cf = (ef, g) if ef > wf else (wf, cf)
            wl, cl = (el, g) if el > wl else (wl, cl)
            wd, cd = (ed, g) if ed > wd else (wd, cd)
        if first_pass:
            hb = HEAD_F32 if fp32 else 1e-5
            ck.worst(f"head pooled features (all {G} chunks)", wf, cf, hb)
            ck.worst(f"logits, loss and #correct (all {G} chunks)", wl, cl, hb)
            ck.worst(f"dlogits (all {G} chunks)", wd, cd, hb)

        # ------------------------------------------------------------------------------------------------------- backward walk --
        d = eng.pool.get((n, plan.h_final, plan.h_final, plan.feat))
        call("fb_head_bwd", eng.feat.data_ptr(), eng.dlogits.data_ptr(), theta.data_ptr() + 4 * plan.fcw_off, pstride, gout.data_ptr() + 4 * plan.fcw_off,
             gout.data_ptr() + 4 * plan.fcb_off, plan.P, d.data_ptr(), G, chunk, hw, plan.feat, plan.classes, eng.dtc)
        wg = wi = 0.0
        cg = ci = 0
        for g in range(G) if first_pass else ():     # fc gradients and the head's input gradient of EVERY chunk against float64 on the engine's own dlogits / features
            gw64, gb64 = sl(dl_e, g).t() @ sl(feat_e, g), sl(dl_e, g).sum(0)
            eg = max(float((grad_of(g, "fc.weight").double() - gw64).norm() / gw64.norm()), float((grad_of(g, "fc.bias").double() - gb64).norm() / gb64.norm()))
            di = q((sl(dl_e, g) @ fcw[g]) / hw)                           # (stored in the compute dtype)
            ei = float((sl(d, g).reshape(chunk, hw, plan.feat).double() - di[:, None, :]).norm() / (di.norm() * hw ** 0.5))
            wg, cg = (eg, g) if eg > wg else (wg, cg)
            wi, ci = (ei, g) if ei > wi else (wi, ci)
        if first_pass:
            ck.worst(f"fc gradients (all {G} chunks)", wg, cg, HEAD_F32 if fp32 else 1e-4)
            ck.worst(f"head input gradient (all {G} chunks)", wi, ci, REL_L2_F32 if fp32 else REL_L2)
        da = {}
        for g in smp:
            t = tapes[g]
            head = t["tape"][-1]
            da[g] = q(((t["dlogits"] @ t["params"]["fc.weight"]) / head["spatial"])[:, :, None, None].expand(head["shape"]).contiguous())
            ck.close(sl(d, g), da[g], f"head input gradient{sfx(g)}")
            ck.close_vec(grad_of(g, "fc.weight"), t["dlogits"].t() @ head["feat"], f"fc.weight gradient{sfx(g)}", 1e-4)
            inject(d, g, da[g])

        def sync_wgrad():
            if eng.wstream is not None:
                torch.cuda.current_stream().wait_stream(eng.wstream)

        def bn_bwd_oracle(L, rec, dy_o, g, tag):
            dxc, dgam, dbet = orc.bn_train_bwd(dy_o, rec["gamma"], rec["bn"])
            ck.close_vec(gout[g, L.g_off:L.g_off + L.cout], dgam, f"{tag} dgamma{sfx(g)}", 2e-4)
            ck.close_vec(gout[g, L.b_off:L.b_off + L.cout], dbet, f"{tag} dbeta{sfx(g)}", 2e-4)
            return q(dxc)

        def wgrad(L, src, dx_e, rec_of, dxc, tag, bn=None):
            eng._wgrad(L, src, dx_e, G, gout, bn=bn)
            sync_wgrad()
            for g in smp:
                rec = rec_of(tapes[g]["tape"])
                _, dw = orc.conv_bwd(rec["x"], rec["w"], dxc[g], rec["stride"], rec["pad"], need_dx=False)
                ck.close_vec(grad_of(g, f"{L.conv_name}.weight"), dw, f"{tag} weight gradient{sfx(g)}", 1e-3)

        def bwd_layer(L, rec_of, d_e, mask_act, dy_of, src, tag, want_dy=False):
            """BN backward (reduce, finalize, apply -- with the ReLU bitmask of ``mask_act``) of the full group, then its weight gradient; sampled chunks
            against the oracle.  Returns (engine dx with the oracle's rounded dx injected, {chunk: oracle's rounded dx})."""
            dx_e, dy_e = eng._bn_bwd(L, d_e, mask_act, G, gout, pidx, want_dy=want_dy)
            dxc = {}
            for g in smp:
                dxc[g] = bn_bwd_oracle(L, rec_of(tapes[g]["tape"]), dy_of(g), g, tag)
                ck.close(sl(dx_e, g), dxc[g], f"{tag} BN backward dx{sfx(g)}")
                if want_dy:
                    ck.close(sl(dy_e, g), dy_of(g), f"{tag} masked gradient dy{sfx(g)}")
                inject(dx_e, g, dxc[g])
            wgrad(L, src, dx_e, rec_of, dxc, tag)
            return dx_e, dxc, dy_e

        def dgrad(L, dx_e, rec_of, dxc, tag, **kw):
            out = eng._dgrad(L, dx_e, G, wsets, **kw)
            ref = {g: torch.nn.grad.conv2d_input(rec_of(tapes[g]["tape"])["x"].shape, rec_of(tapes[g]["tape"])["w"], dxc[g],
                                                 rec_of(tapes[g]["tape"])["stride"], rec_of(tapes[g]["tape"])["pad"]) for g in smp}
            return out, ref

        stem_res = eng.stem_pooled if plan.stem_pool else eng.stem_out
        for bi in range(len(plan.blocks) - 1, -1, -1):
            b = plan.blocks[bi]
            tag = f"block {bi}"
            E = lambda tp: tp[1 + bi]                                       # noqa: E731
            first, last = b.convs[0], b.convs[-1]
            a0 = plan.blocks[bi - 1].out if bi > 0 else stem_res
            srcs = [a0] + b.mids
            dy_o = {g: q(da[g] * (E(tapes[g]["tape"])["out"] > 0)) for g in smp}
            out_bits = eng.masks.get(b.out.data_ptr())
            lazy = out_bits is not None and (b.shortcut is not None or eng._masked_addend_ok(first, G, wsets))
            nc = len(b.convs)
            dual = lazy and b.shortcut is not None and eng._bn_bwd2_ok(last, b.shortcut, G)
            dy_e = None
            if dual:                             # production: conv{nc}'s and the shortcut's BatchNorm backward in one pass over d
                dx_e, dxs_e = eng._bn_bwd2(last, b.shortcut, d, b.out, G, gout, pidx)
                dxc, dxcs = {}, {}
                for g in smp:
                    dxc[g] = bn_bwd_oracle(last, E(tapes[g]["tape"])["recs"][-1], dy_o[g], g, f"{tag} conv{nc}")
                    dxcs[g] = bn_bwd_oracle(b.shortcut, E(tapes[g]["tape"])["rd"], dy_o[g], g, f"{tag} shortcut")
                    ck.close(sl(dx_e, g), dxc[g], f"{tag} conv{nc} BN backward dx (dual pass){sfx(g)}")
                    ck.close(sl(dxs_e, g), dxcs[g], f"{tag} shortcut BN backward dx (dual pass){sfx(g)}")
                    inject(dx_e, g, dxc[g])
                    inject(dxs_e, g, dxcs[g])
                wgrad(last, srcs[-1], dx_e, lambda tp: E(tp)["recs"][-1], dxc, f"{tag} conv{nc}")
            else:
                dx_e, dxc, dy_e = bwd_layer(last, lambda tp: E(tp)["recs"][-1], d, b.out, lambda g: dy_o[g], srcs[-1], f"{tag} conv{nc}", want_dy=not lazy)
            for i in range(nc - 1, 0, -1):
                rec_i = lambda tp, i=i: E(tp)["recs"][i]                     # noqa: E731
                d_mid, ref = dgrad(b.convs[i], dx_e, rec_i, dxc, f"{tag} conv{i + 1}")
                d_mid_o = {}
                for g in smp:
                    d_mid_o[g] = q(ref[g])
                    ck.close(sl(d_mid, g), d_mid_o[g], f"{tag} conv{i + 1} input gradient{sfx(g)}")
                    inject(d_mid, g, d_mid_o[g])
                eng.pool.put(dx_e)
                dx_e, dxc, _ = bwd_layer(b.convs[i - 1], lambda tp, i=i: E(tp)["recs"][i - 1], d_mid, b.mids[i - 1],
                                         lambda g, i=i: q(d_mid_o[g] * (E(tapes[g]["tape"])["mids"][i - 1] > 0)), srcs[i - 1], f"{tag} conv{i}")
                eng.pool.put(d_mid)
            rec0 = lambda tp: E(tp)["recs"][0]                               # noqa: E731
            if b.shortcut is not None:
                S = b.shortcut
                rd = lambda tp: E(tp)["rd"]                                   # noqa: E731
                src = b.pooled if b.pooled is not None else a0
                if dual:
                    wgrad(S, src, dxs_e, rd, dxcs, f"{tag} shortcut")
                elif lazy:
                    dxs_e, dxcs, _ = bwd_layer(S, rd, d, b.out, lambda g: dy_o[g], src, f"{tag} shortcut")
                else:
                    dxs_e, dxcs, _ = bwd_layer(S, rd, dy_e, None, lambda g: dy_o[g], src, f"{tag} shortcut")
                d_p, ref = dgrad(S, dxs_e, rd, dxcs, f"{tag} shortcut")
                dp_o = {}
                for g in smp:
                    dp_o[g] = q(ref[g])
                    ck.close(sl(d_p, g), dp_o[g], f"{tag} shortcut input gradient{sfx(g)}")
                    inject(d_p, g, dp_o[g])
                eng.pool.put(dxs_e)
                d_in, ref = dgrad(first, dx_e, rec0, dxc, tag, addend=d_p, addend_mode=2 if b.pooled is not None else 1)
                d_o = {g: ref[g] + (orc.avgpool2_bwd(dp_o[g]) if b.stride == 2 else dp_o[g]) for g in smp}
                eng.pool.put(d_p)
                what = "conv1 dgrad + residual branch"
            elif lazy:
                d_in, ref = dgrad(first, dx_e, rec0, dxc, tag, addend=d, addend_mode=1, addend_mask=out_bits)
                d_o = {g: ref[g] + dy_o[g] for g in smp}
                what = "conv1 dgrad + residual branch, masked addend"
            else:
                d_in, ref = dgrad(first, dx_e, rec0, dxc, tag, addend=dy_e, addend_mode=1)
                d_o = {g: ref[g] + dy_o[g] for g in smp}
                what = "conv1 dgrad + residual branch"
            for g in smp:
                da[g] = q(d_o[g])
                ck.close(sl(d_in, g), da[g], f"{tag} input gradient ({what}){sfx(g)}")
                inject(d_in, g, da[g])
            eng.pool.put(dx_e, d)
            if dy_e is not None:
                eng.pool.put(dy_e)
            d = d_in
        S = plan.stem
        stem_e = lambda tp: tp[0]                                            # noqa: E731
        if plan.stem_pool:
            # MaxPool backward from the remembered argmax (the oracle scatters through torch's own indices of the same rounded tensor)
            d_r = eng.pool.get((n, S.hout, S.wout, 64))
            call("fb_maxpool3s2_bwd_idx", eng.stem_pool_idx.data_ptr(), d.data_ptr(), d_r.data_ptr(), n, S.hout, S.wout, 64, eng.dtc)
            for g in smp:
                r = tapes[g]["tape"][0]["relu_out"]
                dr = torch.zeros_like(r).flatten(2)
                dr.scatter_add_(2, tapes[g]["tape"][0]["pool_idx"].flatten(2), da[g].flatten(2))
                da[g] = q(dr.view_as(r))
                ck.close(sl(d_r, g), da[g], f"stem MaxPool backward{sfx(g)}")
                inject(d_r, g, da[g])
            eng.pool.put(d)
            d = d_r
        stem_act = {g: tapes[g]["tape"][0]["relu_out" if plan.stem_pool else "out"] for g in smp}
        dy_s = {g: q(da[g] * (stem_act[g] > 0)) for g in smp}
        dx_e, dxc, _ = bwd_layer(S, lambda tp: tp[0]["rec"], d, eng.stem_out, lambda g: dy_s[g], patches, "stem")
        eng.pool.put(dx_e)
        if eng._wgrad_bn_ok(S, eng.stem_out):
            # the production form of the stem's backward: no dx tensor -- the weight gradient applies the BatchNorm backward in its operand loader
            gout[:G, S.w_off:S.w_off + S.cout * S.taps * S.cin_real].zero_()
            eng._bn_bwd(S, d, eng.stem_out, G, gout, pidx, want_dy=False, apply=False)
            # (dx becomes an MFMA operand in the loader: the same rounding point as the stored dx)
            wgrad(S, patches, None, lambda tp: tp[0]["rec"], dxc, "stem (BatchNorm backward in the loader)", bn=(d, eng.stem_out))
        eng.pool.put(d)
        torch.cuda.synchronize()

    passes = [([0], False)] if passes is None else (passes(eng) if callable(passes) else passes)
    lib.profile_enable(True, 1 << 16)
    try:
        for smp, per_chunk in passes:
            assert per_chunk_sets or not per_chunk
            one_pass(smp, per_chunk)
        torch.cuda.synchronize()
        ck.launches = _launch_set(lib.profile_read_launches())
        lib.profile_read()
        # what a plain group_gradient of the same engine at the same group launches: the walk must have launched all of it
        want = set()
        for per_chunk in sorted({pc for _, pc in passes}):
            if per_chunk:
                eng.prep_weights(eng.theta_k, G, per_chunk=True)
                eng.group_gradient(patches, y_dev, G, eng.g_fd[0], 2, eng.theta_k, 1)
            else:
                eng.prep_weights(eng.theta, 1)
                eng.group_gradient(patches, y_dev, G, eng.g)
            torch.cuda.synchronize()
            want |= _launch_set(lib.profile_read_launches())
            lib.profile_read()
    finally:
        lib.profile_enable(False)
    missing = want - ck.launches

    worst = sorted(ck.report, key=lambda r: -r[1])[:8]
    kernels = sorted({lib.PROF_KERNELS.get(w[-1], str(w[-1])) for c, w in ck.launches if c in ("igemm_fwd", "igemm_dgrad", "wgrad")})
    print(f"resnet{depth} / {stem} stem / {pixels} px / {G} x {chunk} / {'fp32 ' + split if fp32 else 'bf16'}: sampled chunks {ck.samples}; "
          f"{len(ck.report)} tensors compared; largest relative L2 distances:")
    for what, rel, bad in worst:
        print(f"  {what}: {rel:.3e} ({bad:.1e} of the elements beyond 2 ulp)")
    if G > 1:
        print(f"  checks over all {G} chunks of the group, largest values (chunk):")
        for what, value, g in sorted(ck.stats, key=lambda r: -r[1])[:6]:
            print(f"    {what}: {value:.3e} (chunk {g})")
    print(f"  largest relative L2: tensors {ck.worst_tensor:.3e}, per-channel reductions {ck.worst_sum:.3e}")
    print(f"  {len(ck.launches)} distinct launches (class, shape, kernel), convolution kernels {kernels}; of group_gradient's {len(want)}: {len(missing)} not walked")
    if missing:
        ck.fails.append(f"launches of group_gradient the walk did not make: {sorted(missing)[:8]}")
    return ck


def test_resnet18_bf16_kernels_layer_by_layer_against_the_oracle():
    ck = _walk(18, "CIFAR", 32, 128)
    assert len(ck.report) > 180


@pytest.mark.parametrize("pixels,chunk", [(64, 32), (224, 128)])
def test_resnet50_bottleneck_bf16_kernels_layer_by_layer_against_the_oracle(pixels, chunk):
    """The Bottleneck path of bench.py's ResNet-152 lines (reference resnets.py:271-316, 'standard' stem :74-79), kernel by kernel: ResNet-50 has every layer shape
    of ResNet-152 (the deeper net repeats the identity blocks of stages 2 and 3).  At 224 px with one chunk of 128 images these are the production launches of
    BASELINE config 5's bf16 form: the 7x7 stem on 160-value patches and its 64 x 160 weight-gradient tile, MaxPool with a remembered argmax, streaming / pipelined
    1x1 kernels on 56 / 28 / 14 / 7 maps incl. the masked residual addend of the identity blocks, the all-taps 3x3 weight gradients on ImageNet-shaped maps, the
    1x1 weight-gradient GEMM, stride-2 3x3 layers, shortcuts with and without AvgPool; 64 px / chunks of 32: the shapes of the engine-level oracle tests."""
    ck = _walk(50, "standard", pixels, chunk)
    names = [r[0] for r in ck.report]
    assert sum("masked addend" in w for w in names) >= 10 and any("MaxPool backward" in w for w in names)
    assert len(ck.report) > 500


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# The same walk at the chunk groups the shipped configurations run.  Every launch covers the whole group of distinct chunks (the kernel a launch selects, the
# K-slice counts and the tiles a persistent workgroup walks across chunk boundaries all depend on the group size); the float64 oracle's tensors are injected
# into the slices of the sampled chunks only, and every launch's output is compared there.  The BatchNorm statistics and the head are checked on EVERY chunk.
def _auto(per_chunk=False):
    return lambda eng: [(_sampled_chunks(eng, eng.G), per_chunk)]


def _one_at_a_time(per_chunk=False):
    """224 px: one oracle tape (a chunk of 128 images in float64, ~20 GB) at a time -- a pass per sampled chunk"""
    return lambda eng: [([g], per_chunk) for g in _sampled_chunks(eng, eng.G)]


def _config3_group():
    """config 3's chunk group by the trainer's own rule (FullBatchTrainer: group_size of the whole problem, capped by max_group with one finite-difference set)"""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Plan, max_group
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.parallel import group_size

    torch.manual_seed(0)
    plan = Plan(construct_model(compose(["model=resnet18", "model.stem=CIFAR"]).model, 3, 10), 32)
    return group_size(N_CHUNKS_CIFAR, 98, cap=max_group(plan, 128, torch.float32, use_free=False, fd_sets=1))


@pytest.mark.parametrize("chunk,G", [(128, 98), (200, 84)], ids=["headline-128x98", "k250-200x84"])
def test_resnet18_bf16_walk_at_the_production_chunk_group(chunk, G, monkeypatch):
    """W1 / W2: the headline's group (98 chunks of 128) and configs.k250's (84 chunks of 200: its 64-channel tensors exceed 2^31 bytes, and 200 is not a multiple
    of the 16-image tile of the persistent halo kernel)."""
    ck = _walk(18, "CIFAR", 32, chunk, G=G, passes=_auto(), monkeypatch=monkeypatch)
    smp = ck.samples[0][0]
    assert {0, 1, G - 1} <= set(smp) and len(ck.report) > 180 * len(smp)
    if chunk == 200:                                 # the chunk that holds byte 2^31 of the 64-channel tensors
        assert (1 << 31) // (chunk * 32 * 32 * 64 * 2) in smp


@pytest.mark.parametrize("split", ["bf16x6", "f16x2"])
def test_resnet18_fp32_walk_at_config3_group(split, monkeypatch):
    """W3: fp32 storage at config 3's group, shared weights (the regulariser's base pass) and then one weight set per chunk (its second pass), the input images
    of every chunk scaled by a factor between 1e-3 and 1e3 so that the per-chunk fp16x2 scales differ."""
    G = _config3_group()
    assert 32 < G < 98
    scale = (10.0 ** np.linspace(-3, 3, G)).tolist()
    ck = _walk(18, "CIFAR", 32, 128, G=G, dtype=torch.float32, split=split, x_scale=scale, monkeypatch=monkeypatch, per_chunk_sets=True,
               passes=lambda eng: [(_sampled_chunks(eng, G), False), (_sampled_chunks(eng, G, seed=1), True)])
    assert len(ck.samples) == 2 and ck.samples[1][1]


def test_resnet50_bf16_walk_at_the_resnet152_group(monkeypatch):
    """W4: ResNet-50 ('standard' stem, 224 px) at ResNet-152's bf16 group of 16 chunks of 128 (chunk 10 holds byte 2^31 of the 64- and 256-channel tensors,
    the stem ranges start at chunks 0, 4, 8, 12)."""
    G = 16
    ck = _walk(50, "standard", 224, 128, G=G, monkeypatch=monkeypatch,
               passes=_one_at_a_time())
    assert any(10 in s for s, _ in ck.samples) and any(12 in s for s, _ in ck.samples)


def test_resnet50_fp32_walk_at_config5_group(monkeypatch):
    """W5: ResNet-50 ('standard' stem, 224 px) in fp32 (bf16x6) at config 5's group of 8 chunks of 128 with one weight set per chunk (the regulariser's second
    pass; chunk 5 holds byte 2^31 of the largest tensors, the stem ranges start at chunks 0, 2, 4, 6)."""
    G = 8
    ck = _walk(50, "standard", 224, 128, G=G, dtype=torch.float32, split="bf16x6", monkeypatch=monkeypatch, per_chunk_sets=True,
               passes=_one_at_a_time(per_chunk=True))
    assert any(5 in s for s, _ in ck.samples)
