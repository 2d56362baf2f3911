"""BatchNorm running statistics of EVERY layer after ``Engine.full_gradient`` -- what evaluation later normalises with.

(a) The recurrence.  With one chunk group (``n_chunks <= G``) the per-chunk statistics tables ``mean_tab`` / ``var_tab`` survive the call, and
``running_mean`` / ``running_var`` of all channels must equal the float64 recurrence r <- 0.9 r + 0.1 x over ``mean_tab[p, g]`` and
``var_tab[p, g] * m / (m - 1)`` in chunk-major, pass-minor order, within ``helpers.bn_running_ref``'s arithmetic bound (three roundings per update,
one more for the Bessel product).  m = real images x pixels is computed here, not read from the engine's table.  Every case starts from random running
statistics (mean ~ N(0, 1), var ~ U(0.5, 1.5)): from (0, 1) a lost or doubled update of the mean would be invisible against the decay (1 - m)^K.
Modes: plain, forward differences (2 passes), central differences (3), the ``acc_strength`` pre-pass over blocks of two chunks (its own Bessel factor,
before the main loop's updates; its tables are read in the ``after_pre_pass`` hook), a padded chunk (30 real images stored as 32) and a sub-range
``chunk_ids``.  Several groups are covered by composition: the walk (tests/test_gpu_bf16_structural.py) checks every chunk's table entries against
float64 reductions at production group sizes, and test_gpu_engine.py::test_chunk_group_beyond_2g_byte_tensors_equals_smaller_groups pins the
running statistics bit-equal across group sizes.
ResNet-50 runs with chunks of 32 images: at 64 px its last maps are 2 x 2, and a stored chunk must fill whole 128-pixel statistics blocks.

(b) fp32 against the float64 oracle, all layers, 7 chunks in groups of 3 + 3 + 1, plain and forward differences (the oracle's buffers see the
regulariser's second forward).  Per layer the maximum over channels of |d mean| / sqrt(var + eps) and |d var| / (var + eps) (the normalisation of the
walk's STAT_TOL) must stay within 5 x what plain torch fp32 gets on the same chunks (plain: the parameter container in train mode; forward
differences: the oracle's restatement evaluated in fp32), but not below STAT_TOL[float32] = 1e-5.

Measured (MI355X).  (a) worst error / bound over all cases: mean 0.571, var 0.486 (after the pre-pass alone: 0.558 / 0.478).  (b) worst layer, engine | torch fp32,
(mean, var): ResNet-18 plain layers.2.0.downsample.2 1.03e-6, 3.06e-7 | 3.72e-7, 3.21e-7; ResNet-18 forward differences layers.3.1.bn1 5.19e-7, 1.81e-6 | 2.83e-6, 2.92e-6;
ResNet-50 plain layers.3.2.bn1 9.87e-7, 4.01e-6 | 2.48e-6, 1.33e-5.
"""
import pytest
import torch

from tests.helpers import bessel, bn_running_ref, make_data, oracle_state, to_oracle, within_bound

pytestmark = pytest.mark.gpu

NETS = {"r18": (18, "CIFAR", 32, 32), "r50": (50, "standard", 64, 32)}      # depth, stem, pixels, stored chunk


def _model(net, seed=0, stats_seed=21):
    """the parameter container with RANDOM running statistics (and a non-zero num_batches_tracked)"""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model

    depth, stem, pixels, chunk = NETS[net]
    cfg = compose([f"model=resnet{depth}", f"model.stem={stem}"])
    torch.manual_seed(seed)
    model = construct_model(cfg.model, 3, 10)
    gen = torch.Generator().manual_seed(stats_seed)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=gen))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=gen))
            elif name.endswith("num_batches_tracked"):
                buf.fill_(5)
    return model, depth, stem, pixels, chunk


def _padded_feed(eng, x, y, valid, chunk):
    """stem patches / labels of chunks of ``valid`` real images stored as ``chunk`` rows (zero images, label -1), as FullBatchTrainer feeds them"""
    from fullbatchtraining_amd.engine import stem_patches

    dense = stem_patches(x.cuda(), eng.plan.stem, eng.dt)
    if valid == chunk:
        return dense, y.cuda()
    k = x.shape[0] // valid
    patches = torch.zeros(k * chunk, *dense.shape[1:], device="cuda", dtype=eng.dt)
    patches.view(k, chunk, *dense.shape[1:])[:, :valid].copy_(dense.view(k, valid, *dense.shape[1:]))
    labels = torch.full((k, chunk), -1, dtype=torch.long, device="cuda")
    labels[:, :valid] = y.cuda().view(k, valid)
    return patches, labels.reshape(-1)


MODES = {
    # name: (passes per chunk, fd_sets, full_gradient keywords, chunks fed, chunk_ids, real images per chunk or None)
    "plain": (1, 0, {}, 3, None, None),
    "forward": (2, 1, dict(block_strength=0.5, implementation="forward-differences"), 3, None, None),
    "central": (3, 2, dict(block_strength=0.5, implementation="central-differences"), 2, None, None),
    "acc_pre_block": (2, 1, dict(block_strength=0.5, acc_strength=0.5, implementation="forward-differences"), 4, None, None),
    "padded": (1, 0, {}, 3, None, 30),
    "chunk_ids": (1, 0, {}, 4, range(1, 3), None),
}


@pytest.mark.parametrize("net,dtype,mode", [("r18", torch.bfloat16, "plain"), ("r18", torch.bfloat16, "padded"), ("r18", torch.bfloat16, "chunk_ids"),
                                            ("r18", torch.float32, "plain"), ("r18", torch.float32, "forward"), ("r18", torch.float32, "central"),
                                            ("r18", torch.float32, "acc_pre_block"), ("r18", torch.float32, "padded"), ("r18", torch.float32, "chunk_ids"),
                                            ("r50", torch.bfloat16, "plain"), ("r50", torch.bfloat16, "padded"), ("r50", torch.float32, "forward"),
                                            ("r50", torch.float32, "acc_pre_block")],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_running_statistics_follow_the_recurrence_over_the_engines_tables(net, dtype, mode):
    from fullbatchtraining_amd.engine import Engine, Plan, padded_chunk

    n_passes, fd_sets, kw, n_fed, chunk_ids, valid = MODES[mode]
    model, depth, stem, pixels, chunk = _model(net)
    if valid is not None:
        assert padded_chunk(Plan(model, pixels), valid) == chunk
    valid = chunk if valid is None else valid
    G = 4
    eng = Engine(model, pixels, chunk, G, compute_dtype=dtype, fd_sets=fd_sets, chunk_valid=valid)
    x, y = make_data(n_fed * valid, pixels)
    patches, labels = _padded_feed(eng, x, y, valid, chunk)
    rm0, rv0, nbt0 = eng.running_mean.clone(), eng.running_var.clone(), eng.num_batches_tracked
    assert nbt0 == 5 and float(rm0.abs().max()) > 1.0
    ids = list(range(n_fed)) if chunk_ids is None else list(chunk_ids)
    assert len(ids) <= G
    plan = eng.plan

    def ub_row(images):
        """Bessel factors of every channel for BN batches of ``images`` real images: m / (m - 1), m = images x H x W of the channel's layer"""
        row = torch.empty(plan.ch_total, dtype=torch.float64)
        for L in plan.layers:
            row[L.ch_off:L.ch_off + L.cout] = bessel(images, L.hout, L.wout)
        return row.cuda()

    updates, pre = [], {}
    if mode == "acc_pre_block":
        def hook():                              # the pre-pass is complete: its tables (one row per block of two chunks) are still there
            torch.cuda.synchronize()
            pre["mean"], pre["var"], pre["rm"], pre["rv"] = eng.mean_tab[0].clone(), eng.var_tab[0].clone(), eng.running_mean.clone(), eng.running_var.clone()
        kw = dict(kw, pre_block=2 * chunk, after_pre_pass=hook)
    eng.full_gradient(patches, labels, 0.1, eps=1e-2, chunk_ids=None if chunk_ids is None else ids, **kw)
    torch.cuda.synchronize()
    expected_updates = len(ids) * n_passes
    if mode == "acc_pre_block":
        n_blocks = len(ids) // 2
        ub2 = ub_row(2 * chunk)
        updates += [(pre["mean"][b], pre["var"][b], ub2) for b in range(n_blocks)]
        expected_updates += n_blocks
        # the pre-pass on its own first (its updates come BEFORE the main loop's)
        rm, rv, Bm, Bv = bn_running_ref(rm0, rv0, updates)
        a, b = within_bound(pre["rm"], rm, Bm)[0], within_bound(pre["rv"], rv, Bv)[0]
        print(f"  after the pre-pass ({n_blocks} blocks of {2 * chunk} images): error / bound mean {a:.3f}, var {b:.3f}")
        assert a <= 1.0 and b <= 1.0
    ub = ub_row(valid)
    updates += [(eng.mean_tab[p, g], eng.var_tab[p, g], ub) for g in range(len(ids)) for p in range(n_passes)]
    rm, rv, Bm, Bv = bn_running_ref(rm0, rv0, updates)
    a, ia = within_bound(eng.running_mean, rm, Bm)
    b, ib = within_bound(eng.running_var, rv, Bv)
    decay = 0.9 ** expected_updates
    print(f"{net} {dtype} {mode}: {expected_updates} updates of {plan.ch_total} channels; error / bound mean {a:.3f} (channel {ia}), var {b:.3f} (channel {ib}); "
          f"start value still weighs {decay:.3f}")
    assert a <= 1.0 and b <= 1.0
    assert eng.num_batches_tracked == nbt0 + expected_updates
    # the tables are real statistics (not left-over zeros), and a wrong Bessel factor would have been seen: it moves the variance by more than the bound
    assert float(eng.var_tab[:n_passes, :len(ids)].min()) > 0
    wrong = bn_running_ref(rm0, rv0, [(m, v, ub_row(chunk + 2)) for m, v, _ in updates])[1]
    assert float(((wrong - rv).abs() / Bv).max()) > 1.0


STAT_TOL_F32 = 1e-5          # tests/test_gpu_bf16_structural.STAT_TOL[torch.float32]


@pytest.mark.parametrize("net,mode", [("r18", "plain"), ("r18", "forward"), ("r50", "plain")])
def test_fp32_running_statistics_of_all_layers_vs_the_oracle_over_several_groups(net, mode):
    """(b) of the module docstring: 7 chunks, groups of 3 + 3 + 1."""
    import copy

    from fullbatchtraining_amd.engine import Engine, stem_patches
    from oracle import fb_oracle as orc
    from tests.test_gpu_bf16_structural import STAT_TOL

    assert STAT_TOL[torch.float32] == STAT_TOL_F32
    model, depth, stem, pixels, chunk = _model(net)
    n_chunks, G, lr = 7, 3, 0.1
    fd = mode == "forward"
    eng = Engine(model, pixels, chunk, G, compute_dtype=torch.float32, fd_sets=1 if fd else 0)
    x, y = make_data(n_chunks * chunk, pixels)
    hyp = dict(weight_decay=0.0, block_strength=0.5 if fd else 0.0, eps=1e-2, implementation="forward-differences", grad_clip=None)
    spec = orc.Spec(depth, stem=stem)
    from collections import defaultdict

    def oracle_buffers(dtype):
        params, buffers = oracle_state(model, dtype)
        xo, yo = to_oracle(x, y, dtype=dtype)
        orc._gradient_evaluation(spec, params, buffers, xo, yo, hyp, lr, defaultdict(list), chunk)
        return buffers

    ref = oracle_buffers(torch.float64)
    if fd:
        yard = oracle_buffers(torch.float32)
    else:                                            # the parameter container itself, train mode, plain torch fp32
        m = copy.deepcopy(model).cuda().float().train()
        with torch.no_grad():
            for k in range(n_chunks):
                m(x[k * chunk:(k + 1) * chunk].cuda())
        yard = dict(m.named_buffers())
    eng.full_gradient(stem_patches(x.cuda(), eng.plan.stem, torch.float32), y.cuda(), lr, hyp["block_strength"], hyp["eps"], hyp["implementation"])
    torch.cuda.synchronize()
    passes = 2 if fd else 1
    assert eng.num_batches_tracked == 5 + n_chunks * passes == int(ref["stem.1.num_batches_tracked"])
    worst, fails = (0.0, 0.0, "", 0.0, 0.0), []
    print(f"{net} fp32 {mode}: per layer max over channels, engine | torch fp32  (|d mean| / std, |d var| / var)")
    for L in eng.plan.layers:
        r_m, r_v = ref[f"{L.bn_name}.running_mean"].double().cuda(), ref[f"{L.bn_name}.running_var"].double().cuda()
        std, var = (r_v + 1e-5).sqrt(), r_v + 1e-5
        e_m = float(((eng.running_mean[L.ch_off:L.ch_off + L.cout].double() - r_m).abs() / std).max())
        e_v = float(((eng.running_var[L.ch_off:L.ch_off + L.cout].double() - r_v).abs() / var).max())
        y_m = float(((yard[f"{L.bn_name}.running_mean"].double().cuda() - r_m).abs() / std).max())
        y_v = float(((yard[f"{L.bn_name}.running_var"].double().cuda() - r_v).abs() / var).max())
        print(f"  {L.bn_name:28s} mean {e_m:.2e} | {y_m:.2e}   var {e_v:.2e} | {y_v:.2e}")
        if max(e_m, e_v) > max(worst[0], worst[1]):
            worst = (e_m, e_v, L.bn_name, y_m, y_v)
        if not e_m <= max(5 * y_m, STAT_TOL_F32):
            fails.append(f"{L.bn_name} running_mean {e_m:.3e} (torch fp32 {y_m:.3e})")
        if not e_v <= max(5 * y_v, STAT_TOL_F32):
            fails.append(f"{L.bn_name} running_var {e_v:.3e} (torch fp32 {y_v:.3e})")
    print(f"  worst layer {worst[2]}: engine {worst[0]:.2e} / {worst[1]:.2e}, torch fp32 {worst[3]:.2e} / {worst[4]:.2e}")
    assert not fails, fails
