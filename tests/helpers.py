"""Shared test helpers: synthetic data (same generator recipe as tests/golden/make_golden.py) and summaries."""
import numpy as np
import torch

SAMPLE_STRIDE = 997
NOISE_SEED = 4242      # tests/golden/make_golden.py seeds the default generator with it right before train() of the noise scenarios


def make_data(n, pixels=32, classes=10, seed=1234):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, pixels, pixels, generator=gen)
    y = torch.randint(0, classes, (n,), generator=gen)
    return x, y


def summarise(tensors):
    flat = torch.cat([t.detach().reshape(-1).double() for t in tensors])
    per = np.array([[float(t.double().sum()), float(t.double().pow(2).sum()), float(t.abs().max())] for t in tensors])
    return per, flat[::SAMPLE_STRIDE].numpy()


def hyp_from_cfg(cfg):
    """Flatten the cfg.hyp keys the oracle's step consumes."""
    o = cfg.hyp.optim
    return dict(lr=o.lr, weight_decay=o.weight_decay, momentum=o.momentum, nesterov=o.nesterov, dampening=o.dampening,
                block_strength=cfg.hyp.grad_reg.block_strength, eps=cfg.hyp.grad_reg.eps,
                implementation=cfg.hyp.grad_reg.implementation, grad_clip=cfg.hyp.grad_clip,
                acc_strength=cfg.hyp.grad_reg.acc_strength, optim_modification=dict(cfg.hyp.optim_modification),
                grad_clip_norm=cfg.hyp.grad_clip_norm, norm_bias=dict(cfg.hyp.norm_bias), evaluate_ema=cfg.hyp.evaluate_ema,
                eval_ema_momentum=cfg.hyp.eval_ema_momentum, test_time_flips=cfg.hyp.test_time_flips,
                only_linear_layers_weight_decay=cfg.hyp.only_linear_layers_weight_decay, label_smoothing=cfg.hyp.label_smoothing,
                loss_modification=cfg.hyp.loss_modification, grad_noise=dict(cfg.hyp.grad_noise), block=cfg.data.batch_size,
                batch_clip=cfg.hyp.batch_clip)


def torch_bf16_chunk_grads(model, x, y, chunk, device="cpu"):
    """The INDEPENDENT bf16 yardstick: torch's own ``autocast(bfloat16)`` evaluation of the same model on the same chunks -- the reference's
    ``_compute_batched_gradient`` under ``impl.mixed_precision`` (fullbatch/training/training.py:76-83: forward + CrossEntropyLoss inside
    autocast, ``torch.autograd.grad`` outside).  Plain torch: it touches neither ``libfbengine`` nor ``oracle/``.  Returns
    [(gradient list in ``model.parameters()`` order (fp32, host), loss)] per chunk."""
    import copy

    dev = torch.device(device)
    m = copy.deepcopy(model).to(dev).float().train()
    params = list(m.parameters())
    out = []
    for k in range(x.shape[0] // chunk):
        xb, yb = x[k * chunk:(k + 1) * chunk].to(dev), y[k * chunk:(k + 1) * chunk].to(dev)
        with torch.autocast(device_type=dev.type, dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(m(xb), yb)
        grads = torch.autograd.grad(loss, params)
        out.append(([g.detach().float().cpu() for g in grads], float(loss.detach())))
    return out


def flat64(tensors):
    return torch.cat([t.detach().reshape(-1).double().cpu() for t in tensors])


def err_cos(a, truth):
    """(relative L2 distance, cosine) of flat float64 vectors."""
    return float((a - truth).norm() / truth.norm()), float((a * truth).sum() / (a.norm() * truth.norm()))


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def shuffling_loaders(x, y, batch):
    """The loaders tests/golden/make_golden.py hands to the reference in the "shuffle" scenarios: RandomSampler train loader and a
    validation loader that share one generator seeded with 0."""
    ds = torch.utils.data.TensorDataset(x, y)
    own = torch.Generator().manual_seed(0)
    train = torch.utils.data.DataLoader(ds, batch_size=min(batch, len(ds)), shuffle=True, drop_last=True, generator=own)
    valid = torch.utils.data.DataLoader(ds, batch_size=min(batch, len(ds)), shuffle=False, drop_last=False, generator=own)
    return train, valid


def loader_pass_indices(loader):
    """Sample indices of one pass over ``loader`` in its order, consuming its generator exactly like ``for batch in loader`` does
    (torch DataLoader: the iterator draws a base seed first, then the sampler draws its permutation)."""
    torch.empty((), dtype=torch.int64).random_(generator=loader.generator)
    return torch.tensor([i for batch in loader.batch_sampler for i in batch], dtype=torch.long)


# ----------------------------------------------------------------------------------------------------------------------------------
# A dict-backed stand-in for the part of the third-party `lmdb` API the reference's LMDB dataset code uses (fullbatch/data/
# lmdb_datasets.py: open / begin / put / get / commit / cursor first-key-value-set_key-next).  tests/golden/make_golden.py --r2 hands it
# to the REFERENCE's writer and reader (the `lmdb` package is not installed in the build image); the tests rebuild a store from the
# committed key/value fixture.  Keys iterate in byte order, like LMDB's B+tree.
class DictLMDB:
    _stores = {}

    class _Cursor:
        def __init__(self, store):
            self.store, self.keys, self.pos = store, sorted(store), 0

        def first(self):
            self.pos = 0
            return bool(self.keys)

        def key(self):
            return self.keys[self.pos] if self.pos < len(self.keys) else b""

        def value(self):
            return self.store[self.keys[self.pos]] if self.pos < len(self.keys) else b""

        def set_key(self, key):
            import bisect
            i = bisect.bisect_left(self.keys, key)
            if i < len(self.keys) and self.keys[i] == key:
                self.pos = i
                return True
            return False

        def next(self):
            self.pos += 1
            return self.pos < len(self.keys)

    class _Txn:
        def __init__(self, store):
            self.store = store

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def put(self, key, value):
            self.store[bytes(key)] = bytes(value)
            return True

        def get(self, key, default=None):
            return self.store.get(bytes(key), default)

        def commit(self):
            pass

        def cursor(self):
            return DictLMDB._Cursor(self.store)

    def __init__(self, store=None):
        self.store = {} if store is None else store

    def begin(self, write=False, **kwargs):
        return DictLMDB._Txn(self.store)

    @classmethod
    def open(cls, path, **kwargs):
        return cls(cls._stores.setdefault(str(path), {}))


# ----------------------------------------------------------------------------------------------------------------------------------
PG_TIMEOUT_S = 120       # every process group of the tests: a collective that never completes fails after two minutes, not thirty


def pg_timeout():
    import datetime
    return datetime.timedelta(seconds=PG_TIMEOUT_S)


def spawn_bounded(fn, args, nprocs, timeout=150.0):
    """``torch.multiprocessing.spawn(fn, args, nprocs)`` with a wall-clock cap: the ranks are fresh `spawn` children (never a re-exec of a
    process that touched the GPU); the parent polls them, and when the cap passes it KILLS every child that is still alive and fails the
    calling test.  An exception in a rank surfaces as torch's ProcessRaisedException, as with ``join=True``."""
    import time

    import torch.multiprocessing as mp

    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + timeout
    try:
        while not ctx.join(timeout=2.0):
            if time.monotonic() > deadline:
                raise TimeoutError(f"{getattr(fn, '__name__', fn)} with {nprocs} rank(s) still running after {timeout:.0f} s: ranks killed")
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
        for proc in ctx.processes:
            proc.join(10)


# ----------------------------------------------------------------------------------------------------------------------------------
# Where the float64 oracle's tensors live in the `-m gpu` tests.  oracle/fb_oracle.py is a restatement in plain torch ops and does not
# care: on the host cores of a GPU box one float64 chunk gradient of ResNet-18 (128 images, 32 px) takes 29 s, with its tensors on the
# device 0.5 s, and the two agree to 2e-14 (tools/scratch/oracle_on_gpu.py; asserted by tests/test_gpu_engine.py::
# test_oracle_on_the_device_equals_the_oracle_on_the_host).  The convolutions then run in torch's own GPU kernels -- independent of
# libfbengine either way.  FB_ORACLE_DEVICE=cpu puts it back on the host; the `-m "not gpu"` tests always run it there.
def oracle_device():
    import os
    want = os.environ.get("FB_ORACLE_DEVICE", "cuda")
    return torch.device(want if (want == "cpu" or torch.cuda.is_available()) else "cpu")


def oracle_state(model, dtype=torch.float64, device=None):
    """(params, buffers) of the oracle from a parameter container, in ``dtype`` on the oracle's device."""
    from oracle import fb_oracle as orc
    device = oracle_device() if device is None else device
    state = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()).to(device) for k, v in model.state_dict().items()}
    return orc.split_state(state)


def to_oracle(*tensors, dtype=torch.float64):
    dev = oracle_device()
    out = tuple(t.to(dev, dtype) if t.is_floating_point() else t.to(dev) for t in tensors)
    return out[0] if len(out) == 1 else out


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 references of the update / regulariser kernels (csrc/multi_tensor.hip) with ELEMENTWISE error bounds that follow from the
# arithmetic: u = 2^-24 (one fp32 rounding, relative) times the sum of the absolute values of the terms of the expression times the
# number of roundings on the longest path.  Shared by tests/test_cpu_bounds.py (fp32 torch emulations of the kernels + planted errors:
# the checker is shown to bite) and tests/test_gpu_update_production.py (the kernels at arena size).  Every function works on tensors of
# any device, one row at a time, and takes the host-side scalars ROUNDED TO fp32 (`f32r`): they reach the kernels as `float`, and the
# scalar's own rounding (0.9f vs 0.9: 2.6e-8 relative) is larger than the bounds.
U32 = 2.0 ** -24
COEF_ROUNDINGS = 4       # clip / (sqrtf(norm2) + 1e-6f), eps / sqrtf(vnorm2): sqrt, add, divide + one of slack, relative


def f32r(x):
    """The value a Python float has once it is passed to a kernel as ``float``."""
    return float(np.float32(x))


def within_bound(got, ref, bound):
    """(worst |got - ref| / bound, flat index of it).  ``ref`` float64, ``bound`` a float64 tensor (or a number) >= 0; where the bound is 0
    the values must be equal (ratio 0 if they are, inf otherwise); a NaN anywhere counts as inf."""
    if got.numel() == 0:
        return 0.0, -1
    err = (got.double() - ref).abs().reshape(-1)
    b = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand(got.shape).reshape(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    i = int(torch.argmax(ratio))
    return float(ratio[i]), i


# ----------------------------------------------------------------------------------------------------------------------------------
# Elementwise bounds of the bf16 kernels that do the work (convolutions on the matrix pipe, BatchNorm apply / backward apply, pools): the
# float64 reference of the same operation on the same bf16 operands, and a bound per ELEMENT that follows from the arithmetic -- fp32
# accumulation of exact products, then ONE rounding to bf16 (to nearest even).  Shared by tests/test_cpu_ops_bounds.py (torch emulations +
# planted errors: the checker is shown to bite) and tests/test_gpu_ops_bounds.py (the kernels).
U_ACC = 2.0 ** -23       # one accumulation step of the matrix pipe: a WHOLE fp32 ulp, see mfma_sum_bound


def half_ulp_bf16(v):
    """Half a bf16 ulp in the binade of v >= 0: 2^(floor(log2(max(v, 2^-126))) - 8), float64, elementwise.  bf16 keeps 8 significand bits (one
    implicit + seven stored): the spacing of its values in [2^e, 2^(e+1)) is 2^(e-7), and round-to-nearest lands within half of that, 2^(e-8) --
    a unit roundoff of 2^-8.  Relative to the value itself half an ulp ranges from 2^-8 at the bottom of a binade down to 2^-9 at its top: the
    2^-9 quoted loosely elsewhere is that MINIMUM, not a bound (an honest fp32-accumulate, round-to-nearest-even emulation exceeds a 2^-9
    bound by 1.6 - 2.0 x).  floor(log2) is taken exactly, from the
    float64 exponent (frexp), not from a rounded logarithm.  Below the normal range (2^-126) the spacing stays that of the lowest binade."""
    v = torch.as_tensor(v, dtype=torch.float64).clamp_min(2.0 ** -126)
    _, e = torch.frexp(v)                                  # v = m 2^e with m in [0.5, 1): floor(log2 v) = e - 1
    return torch.exp2((e - 9).double())


def mfma_sum_bound(A, K):
    """|fp32 sum of K exact products - their exact sum| <= (K + 1) U_ACC A, with A the sum of the products' absolute values (the same float64
    convolution applied to |x| and |w|).  A product of two bf16 values has 16 significand bits: exact in fp32.  Every accumulation step adds
    to a partial sum of magnitude <= A (1 + small) and loses at most one fp32 ulp of it, U_ACC = 2^-23 relative -- a whole ulp, not half:
    fullbatchtraining_amd/csrc/common.h records at mma_split6 (measured by tools/mfma_accum_probe.hip) that the matrix pipe TRUNCATES small addends against a large
    accumulator.  K products take at most K additions however they are ordered, blocked into 32-deep instructions or split across waves
    (a tree over K leaves has K - 1 inner nodes; one more for a zero-started accumulator); + 1 absorbs the second-order terms.  So the bound
    holds for every tile shape and K-split and carries no constant fitted to a kernel.  What it can see: with K <= 576 it stays below half a
    bf16 ulp of a typical output, and one-ulp errors (truncation, a second rounding, a value off by one ulp) exceed the total; at K >= 2048
    the accumulation term dominates the rounding term and such errors are no longer seen -- errors of the size of one missing product
    (a dropped tap, a wrong row, exchanged channels) still are, at every K."""
    return (int(K) + 1) * U_ACC * A


def rounded_to_bf16_bound(ref, E):
    """Bound on |stored - ref| for a value stored with ONE round-to-nearest-even to bf16 when E bounds |fp32 value before rounding - ref|:
    half_ulp_bf16(|ref| + E) + E.  The fp32 value lies within E of ref, so its magnitude is at most |ref| + E and the rounding moves it by at
    most half an ulp of that magnitude's binade; a value that rounds UP into the next binade (to the power of two itself) moved by at most
    half an ulp of the binade it came from."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    E = torch.as_tensor(E, dtype=torch.float64, device=ref.device)
    return half_ulp_bf16(ref.abs() + E) + E


def block_stat_bounds(r, E, block=128):
    """Per-(block, channel) sums and sums of squares of the fp32 accumulators of a convolution (fb_conv2d's stat_partial) against float64.
    ``r`` [M, C] float64 reference in pixel order, ``E`` [M, C] the bound on each accumulator (mfma_sum_bound); the last block is partly
    filled when M % block != 0.  -> (sum, bound_sum, sumsq, bound_sumsq), each [ceil(M / block), C].  Each accumulator a_p is within E_p of
    r_p: that alone moves the sum by sum E_p and the sum of squares by sum (2 |r_p| E_p + E_p^2).  Adding ``block`` fp32 values of
    magnitude <= |r_p| + E_p in any order takes block - 1 additions, each within 2^-24 of a partial sum that is at most sum (|r_p| + E_p):
    block 2^-24 sum (|r_p| + E_p); the squares carry one rounding more (the product, or none where it is fused): block + 1."""
    M, C = r.shape
    nblk = -(-M // block)
    pad = nblk * block - M

    def blocks(t):
        if pad:
            t = torch.cat([t, torch.zeros(pad, C, dtype=t.dtype, device=t.device)])
        return t.view(nblk, block, C).sum(1)

    mag = r.abs() + E
    s, q = blocks(r), blocks(r * r)
    bs = blocks(E) + block * U32 * blocks(mag)
    bq = blocks(2 * r.abs() * E + E * E) + (block + 1) * U32 * blocks(mag * mag)
    return s, bs, q, bq


def bn_apply_ref(x, scale, shift, res=None, rscale=None, rshift=None):
    """fb_bn_apply before ReLU and rounding, float64: v = x scale + shift (+ res | + res rscale + rshift), all operands already broadcast to
    x's shape -> (v, e) with e = 5 * 2^-24 (|x scale| + |shift| + |res rscale| + |rshift|): at most five fp32 roundings on the path (two
    products, three sums; fewer where the compiler fuses), each relative to a partial result no larger than the sum of the terms'
    magnitudes."""
    x = x.double()
    v = x * scale.double() + shift.double()
    mag = (x * scale.double()).abs() + shift.double().abs()
    if res is not None:
        t = res.double() * rscale.double() if rscale is not None else res.double()
        v = v + t
        mag = mag + t.abs()
        if rshift is not None:
            v = v + rshift.double()
            mag = mag + rshift.double().abs()
    return v, 5 * U32 * mag


def bn_mask_check(bits, v, e, out=None, relu=False):
    """The ReLU mask bit of fb_bn_apply (1 = the fp32 value is > 0) against the float64 value ``v`` with its bound ``e``: the bit must equal
    v > 0 wherever |v| > e; inside that band the fp32 value may have either sign and either bit is accepted.  Where the bit is set and ReLU
    is on, the stored output must not be negative.  -> (number of wrong bits outside the band, share of elements inside the band, number
    of negative outputs under a set bit)."""
    bits = bits.bool()
    band = v.abs() <= e
    wrong = (bits != (v > 0)) & ~band
    neg = int((bits & (out.double() < 0)).sum()) if (relu and out is not None) else 0
    return int(wrong.sum()), float(band.double().mean()), neg


def padding_exact_zero(t, real):
    """True if every element of the padding images of ``t`` ([n, ...], ``real`` [n] bool: the images that are not padding) is EXACTLY zero --
    all bits clear, so a -0 or a denormal fails: fb_bn_apply writes the padding pixels of a ragged statistics group, their mask bytes and
    their pooled output as zero bits.  Works on bf16 / fp32 values, mask bytes and booleans."""
    pad = t[~real].contiguous()
    if pad.numel() == 0:
        return True
    if pad.dtype == torch.bool:
        return not bool(pad.any())
    if pad.is_floating_point():
        pad = pad.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[pad.element_size()])
    return int((pad != 0).sum()) == 0


def bn_dx_ref(coef_dy, coef_x, coef_0, dy, x):
    """fb_bn_dx (fullbatchtraining_amd/csrc/common.h): dx = fma(c_dy, dy, fma(c_x, x, c_0)) -> (reference, E) with E = 2 * 2^-24 (|c_dy dy| + |c_x x| + |c_0|): two
    fused multiply-adds, one rounding each, of partial results no larger than the sum of the three terms' magnitudes."""
    a, b, c = coef_dy.double() * dy.double(), coef_x.double() * x.double(), coef_0.double()
    return a + b + c, 2 * U32 * (a.abs() + b.abs() + c.abs())


def bn_case(C, hw, ipg, groups, valid, seed=4):
    """Inputs of the BatchNorm bound tests for the shape (channels, map size, images per group, groups, real images per group), NCHW fp32
    tensors holding bf16-exact values: x (padding images [valid, ipg) of every group exact zeros, as the engine stores them), res, dout,
    and per-group gamma, beta, rscale, rshift [groups, C] (fp32)."""
    gen = torch.Generator().manual_seed(seed + C + hw)
    n = ipg * groups
    x = (torch.randn(n, C, hw, hw, generator=gen) * 1.5 + 0.3).bfloat16().float()
    res = torch.randn(n, C, hw, hw, generator=gen).bfloat16().float()
    dout = torch.randn(n, C, hw, hw, generator=gen).bfloat16().float()
    gamma, beta = torch.rand(groups, C, generator=gen) + 0.5, torch.randn(groups, C, generator=gen) * 0.1
    rscale, rshift = torch.rand(groups, C, generator=gen) + 0.5, torch.randn(groups, C, generator=gen) * 0.3
    real = (torch.arange(n) % ipg) < valid
    x[~real] = 0
    return dict(x=x, res=res, dout=dout, gamma=gamma, beta=beta, rscale=rscale, rshift=rshift, real=real)


def running_mean_ref(a0, rows, counter0):
    """The running mean a_{j+1} = a_j + (v_j - a_j) / (c + j + 1) of fb_mt_accumulate (and of the mean inside fb_mt_fd_combine_accumulate) as a
    float64 recurrence, with the bound B carried alongside: B += u * (3 |v_j - a_j| / (c+j+1) + |a_{j+1}|) per folded chunk (the subtraction, the
    product and the fp32 rounding of 1/(c+j+1); the sum).  An earlier error is multiplied by 1 - 1/(c+j+1) <= 1, so the terms add up.
    ``rows`` yields v_j, or (v_j, e_j) where e_j bounds the error v_j itself arrives with (the recombined gradient): B += e_j / (c+j+1).
    -> (mean, B, sum of the v_j), all float64."""
    a = a0.double().clone()
    B, total = torch.zeros_like(a), torch.zeros_like(a)
    for j, v in enumerate(rows):
        v, e = v if isinstance(v, tuple) else (v, None)
        v = v.double()
        inv = 1.0 / (counter0 + j + 1)
        total += v
        d = v - a
        a += d * inv
        B += d.abs_() * (3 * U32 * inv)
        B += a.abs() * U32
        if e is not None:
            B += e * inv
    return a, B, total


def reduction_bound(count, blocks, r, extra=0.0):
    """Relative error of a two-stage sum of non-negative terms: fp32 partials per thread (``r`` roundings per iteration, ``count`` iterations
    spread over ``blocks`` workgroups of 256 threads), a 16-deep fp32 tree inside the workgroup, the second stage in double."""
    iters = -(-int(count) // (int(blocks) * 256))
    return (r * iters + 16) * U32 + extra


def clip_coef_ref(norm2, clip):
    """(coef, hit) of the clip the kernels form from the device scalar ``norm2`` (an fp32 value): norm > clip -> clip / (norm + 1e-6).  The
    kernels form it in fp32: COEF_ROUNDINGS * u relative is allowed wherever it enters."""
    if clip is None or clip < 0:
        return 1.0, False
    norm, c = float(np.sqrt(np.float64(np.float32(norm2)))), f32r(clip)
    if not norm > c:
        return 1.0, False
    return c / (norm + f32r(1e-6)), True


def sgd_ref(p, g, m, coef, hit, lr, weight_decay, momentum, dampening, nesterov, first):
    """fb_mt_clip_sgd in float64 -> {"grad" | "mom" | "param": (reference, bound)}.  With S = |coef g| + wd |p| + mu |m|:
    clipped gradient u |coef g| (+ the allowance on coef; not clipped: the bits of g), momentum 4u S, parameters u (|p| + |p'| + 8 lr S);
    where the clip is hit the allowance on coef (COEF_ROUNDINGS u |coef g|) passes linearly into the momentum (factor <= 1) and the
    parameters (factor <= lr (1 + mu))."""
    lr, wd, mu, damp = f32r(lr), f32r(weight_decay), f32r(momentum), f32r(dampening)
    p, g = p.double(), g.double()
    cg = g * coef
    ce = COEF_ROUNDINGS * U32 * cg.abs() if hit else torch.zeros_like(cg)
    d = cg + wd * p
    S = cg.abs() + wd * p.abs()
    out = {"grad": (cg, U32 * cg.abs() + ce if hit else torch.zeros_like(cg))}
    if mu != 0.0:
        if first:
            buf = d
        else:
            buf = mu * m.double() + (1.0 - damp) * d
            S = S + mu * m.double().abs()
        out["mom"] = (buf, 4 * U32 * S + ce)
        d = d + mu * buf if nesterov else buf
    pn = p - lr * d
    out["param"] = (pn, U32 * (p.abs() + pn.abs() + 8 * lr * S) + lr * (1 + mu) * ce)
    return out


def fd_combine_ref(g, ga, gb, eps_j, cf):
    """gt = g + cf (ga - gb) / eps_j (fb_mt_fd_combine, and per chunk inside fb_mt_fd_combine_accumulate): (gt, u (3 cf |ga - gb| / eps_j + |gt|)) --
    the difference, the quotient and the product are amplified by cf / eps_j, the sum is not.  ``eps_j``: the fp32 value the kernel reads."""
    cf = f32r(cf)
    amp = (ga.double() - gb.double()) * (cf / float(eps_j))
    gt = g.double() + amp
    return gt, U32 * (3 * amp.abs_() + gt.abs())


def fd_perturb_ref(theta0, g, s, alpha, pre=None, acc=0.0):
    """theta0 + alpha (s g + acc pre) of fb_mt_fd_perturb (alpha = sign * eps_n[j] in float64):
    (out, u (|theta0| + 3 |alpha| (|s g| + |acc pre|) + |out|))."""
    s, acc = f32r(s), f32r(acc)
    w = s * g.double()
    mag = w.abs()
    if pre is not None:
        q = acc * pre.double()
        w = w + q
        mag = mag + q.abs()
    out = theta0.double() + alpha * w
    return out, U32 * (theta0.double().abs() + 3 * abs(alpha) * mag + out.abs())


def scale_ref(x, a):
    """fb_mt_scale / the clip-free product: ONE correctly rounded fp32 product: (a x, u |a x|)."""
    out = f32r(a) * x.double()
    return out, U32 * out.abs()


def sam_ref(theta, g, norm2, clip, rho):
    """fb_mt_sam_ascent as the reference states it (sam.py:56-69 after the closure's clip): g_c = coef g, e = g_c rho / (|g_c| + 1e-12) with
    |g_c| the float64 norm OF THE CLIPPED VECTOR (the kernel forms it as sqrt(norm2) * coef), theta' = theta + e.
    -> {"e": ..., "theta": ...}.  e: the two products, sqrt, product, add, divide of the scale, one for norm2's own fp32 rounding: 7u |e|, and
    twice the allowance on coef where the clip is hit; theta': that + u |theta'|."""
    coef, hit = clip_coef_ref(norm2, clip)
    gc = g.double() * coef
    norm_c = float(gc.pow(2).sum().sqrt())
    e = gc * (f32r(rho) / (norm_c + f32r(1e-12)))
    be = (7 + (2 * COEF_ROUNDINGS if hit else 0)) * U32 * e.abs()
    tn = theta.double() + e
    return {"e": (e, be), "theta": (tn, be + U32 * tn.abs()), "norm_c": norm_c, "coef": coef, "hit": hit}


def norm_bias_ref(grad, theta, pnorm2, strength, bias, norm_type):
    """fb_mt_norm_bias: diff = pnorm2 - bias^2; type 1: grad + strength sign(diff) (one rounding); else grad + 2 strength diff theta, where
    c = 2 strength diff carries u (2 |2 strength| (pnorm2 + bias^2) + |c|) (bias^2, the difference; the product) and the update one rounding
    for c theta and one for the sum."""
    strength, bias, pn2 = f32r(strength), f32r(bias), float(np.float32(pnorm2))
    diff = pn2 - bias * bias
    g, t = grad.double(), theta.double()
    if norm_type == 1:
        out = g + strength * (1.0 if diff > 0 else (-1.0 if diff < 0 else 0.0))
        return out, U32 * out.abs()
    c = strength * 2.0 * diff
    c_err = U32 * (2 * abs(2 * strength) * (pn2 + bias * bias) + abs(c))
    out = g + c * t
    return out, c_err * t.abs() + U32 * ((c * t).abs() + out.abs())


SENTINEL = 1.2345e30     # fills the padding columns between a row's n values and the group stride: no kernel may touch them


def distinct_rows(G, n, stride, scale, seed, device, bands=True):
    """[G, stride] fp32 test rows: seeded randn * scale; a band of 1000 columns scaled by 1e3 and another by 1e-3; row j multiplied by 1 + j/G
    (a row mix-up changes every result); the padding columns [n, stride) hold SENTINEL."""
    gen = torch.Generator(device=device).manual_seed(seed)
    buf = torch.empty(G, stride, device=device, dtype=torch.float32)
    buf.normal_(generator=gen).mul_(scale)
    if bands and n > 8000:
        buf[:, 5000:6000] *= 1e3
        buf[:, n // 2:n // 2 + 1000] *= 1e-3
    buf *= (1.0 + torch.arange(G, device=device, dtype=torch.float32) / G)[:, None]
    buf[:, n:] = SENTINEL
    return buf


def padding_untouched(buf, n):
    return bool((buf[..., n:] == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# BatchNorm running statistics and evaluation coefficients (csrc/bn.hip bn_running_update_kernel, csrc/head_pool.hip bn_eval_coeffs_kernel)
# as float64 references with elementwise bounds from the arithmetic.  Shared by tests/test_cpu_bounds.py (fp32 emulations + planted errors),
# tests/test_gpu_running_stats.py and tests/test_gpu_eval.py.
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def bessel(valid_images, hout, wout):
    """m / (m - 1) with m = real images of a BN batch x pixels of the feature map, as the fp32 value the kernel multiplies by."""
    m = int(valid_images) * int(hout) * int(wout)
    return f32r(m / (m - 1))


def bn_running_ref(rm0, rv0, updates, momentum=BN_MOMENTUM):
    """Running mean / variance after ``updates`` = [(batch mean row, BIASED batch variance row, Bessel factor: number or per-channel tensor)]
    applied in that order: r <- keep r + mom x with keep = fl(1 - fl(mom)) (the kernel forms it in fp32; the scalars through ``f32r``), x the
    mean, or the variance times the Bessel factor.  -> (mean, var, bound_mean, bound_var), float64.  Bound per update: three roundings (the two
    products, the sum): B <- keep B + u (|keep r| + |mom x| + |r'|); the variance one more for var * ub: + u |mom x|.  An earlier error is
    multiplied by keep < 1, so the terms add up."""
    mom = f32r(momentum)
    keep = float(np.float32(1.0) - np.float32(momentum))
    m, v = rm0.double().clone(), rv0.double().clone()
    Bm, Bv = torch.zeros_like(m), torch.zeros_like(v)
    for mean, var, ub in updates:
        ub = ub.double().to(m.device) if torch.is_tensor(ub) else float(ub)
        xm, xv = mom * mean.double().to(m.device), mom * (var.double().to(m.device) * ub)
        m_new, v_new = keep * m + xm, keep * v + xv
        Bm = keep * Bm + U32 * ((keep * m).abs() + xm.abs() + m_new.abs())
        Bv = keep * Bv + U32 * ((keep * v).abs() + 2 * xv.abs() + v_new.abs())
        m, v = m_new, v_new
    return m, v, Bm, Bv


def bn_eval_coeffs_ref(gamma, beta, rm, rv, eps=BN_EPS):
    """scale = gamma / sqrt(rv + eps), shift = beta - rm scale (BatchNorm2d in eval mode) -> (scale, shift, bound_scale, bound_shift), float64.
    The kernel: the sum rv + eps, sqrtf, the reciprocal, the product: 4u |scale|; the shift: the product rm * scale (carrying scale's error)
    and the difference: u (5 |rm scale| + |shift|)."""
    g, b, m, v = gamma.double(), beta.double(), rm.double(), rv.double()
    scale = g / (v + f32r(eps)).sqrt()
    shift = b - m * scale
    return scale, shift, 4 * U32 * scale.abs(), U32 * (5 * (m * scale).abs() + shift.abs())


def mean_loss_bound(n, classes, logits64, labels):
    """Bound on |fp32 mean cross entropy - float64 mean cross entropy| of the SAME logits (fb_head_loss: a thread per image, then one sequential
    fp32 sum over the n images and a division; in the style of ``reduction_bound``): per image l = lse - (z_t - max), with z - max (one rounding),
    ``classes`` exponentials (2 ulp each) and their sequential sum (relative (classes + 2) u of a sum in [1, classes]), logf (2 ulp), the
    difference: u (2 |z_t - max| + (classes + 2) + 3 lse + l); the sum of n non-negative terms: (n - 1) u relative, the division one more."""
    z = logits64.double()
    zm = z - z.max(dim=1, keepdim=True).values
    lse = zm.exp().sum(dim=1).log()
    zt = zm[torch.arange(z.shape[0], device=z.device), labels]
    li = lse - zt
    per_image = U32 * (2 * zt.abs() + (classes + 2) + 3 * lse + li)
    return float(per_image.mean() + n * U32 * li.mean())


def eval_state(model, spec, x, seed=11, stat_images=32):
    """Parameters and running statistics under which evaluation is NOT degenerate (at the init state gamma = 1, beta = 0, running statistics
    (0, 1) make every BatchNorm the identity), written into ``model`` (the parameter container) in place:
      * gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1) in every BatchNorm;
      * running mean / (unbiased) variance = the float64 oracle's train-mode batch statistics of ``x[:stat_images]``;
      * in every layer two channels on the epsilon path: ``running_var`` exactly 0 in one and exactly 1e-6 in the other.  So that these
        channels leave their BatchNorm with O(1) values -- gamma / sqrt(eps) = 316 gamma on an O(1) channel in each of 20 .. 53 layers compounds
        to an overflow -- the rows of the convolution weight that produce them are scaled by 1e-4 and 1e-3 first: the channels' true variance is
        then ~1e-8 and ~1e-6, the recorded one 0 and 1e-6, and eps decides the result (without it: inf, and a factor 3.3).
    -> {bn name: (channel with running_var 0, channel with running_var 1e-6)}."""
    from oracle import fb_oracle as orc

    gen = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    names = spec.bn_names()
    conv_of = {bn: (bn[:-1] + "0" if bn == "stem.1" else (bn.replace(".downsample.2", ".downsample.1") if "downsample" in bn else bn.replace(".bn", ".conv")))
               for bn in names}
    eps_ch = {}
    with torch.no_grad():
        for li, bn in enumerate(names):
            C = sd[f"{bn}.weight"].numel()
            sd[f"{bn}.weight"].copy_(0.5 + torch.rand(C, generator=gen))
            sd[f"{bn}.bias"].copy_(0.1 * torch.randn(C, generator=gen))
            c0, c1 = 1 + li % 5, C - 2 - li % 3
            eps_ch[bn] = (c0, c1)
            w = sd[f"{conv_of[bn]}.weight"]
            w[c0] *= 1e-4
            w[c1] *= 1e-3
        state = {k: (v.detach().clone().double() if v.is_floating_point() else v.detach().clone()).to(oracle_device()) for k, v in sd.items()}
        params, buffers = orc.split_state(state)
        for bn in names:                      # (running statistics (0, 0) + one update with momentum 0.1: the buffers hold 0.1 x the batch statistics)
            buffers[f"{bn}.running_mean"].zero_()
            buffers[f"{bn}.running_var"].zero_()
        orc.forward(spec, params, buffers, to_oracle(x[:stat_images]), update_bn=True, train=True)
        for bn in names:
            c0, c1 = eps_ch[bn]
            rv = (buffers[f"{bn}.running_var"] / orc.BN_MOMENTUM).float().cpu()
            rv[c0], rv[c1] = 0.0, 1e-6
            sd[f"{bn}.running_mean"].copy_((buffers[f"{bn}.running_mean"] / orc.BN_MOMENTUM).float().cpu())
            sd[f"{bn}.running_var"].copy_(rv)
    return eps_ch


# ----------------------------------------------------------------------------------------------------------------------------------
# Confinement: a launch may read its inputs and write its outputs, and nothing else.  ``confined`` carves every operand out of the middle of a
# byte slab of its own, runs the launch once per fill byte with the guard bands (and the outputs' prior content) filled with that byte, and
# holds the launch to four properties: reads confined (same output bits whatever surrounds the operands), outputs fully defined (same bits
# whatever the outputs held before; finite), writes confined (guards and stride gaps still hold the fill), inputs unchanged.  Works on
# tensors of any device: tests/test_cpu_confinement.py plants each error in plain torch functions, tests/test_gpu_confinement.py runs the kernels.
GUARD_BYTES = 256 * 4096 * 4      # the largest tile any kernel stages at the shapes of the tests: 256 pixels x 4096 channels x 4 B = 4 MiB, so
                                  # a prefetch of one whole tile past an operand's end still lands in the guard (derived, not measured)
FILLS = (0x00, 0xFF, 0x7F)        # 0xFF..: NaN in bf16 and fp32, -1 as a label or index; 0x7F..: a huge finite value (3.4e38) in both.  Both
                                  # are needed: fmaxf(NaN, 0) hides a stray NaN, it does not hide a stray 3e38


class ConfinementError(AssertionError):
    pass


class Strided:
    """An operand of ``rows`` rows of ``width`` elements, ``stride`` elements apart (a slab of the [g][P] gradient arena, columns of a
    statistics table, parameter rows): carved as ONE slab; the gaps between the rows are filled and checked like guards.  ``data``
    ([rows, width]) for inputs and inout operands.  The launch receives a [rows, width] view with strides (stride, 1)."""

    def __init__(self, rows, width, stride, dtype=torch.float32, data=None):
        assert stride >= width and rows >= 1
        self.rows, self.width, self.stride, self.dtype, self.data = int(rows), int(width), int(stride), dtype, data


class _Slab:
    def __init__(self, name, spec, device, guard):
        self.name, self.guard = name, guard
        if isinstance(spec, Strided):
            self.dtype, self.data = spec.dtype, spec.data
            self.shape, self.stride = (spec.rows, spec.width), spec.stride
            n_el = (spec.rows - 1) * spec.stride + spec.width
        else:
            if torch.is_tensor(spec):
                self.dtype, self.data, self.shape = spec.dtype, spec, tuple(spec.shape)
            else:
                shape, self.dtype = spec
                self.data, self.shape = None, tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
            self.stride = None
            n_el = 1
            for s in self.shape:
                n_el *= s
        self.item = torch.empty((), dtype=self.dtype).element_size()
        self.nbytes = n_el * self.item
        self.buf = torch.empty(guard + self.nbytes + guard, dtype=torch.uint8, device=device)
        mid = self.buf[guard:guard + self.nbytes].view(self.dtype)
        if self.stride is None:
            self.view, self.gap = mid.view(self.shape), None
        else:
            self.view = torch.as_strided(mid, self.shape, (self.stride, 1))
            gap = torch.ones(n_el, dtype=torch.bool, device=device)
            torch.as_strided(gap, self.shape, (self.stride, 1)).fill_(False)
            self.gap = gap.repeat_interleave(self.item) if gap.any() else None
        if self.data is not None:
            self.data = self.data.detach().to(device=device, dtype=self.dtype).reshape(self.shape).contiguous()

    def arm(self, guard_fill, content_fill):
        g = self.guard
        self.buf[:g].fill_(guard_fill)
        self.buf[g + self.nbytes:].fill_(guard_fill)
        self.buf[g:g + self.nbytes].fill_(guard_fill if self.gap is not None else content_fill)
        if self.gap is not None and self.data is None:
            rows, width = self.shape
            torch.as_strided(self.buf[g:g + self.nbytes], (rows, width * self.item), (self.stride * self.item, 1)).fill_(content_fill)
        if self.data is not None:
            self.view.copy_(self.data)

    def bytes_now(self):
        return self.view.contiguous().reshape(-1).view(torch.uint8).clone()

    def touched(self, fill):
        """None, or where a byte outside the operand no longer holds ``fill``."""
        g = self.guard
        for what, part, base in (("the guard before it", self.buf[:g], -g), ("the guard behind it", self.buf[g + self.nbytes:], self.nbytes)):
            bad = part != fill
            if bool(bad.any()):
                first = int(bad.nonzero()[0])
                return f"{what} (byte {base + first:+d} relative to the operand's first byte, {int(bad.sum())} bytes in all)"
        if self.gap is not None:
            bad = (self.buf[g:g + self.nbytes] != fill) & self.gap
            if bool(bad.any()):
                first = int(bad.nonzero()[0])
                return (f"the gap between its rows (byte {first} = row {first // (self.stride * self.item)}, element "
                        f"{first % (self.stride * self.item) // self.item} of the stride; {int(bad.sum())} bytes in all)")
        return None


def confined(fn, inputs, outputs, inout=(), device="cuda", scratch=(), fills=FILLS, guard=GUARD_BYTES):
    """Run ``fn(ops)`` once per fill byte with every operand carved out of its own slab and assert that the launch is confined to its operands.

    ``inputs``: {name: tensor | Strided(data=...)}; ``outputs``: {name: (shape, dtype) | Strided}; ``inout``: {name: tensor | Strided(data=...)} --
    accumulators, counters and workspaces that must hold defined content at launch: restored before every run, only their surroundings are filled;
    ``scratch``: {name: (shape, dtype)} -- workspaces whose content after the launch means nothing (filled like an output before it, not compared).
    ``fn`` gets {name: view on ``device``} and must leave the work finished or on the current stream.  Returns {name: result of the FIRST run} for
    the outputs and inout operands (clones)."""
    inputs, outputs, inout, scratch = dict(inputs), dict(outputs), dict(inout), dict(scratch)
    slabs = {}
    for group in (inputs, outputs, inout, scratch):
        for name, spec in group.items():
            assert name not in slabs, f"operand name {name!r} used twice"
            slabs[name] = _Slab(name, spec, device, guard)
    for name in list(inputs) + list(inout):
        assert slabs[name].data is not None, f"{name!r} needs content"
    results = list(outputs) + list(inout)
    is_cuda = torch.device(device).type == "cuda"

    def run(guard_fill, content_fill):
        for s in slabs.values():
            s.arm(guard_fill, content_fill)
        fn({name: s.view for name, s in slabs.items()})
        if is_cuda:
            torch.cuda.synchronize()
        return {name: slabs[name].bytes_now() for name in results}

    def where(a, b, s):
        i = int((a != b).nonzero()[0]) // s.item
        return i, int((a != b).view(-1, s.item).any(1).sum())

    first, first_fill = None, None
    for fill in fills:
        got = run(fill, fill)
        for name, s in slabs.items():                                           # writes confined
            hit = s.touched(fill)
            if hit is not None:
                raise ConfinementError(f"writes confined: the launch wrote outside operand {name!r}: {hit}; fill 0x{fill:02X}")
        for name in inputs:                                                     # inputs unchanged
            s = slabs[name]
            now, want = s.bytes_now(), s.data.reshape(-1).view(torch.uint8)
            if not torch.equal(now, want):
                i, cnt = where(now, want, s)
                raise ConfinementError(f"inputs unchanged: the launch modified input {name!r} (element {i}, {cnt} elements in all); fill 0x{fill:02X}")
        if first is None:
            first, first_fill = got, fill
            continue
        for name in results:
            if torch.equal(got[name], first[name]):
                continue
            s = slabs[name]
            i, cnt = where(got[name], first[name], s)
            stale = all(bool((r[name][i * s.item:(i + 1) * s.item] == f).all()) for r, f in ((first, first_fill), (got, fill)))
            if name in outputs and stale:
                raise ConfinementError(f"outputs fully defined: element {i} of output {name!r} is never written ({cnt} elements differ between "
                                       f"fill 0x{first_fill:02X} and fill 0x{fill:02X}; it still holds the fill)")
            # which memory does the result depend on: what surrounds the operands, or what the outputs held before?  The surroundings of the first run,
            # the prior content of this one
            probe = run(first_fill, fill)
            if torch.equal(probe[name], first[name]):
                raise ConfinementError(f"reads confined: {name!r} depends on memory outside the operands: element {i} ({cnt} elements in all) differs "
                                       f"between fill 0x{first_fill:02X} and fill 0x{fill:02X} of the guards")
            raise ConfinementError(f"outputs fully defined: {name!r} depends on what the outputs held before the launch (read-modify-write): element {i} "
                                   f"({cnt} elements in all) differs between fill 0x{first_fill:02X} and fill 0x{fill:02X}")
    out = {}
    for name in results:
        s = slabs[name]
        t = first[name].view(s.dtype).view(s.shape)
        if t.is_floating_point() and not bool(torch.isfinite(t.float()).all()):
            i = int((~torch.isfinite(t.float().reshape(-1))).nonzero()[0])
            raise ConfinementError(f"outputs fully defined: {name!r} is not finite (element {i})")
        out[name] = t
    return out
