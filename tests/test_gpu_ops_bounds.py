"""The bf16 kernels that do the work -- convolutions forward (with BatchNorm partial statistics) and input gradient (with every addend
mode), BatchNorm finalize / apply / backward, the pools, the head's input gradient, the shortcut sampling -- against float64 references of
the same operation on the same bf16 operands, ELEMENT BY ELEMENT: every assertion is ``within_bound(got, ref, bound)[0] <= 1.0`` over all
elements with a bound derived from the arithmetic (tests/helpers.py: half_ulp_bf16, mfma_sum_bound, rounded_to_bf16_bound, block_stat_bounds,
bn_apply_ref, bn_dx_ref); no allowed fraction, no norm.  tests/test_cpu_ops_bounds.py shows on the CPU that these bounds pass an honest
emulation and reject one wrong element, truncation, a second rounding, a pixel in the wrong statistics block.  Set FB_BOUNDS_REPORT to a file
name to have every worst ratio appended to it (profiles/ops_bounds.md is written from such a run)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import (U32, block_stat_bounds, bn_apply_ref, bn_case, bn_dx_ref, bn_mask_check, mfma_sum_bound, padding_exact_zero,
                           rounded_to_bf16_bound, to_oracle, within_bound)
from tests.test_gpu_ops import CONV_DGRAD_CASES, CONV_FWD_CASES, krsc, nhwc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BN_EPS = 1e-5
U1 = U32 * (1 + 2.0 ** -20)          # one fp32 rounding of a value that was computed in double (the finalize kernels): the double's own error rides on top


def _lib():
    from fullbatchtraining_amd import lib
    return lib


def _report(family, what, ratio):
    path = os.environ.get("FB_BOUNDS_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(f"{family}\t{what}\t{ratio:.4f}\n")


def hold(family, what, got, ref, bound, dims=("image", "y", "x", "channel")):
    """Assert that every element of ``got`` is within ``bound`` of ``ref``; on failure name the flat index, its coordinates and the ratio."""
    ratio, i = within_bound(got, ref, bound)
    print(f"{family}: {what}: worst |got - ref| / bound = {ratio:.4f}")
    _report(family, what, ratio)
    if ratio <= 1.0:
        return
    coords, rest = [], i
    for size in reversed(got.shape):
        coords.append(rest % size)
        rest //= size
    names = dims if len(dims) == len(coords) else tuple(f"dim {j}" for j in range(len(coords)))
    at = ", ".join(f"{d} {c}" for d, c in zip(names, reversed(coords)))
    b = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand(got.shape).reshape(-1)[i]
    raise AssertionError(f"{family}: {what}: flat index {i} ({at}): got {float(got.reshape(-1)[i])!r}, reference {float(ref.reshape(-1)[i])!r}, "
                         f"bound {float(b):.3e}, ratio {ratio:.3f}")


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
# convolutions
@pytest.mark.parametrize("cin,cout,k,stride,hw,n", CONV_FWD_CASES)
def test_conv_fwd_and_block_statistics_elementwise(cin, cout, k, stride, hw, n):
    """fb_conv2d(mode 0, stat_partial) at every bf16 shape of test_conv_fwd_and_stats.  Output: one rounding of an fp32 sum of K = cin k k
    exact products.  Statistics: per 128-pixel block and channel, sums of the fp32 ACCUMULATORS (include/fb_engine.h), hence against the
    float64 sums of the reference r itself, not of the rounded output -- block by block, so that a pixel counted in the neighbouring block
    is seen (the sum over blocks is blind to it).  The float64 reference of the two largest tuples takes well under a second on the device:
    it is computed for every image."""
    lib = _lib()
    torch.manual_seed(0)
    pad = k // 2
    x = torch.randn(n, cin, hw, hw).to(BF)
    w = (torch.randn(cout, cin, k, k) * 0.1).to(BF)
    xd, wd = nhwc(x).cuda(), krsc(w).cuda()
    x64, w64 = to_oracle(x.float(), w.float())
    r = F.conv2d(x64, w64, None, stride, pad)
    A = F.conv2d(x64.abs(), w64.abs(), None, stride, pad)
    ho = r.shape[2]
    r, A = (t.permute(0, 2, 3, 1).contiguous() for t in (r, A))
    out = torch.empty(n, ho, ho, cout, dtype=BF, device="cuda")
    M = n * ho * ho
    nblk = (M + 127) // 128
    stat = torch.zeros(2, nblk, cout, device="cuda")
    lib.conv2d(xd, wd, out, k, k, stride, pad, 0, stat_partial=stat)
    torch.cuda.synchronize()
    E = mfma_sum_bound(A, cin * k * k)
    dev = r.device
    hold("conv forward", f"output {(cin, cout, k, stride, hw, n)}", out.to(dev), r, rounded_to_bf16_bound(r, E))
    s, bs, q, bq = block_stat_bounds(r.view(M, cout), E.view(M, cout))
    hold("conv forward", f"block sums {(cin, cout, k, stride, hw, n)}", stat[0].to(dev), s, bs, dims=("block", "channel"))
    hold("conv forward", f"block sums of squares {(cin, cout, k, stride, hw, n)}", stat[1].to(dev), q, bq, dims=("block", "channel"))


@pytest.mark.parametrize("cin,cout,k,stride,hw,n,amode", CONV_DGRAD_CASES)
def test_conv_dgrad_elementwise(cin, cout, k, stride, hw, n, amode):
    """fb_conv2d(mode 1) at every bf16 shape of test_conv_dgrad with its addend mode.  r = conv (+ a | + 0.25 a upsampled); the addend enters
    in fp32 BEFORE the single rounding (every epilogue: the implicit GEMMs, the halo kernels, the stride-2 quad kernel, the 1x1 streaming
    kernels), so the value before rounding is within E = mfma_sum_bound(A, cout k k) + 2 * 2^-24 (|conv| + |a|) of r (the product 0.25 a is
    exact; the sum rounds once, one more for a fused form) and the stored one within rounded_to_bf16_bound(r, E).  No kernel gets a second
    half-ulp term."""
    lib = _lib()
    torch.manual_seed(1)
    pad = k // 2
    ho = (hw + 2 * pad - k) // stride + 1
    w = (torch.randn(cout, cin, k, k) * 0.1).to(BF)
    dy = torch.randn(n, cout, ho, ho).to(BF)
    w64, dy64 = to_oracle(w.float(), dy.float())
    conv = torch.nn.grad.conv2d_input((n, cin, hw, hw), w64, dy64, stride, pad)
    A = torch.nn.grad.conv2d_input((n, cin, hw, hw), w64.abs(), dy64.abs(), stride, pad)
    add_d, a64 = None, torch.zeros_like(conv)
    if amode == 1:
        addend = torch.randn(n, cin, hw, hw).to(BF)
        a64 = to_oracle(addend.float())
        add_d = nhwc(addend).cuda()
    elif amode == 2:
        addend = torch.randn(n, cin, hw // 2, hw // 2).to(BF)
        a64 = 0.25 * to_oracle(addend.float()).repeat_interleave(2, 2).repeat_interleave(2, 3)
        add_d = nhwc(addend).cuda()
    r = conv + a64
    E = mfma_sum_bound(A, cout * k * k) + 2 * U32 * (conv.abs() + a64.abs())
    wt = w.permute(1, 2, 3, 0).reshape(cin, k * k, cout).contiguous().cuda()
    out = torch.empty(n, hw, hw, cin, dtype=BF, device="cuda")
    lib.conv2d(nhwc(dy).cuda(), wt, out, k, k, stride, pad, 1, addend=add_d, addend_mode=amode)
    torch.cuda.synchronize()
    r, E = (t.permute(0, 2, 3, 1).contiguous() for t in (r, E))
    hold("conv input gradient", f"addend mode {amode} {(cin, cout, k, stride, hw, n)}", out.to(r.device), r, rounded_to_bf16_bound(r, E))


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm.  (C, hw, images per group, groups, real images per group): each reaches one form of fb_bn_apply
BN_GRID, BN_SPAN_PADDED, BN_SPAN_PADDED3, BN_POOL = (96, 4, 8, 2, 8), (64, 8, 8, 2, 5), (512, 4, 16, 3, 13), (256, 8, 4, 2, 3)
BN_SHAPES = [BN_GRID,            # 12 channel vectors per pixel do not divide 256: grid-stride form
             BN_SPAN_PADDED,     # span form, padded group
             BN_SPAN_PADDED3,    # span form, padded, three groups
             BN_POOL]            # W * C = 2048: pooling form with pool_out, padded
CH_OFF, CH_PAD = 32, 96          # the statistics tables are wider than the layer: its columns start at CH_OFF


def _rep(tab, ipg):
    """[groups, C] per-group coefficients -> [n, 1, 1, C] per image (NHWC broadcast)."""
    return tab.repeat_interleave(ipg, 0)[:, None, None, :]


@functools.lru_cache(maxsize=None)
def bn_state(shape):
    """Inputs on the device, the fp32 partial statistics a convolution epilogue would hand over (built on the host: the convolution test
    checks the real ones), and the tables fb_bn_fwd_finalize makes of them."""
    lib = _lib()
    C, hw, ipg, groups, valid = shape
    case = bn_case(*shape)
    n, ppg = ipg * groups, ipg * hw * hw
    px = n * hw * hw
    xn = nhwc(case["x"]).reshape(px, C)
    nblk = px // 128
    part = torch.stack([xn.view(nblk, 128, C).sum(1), (xn * xn).view(nblk, 128, C).sum(1)]).cuda()
    count = valid * hw * hw
    pg = torch.zeros(groups, 2 * C + 64)
    pg[:, :C], pg[:, C:2 * C] = case["gamma"], case["beta"]
    pgd = pg.cuda()
    mean_tab = torch.zeros(groups, C + CH_PAD, device="cuda")
    var_tab = torch.zeros_like(mean_tab)
    scale, shift, invstd = (torch.zeros(groups, C, device="cuda") for _ in range(3))
    lib.call("fb_bn_fwd_finalize", part.data_ptr(), nblk, groups, C, float(count), pgd.data_ptr(), pgd.data_ptr() + 4 * C, pg.shape[1], BN_EPS,
             mean_tab.data_ptr(), var_tab.data_ptr(), C + CH_PAD, CH_OFF, scale.data_ptr(), shift.data_ptr(), invstd.data_ptr())
    torch.cuda.synchronize()
    dev = {key: nhwc(case[key]).to(BF).cuda() for key in ("x", "res", "dout")}
    return dict(case=case, part=part, count=count, n=n, px=px, ppg=ppg, mean_tab=mean_tab, var_tab=var_tab, scale=scale, shift=shift, invstd=invstd,
                rscale=case["rscale"].cuda(), rshift=case["rshift"].cuda(), real=case["real"].cuda(), **dev)


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_fwd_finalize_tables_elementwise(shape):
    """fb_bn_fwd_finalize: the kernel adds the fp32 partials in double and rounds each table entry to fp32 once, so against the float64
    evaluation of the SAME partials: mean and variance one rounding (the variance also the double's own error on q / m and mean^2, which
    cancel), invstd one, scale = gamma * fl(invstd) two, shift = beta - fl(mean) * scale five (as bn_eval_coeffs_ref).  The count is the
    number of REAL pixels of a padded group."""
    C, hw, ipg, groups, valid = shape
    st = bn_state(shape)
    part = st["part"].double().view(2, groups, -1, C).sum(2)
    mean = part[0] / st["count"]
    ex2 = part[1] / st["count"]
    var = (ex2 - mean * mean).clamp_min(0)
    invstd = 1.0 / (var + BN_EPS).sqrt()
    gamma, beta = st["case"]["gamma"].cuda().double(), st["case"]["beta"].cuda().double()
    scale = gamma * invstd
    shift = beta - mean * scale
    fam, cols = "BatchNorm finalize", slice(CH_OFF, CH_OFF + C)
    hold(fam, f"mean {shape}", st["mean_tab"][:, cols], mean, U1 * mean.abs(), dims=("group", "channel"))
    hold(fam, f"variance {shape}", st["var_tab"][:, cols], var, U1 * var + 2.0 ** -50 * (ex2 + mean * mean), dims=("group", "channel"))
    # invstd inherits the variance's double-precision cancellation error: d invstd = invstd^3 / 2 d var
    hold(fam, f"invstd {shape}", st["invstd"], invstd, U1 * invstd + 0.5 * invstd ** 3 * 2.0 ** -50 * (ex2 + mean * mean), dims=("group", "channel"))
    hold(fam, f"scale {shape}", st["scale"], scale, 2 * U1 * scale.abs() + gamma.abs() * 0.5 * invstd ** 3 * 2.0 ** -50 * (ex2 + mean * mean), dims=("group", "channel"))
    hold(fam, f"shift {shape}", st["shift"], shift, U1 * (5 * (mean * scale).abs() + shift.abs()), dims=("group", "channel"))
    assert float(st["mean_tab"][:, :CH_OFF].abs().max()) == 0 and float(st["mean_tab"][:, CH_OFF + C:].abs().max()) == 0     # the other layers' columns
    # ... and against the float64 statistics of the real pixels themselves: the host-made partials are fp32 sums of 128 values
    x = st["case"]["x"].double().view(groups, ipg, C, hw * hw)[:, :valid]
    true_mean = x.mean((1, 3)).cuda()
    absmean = x.abs().mean((1, 3)).cuda()
    hold(fam, f"mean vs the pixels {shape}", st["mean_tab"][:, cols], true_mean, U1 * mean.abs() + 128 * U32 * absmean, dims=("group", "channel"))


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_apply_elementwise(shape, mode, relu):
    """fb_bn_apply in its grid-stride, span and pooling forms, residual modes 0 / 1 / 2, with and without ReLU, with valid_pixels_per_group on
    the padded shapes.  The float64 value v comes from the kernel's OWN fp32 scale / shift tables (checked above).  Output within
    rounded_to_bf16_bound(relu(v), e); mask bit = (v > 0) outside the band |v| <= e; padding pixels: output bits, mask bytes and pooled
    output exactly zero whatever the residual holds there.  pool_out: the kernel pools the STORED (rounded) outputs in fp32 (fullbatchtraining_amd/csrc/bn.hip:
    'Pooled from the STORED (rounded) values', which is what makes it bit-identical to fb_avgpool2_fwd), so its reference is the float64 2x2
    mean of the stored outputs and the fp32 error before rounding three additions: 3 * 2^-24 * 0.25 sum |y|."""
    lib = _lib()
    C, hw, ipg, groups, valid = shape
    st = bn_state(shape)
    n, px, ppg = st["n"], st["px"], st["ppg"]
    dt = lib.dtype_code(BF)
    x, res = st["x"], st["res"]
    pooling = shape == BN_POOL
    assert lib.load().fb_bn_apply_can_pool(C, hw, ppg, dt) == (1 if pooling else 0)
    y = torch.full_like(x, 7.0)
    bits = torch.full((x.numel() // 8,), 0xAA, dtype=torch.uint8, device="cuda")
    pooled = torch.full((n, hw // 2, hw // 2, C), 7.0, dtype=BF, device="cuda") if pooling else None
    lib.call("fb_bn_apply", x.data_ptr(), y.data_ptr(), st["scale"].data_ptr(), st["shift"].data_ptr(), res.data_ptr() if mode else None,
             st["rscale"].data_ptr() if mode == 2 else None, st["rshift"].data_ptr() if mode == 2 else None, px, C, ppg,
             valid * hw * hw if valid < ipg else 0, relu, bits.data_ptr(), pooled.data_ptr() if pooling else None, hw if pooling else 0, dt, None, None)
    torch.cuda.synchronize()
    v, e = bn_apply_ref(x, _rep(st["scale"], ipg), _rep(st["shift"], ipg), res if mode else None, _rep(st["rscale"], ipg) if mode == 2 else None,
                        _rep(st["rshift"], ipg) if mode == 2 else None)
    real = st["real"]
    fam, what = "BatchNorm apply", f"{shape} residual mode {mode} relu {relu}"
    ref = torch.relu(v) if relu else v
    inf = torch.full((), float("inf"), dtype=torch.float64, device="cuda")         # padding images: held to exact zero below, not to the bound
    hold(fam, f"output {what}", y, ref, torch.where(real[:, None, None, None], rounded_to_bf16_bound(ref, e), inf))
    mask = ((bits.to(torch.int32)[:, None] >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1).view(n, hw, hw, C)
    wrong, band, neg = bn_mask_check(mask[real], v[real], e[real], out=y[real], relu=bool(relu))
    print(f"{fam}: mask {what}: {wrong} wrong bits outside the band, share inside the band {band:.2e}")
    assert wrong == 0 and neg == 0 and band < 1e-3, (wrong, neg, band)
    if valid < ipg:
        assert padding_exact_zero(y, real), "padding pixels must be exact zeros (+0 bits)"
        assert padding_exact_zero(bits.view(n, hw, hw, C // 8), real), "the mask bytes of padding pixels must be clear"
    if pooling:
        yp = y.double().view(n, hw // 2, 2, hw // 2, 2, C)
        pref = yp.mean(dim=(2, 4))
        hold(fam, f"pool_out {what}", pooled, pref, rounded_to_bf16_bound(pref, 3 * U32 * 0.25 * yp.abs().sum(dim=(2, 4))))
        assert padding_exact_zero(pooled, real), "the pooled output of padding images must be exact zeros"


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_backward_elementwise(shape):
    """fb_bn_bwd_reduce -> fb_bn_bwd_finalize -> fb_bn_bwd_apply (and fb_bn_bwd_apply2 where the channel vectors divide 256) behind
    fb_bn_apply(residual, ReLU) with the kernel's own mask bits, so dy = dout where the bit is set, else +0, exactly.
    dbeta / dgamma per (group, channel): a term reaches the row's partial through at most ceil(PB / rows) - 1 additions of its thread's chain
    and ``rows`` additions of the workgroup's row chain (PB pixels per workgroup, rows = 256 / channel vectors per pixel), fp32, then double:
    (ceil(PB / rows) + rows) * 2^-24 * sum |term|, three roundings more inside dy * ((x - mean) * invstd), one for the fp32 result.
    dx: fb_bn_dx's two fused multiply-adds, then one rounding; the reference uses the kernel's own coefficients, which are held to the
    bounds their sums imply."""
    lib = _lib()
    C, hw, ipg, groups, valid = shape
    st = bn_state(shape)
    n, px, ppg, count = st["n"], st["px"], st["ppg"], st["count"]
    dt = lib.dtype_code(BF)
    x, res, dout = st["x"], st["res"], st["dout"]
    y = torch.empty_like(x)
    bits = torch.zeros(x.numel() // 8, dtype=torch.uint8, device="cuda")
    lib.call("fb_bn_apply", x.data_ptr(), y.data_ptr(), st["scale"].data_ptr(), st["shift"].data_ptr(), res.data_ptr(), None, None, px, C, ppg,
             valid * hw * hw if valid < ipg else 0, 1, bits.data_ptr(), None, 0, dt, None, None)
    rows_out = lib.load().fb_bn_bwd_reduce_rows(px, ppg)
    part = torch.zeros(2, rows_out, C, device="cuda")
    lib.call("fb_bn_bwd_reduce", dout.data_ptr(), None, bits.data_ptr(), x.data_ptr(), st["mean_tab"].data_ptr(), st["invstd"].data_ptr(), C + CH_PAD, CH_OFF,
             part.data_ptr(), px, C, ppg, dt)
    gout = torch.zeros(groups, 2 * C + 64, device="cuda")
    coef = torch.zeros(groups, C, 3, device="cuda")
    lib.call("fb_bn_bwd_finalize", part.data_ptr(), rows_out, groups, C, float(count), st["scale"].data_ptr(), st["mean_tab"].data_ptr(), st["invstd"].data_ptr(),
             C + CH_PAD, CH_OFF, gout.data_ptr(), gout.data_ptr() + 4 * C, gout.shape[1], coef.data_ptr(), 0)
    dx, dy_out = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    lib.call("fb_bn_bwd_apply", dout.data_ptr(), None, bits.data_ptr(), x.data_ptr(), coef.data_ptr(), dx.data_ptr(), dy_out.data_ptr(), px, C, ppg, dt, None, None)
    torch.cuda.synchronize()
    mask = ((bits.to(torch.int32)[:, None] >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1).view(n, hw, hw, C).bool()
    dy = torch.where(mask, dout, torch.zeros_like(dout))
    assert bits_equal(dy_out, dy), "dy_out must be dout where the mask bit is set and +0 elsewhere, bit for bit"
    mu, inv = st["mean_tab"][:, CH_OFF:CH_OFF + C].double(), st["invstd"].double()
    term = dy.double() * ((x.double() - _rep(mu, ipg)) * _rep(inv, ipg))
    per_group = lambda t: t.view(groups, ipg * hw * hw, C).sum(1)
    s1, s2, a1, a2 = per_group(dy.double()), per_group(term), per_group(dy.double().abs()), per_group(term.abs())
    PB = px // rows_out
    chain = -(-PB // max(256 // (C // 8), 1)) + max(256 // (C // 8), 1)
    B1, B2 = chain * U32 * a1, (chain + 3) * U32 * a2
    fam = "BatchNorm backward"
    hold(fam, f"dbeta {shape}", gout[:, C:2 * C], s1, B1 + U1 * s1.abs(), dims=("group", "channel"))
    hold(fam, f"dgamma {shape}", gout[:, :C], s2, B2 + U1 * s2.abs(), dims=("group", "channel"))
    sc = st["scale"].double()
    cx = -sc * inv * s2 / count
    c0 = -sc * s1 / count - cx * mu
    Bx = (sc * inv).abs() / count * B2
    assert torch.equal(coef[..., 0], st["scale"])
    hold(fam, f"c_x {shape}", coef[..., 1], cx, Bx + U1 * cx.abs(), dims=("group", "channel"))
    hold(fam, f"c_0 {shape}", coef[..., 2], c0, sc.abs() / count * B1 + mu.abs() * Bx + U1 * c0.abs() + 2.0 ** -50 * ((sc * s1).abs() / count + (cx * mu).abs()),
         dims=("group", "channel"))
    cf = [_rep(coef[..., j], ipg) for j in range(3)]
    ref, E = bn_dx_ref(cf[0], cf[1], cf[2], dy, x)
    hold(fam, f"dx {shape}", dx, ref, rounded_to_bf16_bound(ref, E))
    if 256 % (C // 8) == 0:
        # two BatchNorms behind one gradient: the second one reads `res` as its input with coefficients of its own
        gen = torch.Generator().manual_seed(C)
        coef_b = (torch.randn(groups, C, 3, generator=gen) * 0.5).cuda()
        dxa, dxb = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        lib.call("fb_bn_bwd_apply2", dout.data_ptr(), bits.data_ptr(), x.data_ptr(), coef.data_ptr(), dxa.data_ptr(), res.data_ptr(), coef_b.data_ptr(),
                 dxb.data_ptr(), px, C, ppg, dt)
        torch.cuda.synchronize()
        assert bits_equal(dxa, dx)
        cb = [_rep(coef_b[..., j], ipg) for j in range(3)]
        refb, Eb = bn_dx_ref(cb[0], cb[1], cb[2], dy, res)
        hold(fam, f"dx of the second BatchNorm (fb_bn_bwd_apply2) {shape}", dxb, refb, rounded_to_bf16_bound(refb, Eb))


# ---------------------------------------------------------------------------------------------------------------------------------
# pools, head gradient, shortcut sampling
@pytest.mark.parametrize("hw,n,C", [(8, 3, 64), (7, 2, 64)])
def test_pools_and_sampling_elementwise(hw, n, C):
    """Copies are bit-equal to torch; sums are within rounded_to_bf16_bound(ref, terms * 2^-24 * sum |term|).  fb_avgpool2_fwd takes even maps
    only (it refuses the 7 x 7 one); the max pool and the sampling take both.  Max-pool backward on POST-ReLU input: exact zeros, whole
    windows tie, the first maximum in row-major window order takes the gradient (torch's CPU semantics: the float64 reference is torch's own
    CPU autograd); an input pixel collects at most four windows' gradients."""
    lib = _lib()
    dt = lib.dtype_code(BF)
    torch.manual_seed(7)
    x = torch.relu(torch.randn(n, C, hw, hw) - 0.3).to(BF)
    xd = nhwc(x).cuda()
    ho = (hw + 1) // 2
    # max pool forward: a copy
    ym = torch.full((n, ho, ho, C), 7.0, dtype=BF, device="cuda")
    lib.call("fb_maxpool3s2_fwd", xd.data_ptr(), ym.data_ptr(), n, hw, hw, C, dt)
    xr = x.double().requires_grad_(True)
    mp = F.max_pool2d(xr, 3, 2, 1)
    assert bits_equal(ym.cpu(), nhwc(mp.detach()).to(BF))
    # max pool backward: sums of up to four gradients
    dmp = torch.randn(n, C, ho, ho).to(BF)
    g, = torch.autograd.grad(mp, xr, dmp.double(), retain_graph=True)
    gabs, = torch.autograd.grad(mp, xr, dmp.double().abs())
    dxm = torch.full_like(xd, float("nan"))
    dmpd = nhwc(dmp).cuda()
    lib.call("fb_maxpool3s2_bwd", xd.data_ptr(), dmpd.data_ptr(), dxm.data_ptr(), n, hw, hw, C, dt)
    torch.cuda.synchronize()
    gref = nhwc(g)
    hold("pools", f"max-pool backward {(hw, n, C)}", dxm.cpu(), gref, rounded_to_bf16_bound(gref, 4 * U32 * nhwc(gabs)))
    # average pool
    if hw % 2 == 0:
        xa = torch.randn(n, hw, hw, C).to(BF).cuda()
        ya = torch.full((n, hw // 2, hw // 2, C), 7.0, dtype=BF, device="cuda")
        lib.call("fb_avgpool2_fwd", xa.data_ptr(), ya.data_ptr(), n, hw, hw, C, dt)
        torch.cuda.synchronize()
        q = xa.double().view(n, hw // 2, 2, hw // 2, 2, C)
        hold("pools", f"average pool {(hw, n, C)}", ya, q.mean(dim=(2, 4)), rounded_to_bf16_bound(q.mean(dim=(2, 4)), 4 * U32 * 0.25 * q.abs().sum(dim=(2, 4))))
    else:
        with pytest.raises(lib.EngineError, match="odd"):
            lib.call("fb_avgpool2_fwd", xd.data_ptr(), ym.data_ptr(), n, hw, hw, C, dt)
    # shortcut sampling: forward a copy; backward adds in place on the sampled pixels and touches nothing else
    xs = torch.randn(n, hw, hw, C).to(BF).cuda()
    ys = torch.full((n, ho, ho, C), 7.0, dtype=BF, device="cuda")
    lib.call("fb_subsample2_fwd", xs.data_ptr(), ys.data_ptr(), n, hw, hw, C, dt)
    torch.cuda.synchronize()
    assert bits_equal(ys, xs[:, ::2, ::2])
    dxs = torch.randn(n, hw, hw, C).to(BF).cuda()
    before = dxs.clone()
    dys = torch.randn(n, ho, ho, C).to(BF).cuda()
    lib.call("fb_subsample2_bwd_add", dxs.data_ptr(), dys.data_ptr(), n, hw, hw, C, dt)
    torch.cuda.synchronize()
    sref = before[:, ::2, ::2].double() + dys.double()
    hold("pools", f"sampling backward {(hw, n, C)}", dxs[:, ::2, ::2], sref, rounded_to_bf16_bound(sref, 2 * U32 * (before[:, ::2, ::2].double().abs() + dys.double().abs())))
    keep = torch.ones(hw, hw, dtype=torch.bool, device="cuda")
    keep[::2, ::2] = False
    assert bits_equal(dxs[:, keep], before[:, keep])


def test_head_input_gradient_elementwise():
    """fb_head_bwd's d_a = (dlogits @ W_group) / HW, the same bf16 value at each of the HW pixels: ``classes`` products and sums, the fp32
    reciprocal of HW and the product with it: (classes + 2) * 2^-24 * sum |dz_j W_jc| / HW before the rounding.  (hw, n, C) = (4, 5, 512),
    five groups of one image: a weight matrix each."""
    lib = _lib()
    hw, n, C, classes, ipg = 4, 5, 512, 10, 1
    groups = n // ipg
    torch.manual_seed(6)
    P = classes * C + 16 + 64
    theta = (torch.randn(groups, P) * 0.2).cuda()
    dlogits = (torch.randn(n, classes) * 0.1).cuda()
    feat = torch.randn(n, C).cuda()
    gout = torch.zeros(groups, P, device="cuda")
    d_a = torch.full((n, hw, hw, C), 7.0, dtype=BF, device="cuda")
    boff = classes * C
    lib.call("fb_head_bwd", feat.data_ptr(), dlogits.data_ptr(), theta.data_ptr(), P, gout.data_ptr(), gout.data_ptr() + 4 * boff, P,
             d_a.data_ptr(), groups, ipg, hw * hw, C, classes, lib.dtype_code(BF))
    torch.cuda.synchronize()
    W = theta[:, :boff].view(groups, classes, C).double().repeat_interleave(ipg, 0)          # [n, classes, C]
    terms = dlogits.double()[:, :, None] * W
    ref = (terms.sum(1) / (hw * hw))[:, None, None, :].expand(n, hw, hw, C)
    E = ((classes + 2) * U32 * terms.abs().sum(1) / (hw * hw))[:, None, None, :].expand(n, hw, hw, C)
    hold("head", f"d_a {(hw, n, C)}", d_a, ref, rounded_to_bf16_bound(ref, E))
    assert bits_equal(d_a, d_a[:, :1, :1].expand(n, hw, hw, C))
