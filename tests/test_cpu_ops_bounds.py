"""The elementwise bounds of the bf16 convolution / BatchNorm kernels (tests/helpers.py: half_ulp_bf16, mfma_sum_bound, rounded_to_bf16_bound,
block_stat_bounds, bn_apply_ref, bn_mask_check, bn_dx_ref; applied to the kernels by tests/test_gpu_ops_bounds.py) are shown to bite, on the CPU.
The emulations are torch restatements of the kernels' arithmetic -- bf16-exact inputs, fp32 math, ONE round to nearest even -- and stay
within the bounds at every element; each planted error is outside them:
  * convolution forward / input gradient (addend modes 0, 1, 2): one output moved by one bf16 ulp away from the reference; truncation in place
    of round-to-nearest-even; one tap dropped at a border pixel; two channels exchanged at one pixel; the addend added AFTER the
    convolution was rounded (two roundings);
  * per-block statistics: one pixel's contribution moved to the next 128-pixel block (the totals stay equal);
  * BatchNorm apply: a coefficient of the neighbouring statistics group for one 16-byte vector; the mask bit taken from the rounded output
    where a positive value rounds to +0; a padding pixel that holds rshift; backward apply: c_0 dropped at one element.
What the one-ulp class of errors needs: the accumulation term E = (K + 1) 2^-23 A below what the error adds.  Truncation and a second
rounding move SOME element by almost a whole ulp, two half-ulps, against a bound of one half-ulp + E: such an element fails once E is below
half an ulp of it, E / |r| < 2^-9 .. 2^-8 (top .. bottom of its binade), i.e. A / |r| < 2^14 / (K + 1) .. 2^15 / (K + 1): 14 .. 28 at K = 1152,
8 .. 16 at K = 2048, 3.6 .. 7 at K = 4608.  With random signs the elements of largest |r| (3.5 - 4.5 sigma among 10^4 - 10^5 outputs) sit at
A / |r| ~ 0.18 sqrt(K) = 6 / 8 / 12: inside the window up to K = 2048, outside it at K = 4608.  So "some element fails" is ASSERTED for
truncation and for two roundings at every K <= 2048 and only printed at K = 4608, where the bounds the kernels are held to cannot see a
one-ulp error in random data.  The single output moved by one ulp is asserted at the planted element for K <= 576 and printed above.
Errors of the size of one missing product are asserted at every K."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import (U32, block_stat_bounds, bn_apply_ref, bn_case, bn_dx_ref, bn_mask_check, half_ulp_bf16, mfma_sum_bound,
                           padding_exact_zero, rounded_to_bf16_bound, within_bound)

SHAPES = [(64, 64, 3, 1, 8, 8), (64, 128, 3, 2, 8, 8), (512, 512, 3, 1, 4, 16), (2048, 512, 1, 1, 7, 4), (64, 128, 1, 1, 16, 3), (32, 64, 1, 1, 8, 4)]
ONE_ULP_K = 576                  # ONE output moved by one ulp is asserted at the planted element up to this K
SOME_ELEMENT_K = 2048            # truncation / two roundings: "some element fails" is asserted up to this K (module docstring: only K = 4608 is out of reach)
BF = torch.bfloat16


def rne(v):
    return v.to(BF).float()


def trunc(v):
    """fp32 -> bf16 by dropping the low 16 bits."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def ratios(got, ref, bound):
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def upsample_quarter(a, hw):
    """Gradient of AvgPool2d(2, 2) on an hw x hw map: 0.25 a[y // 2][x // 2]; the last row / column of an odd map lies in no window."""
    up = 0.25 * a.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return F.pad(up, (0, hw - up.shape[3], 0, hw - up.shape[2]))


def test_half_ulp_and_rounding_bound_values():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 2.0 ** -126, 0.0, 3e38], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -134, 2.0 ** -134, 2.0 ** 119], dtype=torch.float64)
    assert torch.equal(half_ulp_bf16(v), want)
    assert float(half_ulp_bf16(1.0 - 2.0 ** -53)) == 2.0 ** -9                  # the exponent, not a rounded logarithm
    # every fp32 value rounds to bf16 within the bound with E = 0, and the bound is attained (a tie): it cannot be tightened
    x = torch.randn(1 << 20, generator=torch.Generator().manual_seed(0)) * torch.exp(3 * torch.randn(1 << 20, generator=torch.Generator().manual_seed(1)))
    assert within_bound(rne(x), x.double(), rounded_to_bf16_bound(x.double(), 0.0))[0] <= 1.0
    tie = torch.tensor([1.0 + 2.0 ** -8])
    assert within_bound(rne(tie), tie.double(), rounded_to_bf16_bound(tie.double(), 0.0))[0] == 1.0
    assert within_bound(rne(x), x.double(), 0.5 * rounded_to_bf16_bound(x.double(), 0.0))[0] > 1.0          # a bound on 2^-9 fails honest rounding
    # rounding UP into the next binade: 1.998 -> 2.0 moved by less than half an ulp of [1, 2)
    up = torch.tensor([2.0 - 2.0 ** -9])
    assert float(rne(up)) == 2.0 and within_bound(rne(up), up.double(), rounded_to_bf16_bound(up.double(), 0.0))[0] <= 1.0
    assert mfma_sum_bound(2.0, 576) == 577 * 2.0 ** -23 * 2.0


# ---------------------------------------------------------------------------------------------------------------------------------
def conv_case(cin, cout, k, stride, hw, n, mode, amode):
    """-> dict: fp32 value before rounding (the emulation's accumulator + addend), float64 reference r, E, the bound, the plain convolution
    parts and a function that gives the centre tap's contribution at pixel (0, 0) of image 0 per output channel."""
    gen = torch.Generator().manual_seed(100 * mode + 10 * amode + k)
    pad = k // 2
    w = rne(torch.randn(cout, cin, k, k, generator=gen) * 0.1)
    if mode == 0:
        x = rne(torch.randn(n, cin, hw, hw, generator=gen))
        acc = F.conv2d(x, w, None, stride, pad)
        conv = F.conv2d(x.double(), w.double(), None, stride, pad)
        A = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad)
        K = cin * k * k
        centre = w[:, :, pad, pad] @ x[0, :, 0, 0]                        # output pixel (0, 0) reads x[0][0] through the centre tap (any stride)
    else:
        ho = (hw + 2 * pad - k) // stride + 1
        dy = rne(torch.randn(n, cout, ho, ho, generator=gen))
        shape = (n, cin, hw, hw)
        acc = torch.nn.grad.conv2d_input(shape, w, dy, stride, pad)
        conv = torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), stride, pad)
        A = torch.nn.grad.conv2d_input(shape, w.double().abs(), dy.double().abs(), stride, pad)
        K = cout * k * k
        centre = w[:, :, pad, pad].t() @ dy[0, :, 0, 0]                   # dx pixel (0, 0) receives dy[0][0] through the centre tap
    a32 = torch.zeros_like(acc)
    if amode == 1:
        a32 = rne(torch.randn(acc.shape, generator=gen))
    elif amode == 2:
        a32 = upsample_quarter(rne(torch.randn(acc.shape[0], acc.shape[1], acc.shape[2] // 2, acc.shape[3] // 2, generator=gen)), acc.shape[2])
    a64 = a32.double()
    r = conv + a64
    E = mfma_sum_bound(A, K) + (2 * U32 * (conv.abs() + a64.abs()) if amode else 0.0)
    return dict(acc=acc, a32=a32, pre=acc + a32, r=r, E=E, bound=rounded_to_bf16_bound(r, E), K=K, centre=centre)


CONV_CASES = [(s, 0, 0) for s in SHAPES] + [(s, 1, am) for s in SHAPES for am in (0, 1, 2)]


@pytest.mark.parametrize("shape,mode,amode", CONV_CASES)
def test_conv_honest_emulation_passes_and_planted_errors_fail(shape, mode, amode):
    c = conv_case(*shape, mode, amode)
    r, bound, K = c["r"], c["bound"], c["K"]
    what = f"{'forward' if mode == 0 else f'input gradient, addend mode {amode}'} {shape} K={K}"
    got = rne(c["pre"])
    ratio, _ = within_bound(got, r, bound)
    print(f"{what}: honest emulation, worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0

    # one output moved by one ulp away from the reference, planted where |r| is largest (there A / |r| is smallest)
    flat = got.reshape(-1).clone()
    i = int(r.abs().reshape(-1).argmax())
    away = 1.0 if float(flat[i]) >= float(r.reshape(-1)[i]) else -1.0
    ulp = 2 * float(half_ulp_bf16(abs(float(flat[i]))))
    moved = flat.clone()
    moved[i] = flat[i] + away * ulp
    assert float(rne(moved[i:i + 1])) == float(moved[i])                 # still a bf16 value
    one = float(ratios(moved[i:i + 1], r.reshape(-1)[i:i + 1], bound.reshape(-1)[i:i + 1]))
    everywhere = (got.double() + torch.where(got.double() >= r, 1.0, -1.0) * 2 * half_ulp_bf16(got.double().abs()) - r).abs() / bound
    print(f"{what}: one ulp away: ratio {one:.2f} at the planted element; {float((everywhere > 1).double().mean()):.1%} of all positions would fail")
    # truncation
    tr = ratios(trunc(c["pre"]), r, bound)
    print(f"{what}: truncation: {float((tr > 1).double().mean()):.1%} of the elements fail, worst {float(tr.max()):.2f}")
    # the addend added after the convolution was rounded
    if amode:
        twice = ratios(rne(rne(c["acc"]) + c["a32"]), r, bound)
        print(f"{what}: two roundings: {float((twice > 1).double().mean()):.2%} of the elements fail, worst {float(twice.max()):.2f}")
    if K <= ONE_ULP_K:
        assert one > 1.0
    if K <= SOME_ELEMENT_K:
        assert float(tr.max()) > 1.0
        if amode:
            assert float(twice.max()) > 1.0

    # one tap dropped at a border pixel: every K.  Planted elements: the channels whose dropped product sum is not itself tiny
    dropped = c["pre"].clone()
    dropped[0, :, 0, 0] -= c["centre"]
    dr = ratios(rne(dropped), r, bound)[0, :, 0, 0]
    ch = int(c["centre"].abs().argmax())
    print(f"{what}: centre tap dropped at pixel (0, 0): {float((dr > 1).double().mean()):.1%} of its channels fail, ratio {float(dr[ch]):.1f} at channel {ch}")
    assert float(dr[ch]) > 1.0 and float((dr > 1).double().mean()) > 0.9
    # two channels exchanged at one pixel (the last one): the channels with the largest and the smallest reference there
    px = r[-1, :, -1, -1]
    c0, c1 = int(px.argmax()), int(px.argmin())
    swapped = got.clone()
    swapped[-1, c0, -1, -1], swapped[-1, c1, -1, -1] = got[-1, c1, -1, -1], got[-1, c0, -1, -1]
    sw = ratios(swapped, r, bound)[-1, :, -1, -1]
    assert float(sw[c0]) > 1.0 and float(sw[c1]) > 1.0
    ratio, i = within_bound(swapped, r, bound)
    N, Cc, H, W = r.shape
    assert ratio > 1.0 and i in [((N - 1) * Cc + ch) * H * W + H * W - 1 for ch in (c0, c1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_block_statistics_bound_and_a_pixel_in_the_wrong_block(shape):
    """Sums and sums of squares of the fp32 accumulators per 128-pixel block (fb_conv2d's stat_partial): an honest fp32 sum passes; one
    pixel's contribution moved to the next block leaves the totals over the blocks equal and fails BOTH blocks, in the sum and in the sum of
    squares, at every K.  A block's bound is at least sum E_p = 128 (K + 1) 2^-23 A, so the error is planted where the REFERENCE says it stands
    out most: the (pixel, channel) of block 0 with the largest margin min(|r_p| / bound_sum, r_p^2 / bound_sumsq) over both blocks -- at
    K = 4608 an arbitrary pixel (A / |a_p| ~ 12 .. 15 against the needed 2^16 / (K + 1) = 14) would sit on the edge."""
    cin, cout, k, stride, hw, n = shape
    c = conv_case(*shape, 0, 0)
    acc = c["acc"].permute(0, 2, 3, 1).reshape(-1, cout)
    r, E = (t.permute(0, 2, 3, 1).reshape(-1, cout) for t in (c["r"], c["E"].expand_as(c["r"])))
    M = acc.shape[0]
    nblk = -(-M // 128)
    s, bs, q, bq = block_stat_bounds(r, E)
    assert s.shape == (nblk, cout)
    padded = torch.cat([acc, torch.zeros(nblk * 128 - M, cout)]).view(nblk, 128, cout)
    got_s, got_q = padded.sum(1), (padded * padded).sum(1)
    rs, rq = within_bound(got_s, s, bs)[0], within_bound(got_q, q, bq)[0]
    print(f"block statistics {shape}: honest fp32 sums, worst ratio {rs:.3f} (sums) {rq:.3f} (sums of squares); {nblk} blocks, last one holds {M - (nblk - 1) * 128} pixels")
    assert rs <= 1.0 and rq <= 1.0
    if nblk < 2:                                           # (64, 128, 3, 2, 8, 8): 128 output pixels, one block -- nothing to move
        return
    r0 = r[:128]
    margin = torch.minimum(torch.minimum(r0.abs() / bs[0], r0.abs() / bs[1]), torch.minimum(r0 * r0 / bq[0], r0 * r0 / bq[1]))
    p, ch = divmod(int(margin.argmax()), cout)             # this pixel of block 0 is counted in block 1
    bad_s, bad_q = got_s.clone(), got_q.clone()
    bad_s[0] -= acc[p]; bad_s[1] += acc[p]
    bad_q[0] -= acc[p] * acc[p]; bad_q[1] += acc[p] * acc[p]
    assert torch.allclose(bad_s.sum(0), got_s.sum(0), rtol=1e-5, atol=1e-5) and torch.allclose(bad_q.sum(0), got_q.sum(0), rtol=1e-5, atol=1e-5)
    seen = [(float(ratios(bad_s, s, bs)[b, ch]), float(ratios(bad_q, q, bq)[b, ch])) for b in (0, 1)]
    print(f"block statistics {shape}: pixel {p} (channel {ch}) counted in block 1: ratios (sum, sum of squares) block 0 {seen[0][0]:.2f} {seen[0][1]:.2f}, block 1 {seen[1][0]:.2f} {seen[1][1]:.2f}")
    assert min(min(pair) for pair in seen) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm apply: fp32, v = x * sc + sh (+ res | + res * rsc + rsh), ReLU, one rounding; the mask bit is v > 0 of the fp32 value
BN_SHAPES = [(96, 4, 8, 2, 8), (64, 8, 8, 2, 5), (512, 4, 16, 3, 13), (256, 8, 4, 2, 3)]            # the shapes of tests/test_gpu_ops_bounds.py


def bn_emulate(case, shape, mode, relu, fused):
    C, hw, ipg, groups, valid = shape
    x, res = case["x"], case["res"]
    xg = x.double().view(groups, ipg, C, hw * hw)[:, :valid]
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    scale = (case["gamma"].double() / (var + 1e-5).sqrt()).float()
    shift = (case["beta"].double() - mean * scale.double()).float()
    rep = lambda t: t.repeat_interleave(ipg, 0)[:, :, None, None]
    sc, sh, rsc, rsh = rep(scale), rep(shift), rep(case["rscale"]), rep(case["rshift"])
    if fused:                                              # the compiler may contract a product and a sum into one rounding
        v = (x.double() * sc.double() + sh.double()).float()
        if mode == 1:
            v = v + res
        if mode == 2:
            v = (res.double() * rsc.double() + v.double()).float() + rsh
    else:
        v = x * sc + sh
        if mode == 1:
            v = v + res
        if mode == 2:
            v = v + res * rsc + rsh
    v64, e = bn_apply_ref(x, sc, sh, res if mode else None, rsc if mode == 2 else None, rsh if mode == 2 else None)
    out = rne(torch.relu(v) if relu else v)
    out[~case["real"]] = 0
    mask = v > 0
    mask[~case["real"]] = False
    return dict(v32=v, out=out, mask=mask, v=v64, e=e, tabs=(sc, sh, rsc, rsh))


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_apply_bound_mask_band_and_planted_errors(shape, mode, relu):
    C, hw, ipg, groups, valid = shape
    case = bn_case(*shape)
    real = case["real"]
    for fused in (False, True):
        em = bn_emulate(case, shape, mode, relu, fused)
        ref = torch.relu(em["v"]) if relu else em["v"]
        bound = rounded_to_bf16_bound(ref, em["e"])
        ratio, _ = within_bound(em["out"][real], ref[real], bound[real])
        wrong, band, neg = bn_mask_check(em["mask"][real], em["v"][real], em["e"][real], out=em["out"][real], relu=bool(relu))
        print(f"BatchNorm apply {shape} mode {mode} relu {relu} fused {fused}: honest ratio {ratio:.3f}; share of elements in the mask's band {band:.2e}")
        assert ratio <= 1.0 and wrong == 0 and neg == 0
        assert band < 1e-3                                 # the condition the GPU test states for these seeds
    # a coefficient of the neighbouring statistics group for one 16-byte vector (8 channels of the first pixel of group 1)
    sc, sh, rsc, rsh = em["tabs"]
    i0 = ipg                                               # first image of group 1
    bad = em["out"].clone()
    vv = case["x"][i0, :8, 0, 0] * sc[0, :8, 0, 0] + sh[i0, :8, 0, 0]      # scale of group 0
    if mode == 1:
        vv = vv + case["res"][i0, :8, 0, 0]
    if mode == 2:
        vv = vv + case["res"][i0, :8, 0, 0] * rsc[i0, :8, 0, 0] + rsh[i0, :8, 0, 0]
    bad[i0, :8, 0, 0] = rne(torch.relu(vv) if relu else vv)
    assert float(ratios(bad, ref, bound)[i0, :8, 0, 0].max()) > 1.0
    assert within_bound(bad[real], ref[real], bound[real])[0] > 1.0
    if valid < ipg:
        # padding pixels: the predicate the GPU test applies (tests/helpers.py padding_exact_zero) accepts the honest result and rejects ONE padding
        # pixel that holds the residual's shift (mode 2) or the BatchNorm's own shift instead of exact zero, a -0, and one set mask bit
        out16, mask = em["out"].to(BF), em["mask"]
        assert padding_exact_zero(out16, real) and padding_exact_zero(mask, real)
        pad_img = valid                                    # first padding image of group 0
        bad = out16.clone()
        bad[pad_img, :, 0, 0] = (rsh if mode == 2 else sh)[pad_img, :, 0, 0].to(BF)
        assert not padding_exact_zero(bad, real)
        bad = out16.clone()
        bad[-1, -1, -1, -1] = -0.0                         # the last element of the last padding image: equal to zero, not its bits
        assert float(bad[-1, -1, -1, -1]) == 0.0 and not padding_exact_zero(bad, real)
        bad = mask.clone()
        bad[pad_img, 3, 0, 0] = True
        assert not padding_exact_zero(bad, real)


def test_bn_mask_bit_taken_from_the_rounded_output():
    """Taking the mask from the stored bf16 value differs from v > 0 exactly where a positive fp32 value rounds to +0 (below 2^-134).  Such a
    value with no cancellation behind it (x * scale, |v| = 1e-41 > e = 5 * 2^-24 |v|) is OUTSIDE the band: the cleared bit is rejected.  Inside
    the band (|v| <= e: the terms cancel to less than their own rounding error) the fp32 value itself may have either sign, and either bit
    is accepted."""
    x = torch.tensor([1.0, 1.0])
    scale, shift = torch.tensor([1e-41, 1.0]), torch.tensor([0.0, -(1.0 - 2.0 ** -24)])
    v, e = bn_apply_ref(x, scale, shift)
    v32 = x * scale + shift
    assert float(v32[0]) > 0 and float(rne(v32)[0]) == 0.0 and float(v[0]) > float(e[0])
    assert 0 < float(v[1]) <= float(e[1])
    from_output = rne(torch.relu(v32)) > 0
    assert bn_mask_check(from_output[:1], v[:1], e[:1])[0] == 1              # rejected outside the band
    for bit in (False, True):
        assert bn_mask_check(torch.tensor([bit]), v[1:], e[1:])[0] == 0      # accepted inside it
    assert bn_mask_check(torch.tensor([False]), torch.tensor([0.5], dtype=torch.float64), torch.tensor([1e-6], dtype=torch.float64))[0] == 1
    # a set bit over a negative stored output is reported when ReLU is on
    assert bn_mask_check(torch.tensor([True]), torch.tensor([1e-9], dtype=torch.float64), torch.tensor([1e-6], dtype=torch.float64),
                         out=torch.tensor([-1e-9]), relu=True)[2] == 1


@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_backward_apply_bound_and_dropped_constant(shape):
    """fb_bn_dx = fma(c_dy, dy, fma(c_x, x, c_0)): each fused multiply-add emulated as the exact product and sum in float64 (24 + 24 bit
    product: exact; the sum within 2^-53) rounded to fp32 once."""
    C, hw, ipg, groups, valid = shape
    case = bn_case(*shape)
    gen = torch.Generator().manual_seed(C)
    coef = torch.randn(groups, C, 3, generator=gen) * 0.5
    coef[..., 2] = (0.2 + 0.3 * torch.rand(groups, C, generator=gen)) * torch.where(torch.rand(groups, C, generator=gen) > 0.5, 1.0, -1.0)
    rep = lambda j: coef[..., j].repeat_interleave(ipg, 0)[:, :, None, None]
    x, dy = case["x"], case["dout"] * (case["res"] > 0)
    inner = (rep(1).double() * x.double() + rep(2).double()).float()
    dx32 = (rep(0).double() * dy.double() + inner.double()).float()
    ref, E = bn_dx_ref(rep(0), rep(1), rep(2), dy, x)
    bound = rounded_to_bf16_bound(ref, E)
    ratio, _ = within_bound(rne(dx32), ref, bound)
    print(f"BatchNorm backward apply {shape}: honest ratio {ratio:.3f}")
    assert ratio <= 1.0
    bad = rne(dx32)
    bad[-1, -1, -1, -1] = rne(dx32 - rep(2))[-1, -1, -1, -1]
    ratio, i = within_bound(bad, ref, bound)
    assert ratio > 1.0 and i == bad.numel() - 1
