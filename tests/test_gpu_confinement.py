"""Every kernel launch is held to its operands (tests/helpers.py ``confined``): each operand lies in the middle of a slab of its own between 4 MiB
guard bands, the launch runs three times with the guards and the outputs' prior content filled with 0x00 / 0xFF (NaN, -1) / 0x7F (3e38), and must give
the same output bits every time (reads confined, outputs fully defined), leave guards and stride gaps alone (writes confined) and its inputs unchanged.
One case per launch form at small shapes; every case also compares the outputs with float64 torch on the same rounded inputs at the tolerance of the
existing test of that entry point in tests/test_gpu_ops.py.  Image counts of the persistent kernels come from the device's CU count: one with fewer tiles
than workers, one where a worker walks two tiles or more and the tile count is no multiple of the worker count (the prefetch past the last tile).

The last two tests are completeness checks: every entry point of ``lib._SIGS`` has a case here (or an exclusion with its reason), and every launch key
(class, kernel id, R, stride, flags word) that small ResNet-18 / -50 / -20(B) engines make is made by a case."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import Strided, confined

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
_KEYS = set()            # launch keys (class, kernel id, R, stride, flags word) made by the cases
_DECLARED = set()        # entry points called inside ``confined`` by a case
_N_CASES = [0]
SWITCHES = ("FB_C1G", "FB_C1S_PIPE", "FB_C1S_ADD_ASM", "FB_H4_COMPACT", "FB_WGRAD3_COMPACT", "FB_IGEMM_NO_MASK", "FB_H4_NO_MASK", "FB_C1P_NO_MASK")


def _lib():
    from fullbatchtraining_amd import lib
    return lib


def tol(dtype, k=1.0):
    return (2e-5 if dtype == F32 else 1.2e-2) * k


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _key(cls, words):
    return (cls, words[10], words[7], words[8], words[9])


def _launched():
    """Keys of the launches recorded since the last call (filed with the cases' key set)."""
    lib = _lib()
    keys = {_key(cls, w) for cls, w, _ in lib.profile_read_launches()}
    lib.profile_read()
    _KEYS.update(keys)
    return keys


@pytest.fixture(autouse=True)
def _case(monkeypatch):
    lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    lib.profile_enable(True)
    try:
        yield
        _launched()
        _N_CASES[0] += 1
    finally:
        lib.profile_enable(False)
        try:
            torch.cuda.synchronize()
        except RuntimeError as err:             # a device fault is sticky: nothing more is started on this GPU
            pytest.exit(f"device error after a confinement case: {err}", returncode=3)


def _call(name, *args):
    _DECLARED.add(name)
    _lib().call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args])


def _p(t):
    return None if t is None else t.data_ptr()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _counts(tiles, workers, step=1, need=lambda n: True, cap=2100):
    """(n with fewer tiles than workers, n where a worker walks >= 2 tiles and tiles % workers != 0); ``need``: whole statistics blocks etc."""
    fit = [n for n in range(step, cap, step) if need(n)]
    small = next((n for n in fit[1:] + fit[:1] if tiles(n) < workers), None)          # (more than one unit of images where that still leaves workers idle)
    assert small is not None, "no image count gives fewer tiles than workers"
    big = next((n for n in range(step, cap, step) if need(n) and tiles(n) > workers and tiles(n) % workers != 0), None)
    assert big is not None, "no image count below the cap walks two tiles per worker"
    return small, big


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(gen, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, device="cuda", generator=gen) * scale).to(dtype)


def _bits(gen, n_el, dtype):
    """A ReLU bitmask as fb_bn_apply writes it: one byte per 16-byte vector; returns (bytes, keep [n_el] bool)."""
    vec = 8 if dtype == BF16 else 4
    keep = torch.rand(n_el, device="cuda", generator=gen) > 0.4
    b = (keep.view(-1, vec).to(torch.int32) << torch.arange(vec, device="cuda", dtype=torch.int32)).sum(1).to(torch.uint8)
    return b, keep


def _nchw64(t):
    return t.double().permute(0, 3, 1, 2)


def _oihw64(w, k):      # KRSC [co][k*k][ci] -> [co][ci][k][k]
    return w.double().view(w.shape[0], k, k, w.shape[2]).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ fb_conv2d --
def _conv_case(dtype, cin, cout, k, stride, hw, n, mode, amode=0, mask=False, bst=False, stat=False, split=None, wsets=1, want=None, seed=0):
    """One fb_conv2d launch form.  Forward: cin -> cout on hw x hw inputs; mode 1: the input gradient of that layer (dst has cin channels on hw x hw).
    ``split``: None | "f16x2" (fp32 with amax_*: fp16x2 planes).  ``wsets`` > 1: one weight set per n / wsets images.  ``want``: the kernel id."""
    lib = _lib()
    gen = _gen(seed + cin + 3 * cout + hw + n)
    pad = k // 2
    ho = (hw + 2 * pad - k) // stride + 1
    master = _randn(gen, wsets, cout, k * k, cin, scale=0.1)                       # forward KRSC sets
    wq = master.to(dtype)
    if mode == 0:
        src = _randn(gen, n, hw, hw, cin, dtype=dtype)
        dshape, wgt = (n, ho, ho, cout), wq
    else:
        src = _randn(gen, n, ho, ho, cout, dtype=dtype)
        dshape, wgt = (n, hw, hw, cin), wq.permute(0, 3, 2, 1).contiguous()            # [ci][tap][co]
    ipw = n // wsets
    ins = {"src": src}
    amax_imgs = 0
    if split == "f16x2":
        am_w = master.reshape(wsets, -1).abs().max(1).values.contiguous()
        planes_f, planes_d = torch.zeros_like(master), torch.zeros_like(master)
        lib.weight_prep(master, master[0].numel(), master[0].numel(), wsets, cout, k * k, cin, cin, planes_f, planes_d, F32, amax=am_w)
        wgt = planes_f if mode == 0 else planes_d
        groups = 2 if n % 2 == 0 else 1
        amax_imgs = n // groups
        ins["amax_src"] = src.reshape(groups, -1).abs().max(1).values.contiguous()
        ins["amax_wgt"] = am_w
    ins["wgt"] = wgt
    if amode == 1:
        ins["addend"] = _randn(gen, *dshape, dtype=dtype)
    elif amode == 2:
        ins["addend"] = _randn(gen, n, dshape[1] // 2, dshape[2] // 2, dshape[3], dtype=dtype)
    keep_a = keep_b = None
    if mask:
        ins["addend_mask"], keep_a = _bits(gen, n * dshape[1] * dshape[2] * dshape[3], dtype)
    if bst:
        ins["bst_x"] = _randn(gen, *dshape, dtype=dtype, scale=1.5)
        ins["bst_mask"], keep_b = _bits(gen, n * dshape[1] * dshape[2] * dshape[3], dtype)
    dtc = lib.dtype_code(dtype)

    def args(o):
        return lib.ConvArgs(_p(o.get("src")), _p(o.get("wgt")), _p(o.get("dst")), _p(o.get("addend")), _p(o.get("stat")), n, src.shape[1], src.shape[2], src.shape[3],
                            dshape[1], dshape[2], dshape[3], k, k, stride, pad, mode, ipw if wsets > 1 else 0, wgt[0].numel() if wsets > 1 else 0, amode, dtc,
                            _p(o.get("addend_mask")), _p(o.get("bst_x")), _p(o.get("bst_mask")), _p(o.get("amax_src")), _p(o.get("amax_wgt")), amax_imgs)

    outs = {"dst": (dshape, dtype)}
    if stat or bst:
        floats = int(lib.load().fb_ws_conv_stat_floats(C.byref(args({}))))
        nblk = -(-n * dshape[1] * dshape[2] // 128)
        assert floats == 2 * nblk * dshape[3]                                             # the size formula the header states
        outs["stat"] = ((2, nblk, dshape[3]), F32)
    if mask:
        assert lib.load().fb_conv_masked_addend_supported(C.byref(args(ins | {"dst": src} | ({"stat": src} if bst else {}))))
    if bst:
        assert lib.load().fb_conv_bwd_stat_supported(C.byref(args(ins | {"dst": src, "stat": src})))

    def fn(o):
        _DECLARED.add("fb_conv2d")
        lib.call("fb_conv2d", C.byref(args(o)))

    got = confined(fn, ins, outs)
    keys = _launched()
    if want is not None:
        assert {kk[1] for kk in keys} == {want}, (keys, want)
    # float64 reference on the same rounded inputs
    wref = master.double() if split == "f16x2" else wq.double()
    parts = []
    for s in range(wsets):
        sl = slice(s * ipw, (s + 1) * ipw)
        w64 = _oihw64(wref[s], k)
        if mode == 0:
            parts.append(F.conv2d(_nchw64(src[sl]), w64, None, stride, pad))
        else:
            parts.append(torch.nn.grad.conv2d_input((ipw, cin, hw, hw), w64, _nchw64(src[sl]), stride, pad))
    ref = torch.cat(parts).permute(0, 2, 3, 1)
    if amode:
        add = ins["addend"].double()
        if amode == 2:
            add = 0.25 * add.repeat_interleave(2, 1).repeat_interleave(2, 2)
        if mask:
            add = add * keep_a.view(add.shape)
        ref = ref + add
    err = rel(got["dst"], ref)
    assert err < (1.5e-6 if split == "f16x2" else tol(dtype)), err
    if stat and mode == 0:
        flat = ref.reshape(-1, dshape[3])
        padded = torch.zeros(nblk * 128, dshape[3], dtype=torch.float64, device="cuda")
        padded[:flat.shape[0]] = flat
        blocks = padded.view(nblk, 128, -1)
        assert rel(got["stat"][0], blocks.sum(1)) < 1e-4 and rel(got["stat"][1], (blocks * blocks).sum(1)) < 1e-4
    if bst:
        g = (got["dst"].double() * keep_b.view(dshape)).reshape(nblk, 128, -1)
        xb = ins["bst_x"].double().reshape(nblk, 128, -1)
        assert rel(got["stat"][0], g.sum(1)) < 1e-4 and rel(got["stat"][1], (g * xb).sum(1)) < 1e-4
    return keys


def _h4_counts(W, ch_tiles, workers_per_cu, stat):
    ipt = 1 if W >= 16 else 256 // (W * W)
    need = (lambda n: n * W * W % 128 == 0) if stat else (lambda n: True)
    return _counts(lambda n: n * W * W // 256 * ch_tiles, workers_per_cu * _cus(), step=ipt, need=need)


def _halo4_cases():
    out = []
    # (dtype, split, cin, cout, W): bf16 W = 32 (not 64 -> 64: that is halo5's), 16, 8; fp32 bf16x6 and f16x2
    for dtype, split, cin, cout, W in ((BF16, None, 64, 128, 32), (BF16, None, 128, 128, 16), (BF16, None, 256, 256, 8),
                                       (F32, None, 64, 64, 32), (F32, None, 128, 128, 16), (F32, None, 128, 128, 8),
                                       (F32, "f16x2", 64, 64, 32), (F32, "f16x2", 128, 128, 16), (F32, "f16x2", 128, 128, 8)):
        tag = f"{'bf16' if dtype == BF16 else 'f32' + (split or 'bf16x6')}-{cin}-{cout}-W{W}"
        out.append(pytest.param(dtype, split, cin, cout, W, 0, 0, False, False, id=f"{tag}-fwd"))
        out.append(pytest.param(dtype, split, cin, cout, W, 1, 0, False, False, id=f"{tag}-dgrad"))
        out.append(pytest.param(dtype, split, cin, cout, W, 1, 1, False, False, id=f"{tag}-dgrad-addend"))
        out.append(pytest.param(dtype, split, cin, cout, W, 1, 1, True, False, id=f"{tag}-dgrad-masked"))
        out.append(pytest.param(dtype, split, cin, cout, W, 1, 2, False, False, id=f"{tag}-dgrad-pooled"))
        if dtype == BF16 and W != 32:
            out.append(pytest.param(dtype, split, cin, cout, W, 1, 0, False, True, id=f"{tag}-dgrad-bst"))
            out.append(pytest.param(dtype, split, cin, cout, W, 1, 1, True, True, id=f"{tag}-dgrad-masked-bst"))
    return out


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("dtype,split,cin,cout,W,mode,amode,mask,bst", _halo4_cases())
def test_conv3x3_halo4(dtype, split, cin, cout, W, mode, amode, mask, bst, which):
    stat = (mode == 0) or bst
    dst_c = cout if mode == 0 else cin
    small, big = _h4_counts(W, dst_c // 64, 2, stat)
    _conv_case(dtype, cin, cout, 3, 1, W, small if which == "small" else big, mode, amode=amode, mask=mask, bst=bst, stat=stat, split=split, want=3)


@pytest.mark.parametrize("which", ["small", "big", "odd"])
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("mode,amode,mask,bst", [(0, 0, False, False), (1, 0, False, False), (1, 1, False, False), (1, 1, True, False), (1, 2, False, False),
                                                  (1, 0, False, True), (1, 1, True, True)])
def test_conv3x3_halo4_on_4x4_maps(mode, amode, mask, bst, compact, which, monkeypatch):
    """W = 4: the compact layout (64-channel tiles, two workgroups per CU) and, with FB_H4_COMPACT=0, the padded one (128-channel tiles, one per CU); 16 images per tile"""
    if not compact:
        monkeypatch.setenv("FB_H4_COMPACT", "0")
    stat = (mode == 0) or bst
    C_ = 512
    small, big = _h4_counts(4, C_ // (64 if compact else 128), 2 if compact else 1, stat)
    n = {"small": small, "big": big, "odd": 48}[which]                # three tiles (the kernel takes whole tiles only: 9 images go to the implicit GEMM, see test_igemm_glds)
    _conv_case(BF16, C_, C_, 3, 1, 4, n, mode, amode=amode, mask=mask, bst=bst, stat=stat, want=3)


@pytest.mark.parametrize("dtype,split", [(BF16, None), (F32, None), (F32, "f16x2")])
@pytest.mark.parametrize("mode", [0, 1])
def test_conv3x3_halo4_per_chunk_weight_sets(dtype, split, mode):
    """imgs_per_wset < n_img: the regulariser's second pass, one weight set per chunk"""
    _conv_case(dtype, 128, 128, 3, 1, 16, 24, mode, stat=mode == 0, split=split, wsets=3, want=3)
    _conv_case(dtype, 64, 64, 3, 1, 32, 6, mode, stat=mode == 0, split=split, wsets=2, want=3)              # (64 -> 64 @32: per-chunk sets keep it off halo5)


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("mode,amode,mask,bst", [(0, 0, False, False), (1, 0, False, False), (1, 1, False, False), (1, 1, True, False), (1, 0, False, True),
                                                  (1, 1, False, True), (1, 1, True, True)])
def test_conv3x3_halo5(mode, amode, mask, bst, which):
    """the resident-filter 64 -> 64 kernel on 32 x 32 maps: the forward form and its six input-gradient instantiations; four tiles per image, one workgroup per CU"""
    small, big = _counts(lambda n: 4 * n, _cus())
    _conv_case(BF16, 64, 64, 3, 1, 32, small if which == "small" else big, mode, amode=amode, mask=mask, bst=bst, stat=mode == 0 or bst, want=4)


@pytest.mark.parametrize("n", [3, 9, 24])
@pytest.mark.parametrize("amode", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,hw", [(64, 128, 32), (128, 256, 16), (256, 512, 8)])
def test_conv3x3s2_dgrad_quad(cin, cout, hw, amode, n):
    """WQ = 16 / 8 / 4 (1 / 2 / 8 images per tile), odd image counts: a last tile that is not full"""
    _conv_case(BF16, cin, cout, 3, 2, hw, n, 1, amode=amode, want=5)


def _c1_counts(cs, cd, hw, mode, add, kernel, stat):
    """1x1 streaming kernels: units of max(16384 / Cs, 128) pixels shared by (1 or 2) x CUs / channel-groups workers"""
    unit = max(16384 // cs, 128)
    if kernel == "pipe":
        nw = 8 if cd % (128 if cs == 64 else 256) == 0 else 4
        cw = 32
    else:
        nw = 4 if add else (8 if mode == 0 else 4)
        cw = 16 if (nw == 8 and cs != 64 and cd % 256 != 0) else 32
    nwc = ((4 if cs == 64 else 8) if nw == 8 else (2 if cs == 64 else 4))
    n_co = cd // (nwc * cw)
    workers = max(1, ((1 if nw == 8 else 2) * _cus()) // n_co)
    need = (lambda n: n * hw * hw % 128 == 0) if stat else (lambda n: True)
    return _counts(lambda n: -(-n * hw * hw // unit), workers, need=need)


def _c1_forms():
    """(Cs, Cd, mode, addend_mode, mask, stat, switches, kernel, kernel id)"""
    out = []
    for cs, cd in ((64, 128), (128, 256), (256, 512), (256, 128)):
        for mode, amode, mask, stat in ((0, 0, False, True), (0, 0, False, False), (1, 0, False, False), (1, 1, False, False), (1, 1, True, False)):
            form = (cs, cd, mode, amode, mask, stat)
            tag = f"{cs}-{cd}-{'fwd' if mode == 0 else 'dgrad'}{'-stat' if stat else ''}{'-addend' if amode else ''}{'-masked' if mask else ''}"
            plain128 = cs == 128 and not amode                       # by default K = 128 without addend stays on the round-3 kernel
            out.append(pytest.param(*form, {}, "stream" if plain128 else "pipe", 7 if plain128 else 9, id=f"{tag}-default"))
            if plain128:
                out.append(pytest.param(*form, {"FB_C1S_PIPE": "2"}, "pipe", 9, id=f"{tag}-pipe2"))
            out.append(pytest.param(*form, {"FB_C1S_PIPE": "0"}, "stream", 2 if mask else 7, id=f"{tag}-pipe0"))      # (no mask in the round-3 kernel: the implicit GEMM applies it)
            if amode and not mask:
                out.append(pytest.param(*form, {"FB_C1S_PIPE": "0", "FB_C1S_ADD_ASM": "0"}, "stream", 7, id=f"{tag}-pipe0-addasm0"))
    return out


@pytest.mark.parametrize("which", ["small", "big", "ragged"])
@pytest.mark.parametrize("cs,cd,mode,amode,mask,stat,env,kernel,want", _c1_forms())
def test_conv1x1_stream_and_pipe(cs, cd, mode, amode, mask, stat, env, kernel, want, which, monkeypatch):
    """K = Cs = 64 / 128 / 256 (forward: cin = Cs; input gradient: the forward layer's cout = Cs), with / without statistics, addend, masked addend, under both
    settings of FB_C1S_PIPE and of FB_C1S_ADD_ASM"""
    monkeypatch.setenv("FB_C1G", "0")
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    hw = 14
    small, big = _c1_counts(cs, cd, hw, mode, bool(amode), kernel, stat)
    n = {"small": small, "big": big, "ragged": 9}[which]
    if which == "ragged":
        hw, n = (8, 6) if stat else (7, 9)                                   # M = 441: no multiple of the unit, of 128 or of 64; statistics: three whole blocks
    cin, cout = (cs, cd) if mode == 0 else (cd, cs)
    _conv_case(BF16, cin, cout, 1, 1, hw, n, mode, amode=amode, mask=mask, stat=stat, want=want)


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("cs,cd,mode,amode,mask,stat,sw", [(128, 512, 0, 0, False, True, "1"), (256, 1024, 0, 0, False, False, "1"), (512, 256, 0, 0, False, True, "1"),
                                                           (512, 256, 0, 0, False, False, "1"), (512, 256, 1, 0, False, False, "2"), (256, 256, 1, 1, False, False, "2"),
                                                           (128, 256, 1, 1, True, False, "2"), (1024, 512, 0, 0, False, True, "1")])
def test_conv1x1_gemm(cs, cd, mode, amode, mask, stat, sw, which, monkeypatch):
    """the 256 x 256-tile GEMM kernel (FB_C1G=1: every forward call it can take, 2: input gradients too): all four instantiations, K = 128 ... 1024"""
    monkeypatch.setenv("FB_C1G", sw)
    hw = 14
    need = (lambda n: n * hw * hw % 128 == 0) if stat else (lambda n: True)
    small, big = _counts(lambda n: -(-n * hw * hw // 256) * (cd // 256), _cus(), need=need)
    cin, cout = (cs, cd) if mode == 0 else (cd, cs)
    _conv_case(BF16, cin, cout, 1, 1, hw, small if which == "small" else big, mode, amode=amode, mask=mask, stat=stat, want=10)


@pytest.mark.parametrize("n", [3, 40, 1032])
def test_conv1x1_k32(n):
    """the stem on its patches (K = 32 -> 64): a wave per 128-pixel block, four per workgroup: n = 3 images of 16 x 16 are 6 blocks; 1032 images of 32 x 32
    are more workgroups than the 8 x CUs the grid holds (grid-stride)"""
    hw = 16 if n == 3 else 32
    if n == 1032:
        assert -(-n * hw * hw // 512) > 8 * _cus() or _cus() > 256
    _conv_case(BF16, 32, 64, 1, 1, hw, n, 0, stat=True, want=6)
    _conv_case(BF16, 32, 64, 1, 1, hw, n, 0, stat=False, want=6)


@pytest.mark.parametrize("dtype,split", [(BF16, None), (F32, None), (F32, "f16x2")])
@pytest.mark.parametrize("cin,cout,k,stride,hw,n,mode,amode,mask,stat", [
    (64, 128, 3, 2, 8, 8, 0, 0, False, True), (64, 128, 3, 2, 32, 3, 0, 0, False, True),       # the 3x3 stride-2 forward
    (128, 128, 3, 1, 7, 9, 0, 0, False, False), (128, 128, 3, 1, 7, 9, 1, 1, True, False),     # 3x3 on 7x7: M = 441
    (64, 64, 3, 1, 14, 5, 0, 0, False, False), (64, 64, 3, 1, 14, 5, 1, 0, False, False),      # 3x3 on 14x14: M = 980
    (64, 512, 1, 1, 7, 9, 1, 0, False, False), (64, 512, 1, 1, 7, 9, 1, 1, False, False),      # 1x1 input gradient with Cs = 512
    (256, 64, 1, 1, 7, 9, 0, 0, False, False), (64, 64, 1, 1, 8, 6, 0, 0, False, True),        # 1x1 layers no streaming kernel takes
    (64, 64, 3, 1, 4, 9, 1, 2, False, False),                                                  # 4x4 maps, nine images: no whole halo tile
    (64, 128, 3, 2, 8, 8, 1, 2, False, False), (64, 128, 3, 2, 8, 8, 1, 0, False, False),      # stride-2 input gradient (fp32: no quad kernel)
    (64, 128, 3, 2, 4, 8, 1, 0, False, False), (64, 128, 3, 2, 4, 8, 1, 2, False, False),      # ... onto a 4 x 4 map: dY is 2 x 2, no quad kernel in bf16 either
    (64, 256, 1, 1, 8, 6, 1, 2, False, False),                                                 # 1x1 input gradient with a pooled addend
])
def test_igemm_glds(dtype, split, cin, cout, k, stride, hw, n, mode, amode, mask, stat):
    want = 2
    if dtype == BF16 and stride == 2 and mode == 1 and hw // 2 in (4, 8, 16):
        want = 5
    _conv_case(dtype, cin, cout, k, stride, hw, n, mode, amode=amode, mask=mask, stat=stat, split=split, want=want)


# ------------------------------------------------------------------------------------------------------------ fb_conv2d_wgrad --
# 1, 5 and more slices than a chunk has images; and the K-slice counts Engine._choose_split picks for the engines of the completeness check below (the profiler
# files split_k in a weight-gradient launch's flags word, so a launch key holds it)
SPLITS = [1, 2, 4, 5, 7, 8, 14, 16, 32, 64]


def _wgrad_case(dtype, cin, cout, k, stride, hw, ipg, groups, split_k, amax=False, gap=0, bn=None, want=None, seed=0):
    """dw[g][split] = sum over chunk g's pixels of dy (x) x, against torch's conv2d_weight in float64 after fb_wgrad_reduce's fixed-order sum (done here in
    float64).  ``gap`` > 0: the arena form, split_k = 1 and group_stride = slab + gap.  ``bn``: None | "mask" | "nomask": the BatchNorm apply in the loader."""
    lib = _lib()
    gen = _gen(seed + cin + cout + hw + ipg)
    pad = k // 2
    n = ipg * groups
    ho = (hw + 2 * pad - k) // stride + 1
    x = _randn(gen, n, hw, hw, cin, dtype=dtype)
    dy = _randn(gen, n, ho, ho, cout, dtype=dtype)
    ins = {"x": x, "dy": dy}
    if amax:
        ins["amax_x"] = x.reshape(groups, -1).abs().max(1).values.contiguous()
        ins["amax_dy"] = dy.reshape(groups, -1).abs().max(1).values.contiguous()
    keep = None
    if bn:
        # multiples of 1/8 and coefficients that are powers of two: dy' = c_dy * dy + c_x * bn_x + c_0 is exact in fp32 in any order of evaluation, so its one
        # rounding to the storage type is the same in the kernel and in float64 (a last-bit difference of a bf16 dy' would be 2^-9 of that element)
        def eighths(*shape):
            return (torch.randint(-32, 33, shape, device="cuda", generator=gen).float() / 8).to(dtype)
        ins["dy"] = dy = eighths(n, ho, ho, cout)
        ins["bn_x"] = eighths(n, ho, ho, cout)
        pick = torch.tensor([0.5, 1.0, 2.0, -1.0], device="cuda")
        ins["bn_coef"] = torch.stack([pick[torch.randint(0, 4, (groups, cout), device="cuda", generator=gen)], pick[torch.randint(0, 4, (groups, cout), device="cuda", generator=gen)],
                                      torch.randint(-8, 9, (groups, cout), device="cuda", generator=gen).float() / 4], -1).contiguous()
        if bn == "mask":
            ins["bn_mask"], keep = _bits(gen, dy.numel(), dtype)
    dtc = lib.dtype_code(dtype)
    slab = cout * k * k * cin

    def args(o, gs):
        return lib.WgradArgs(_p(o.get("x")), _p(o.get("dy")), _p(o.get("dw")), n, hw, hw, cin, ho, ho, cout, k, k, stride, pad, ipg, split_k, dtc, gs,
                             _p(o.get("amax_x")), _p(o.get("amax_dy")), _p(o.get("bn_x")), _p(o.get("bn_mask")), _p(o.get("bn_coef")))

    if gap:
        assert split_k == 1
        outs = {"dw": Strided(groups, slab, slab + gap)}
        gs = slab + gap
    else:
        floats = int(lib.load().fb_ws_wgrad_slab_floats(C.byref(args({}, 0))))
        assert floats == groups * split_k * slab
        outs = {"dw": ((groups, split_k, slab), F32)}
        gs = 0
    if bn:
        assert lib.load().fb_wgrad_bn_fused_supported(C.byref(args(ins, gs)))

    def fn(o):
        _DECLARED.add("fb_conv2d_wgrad")
        lib.call("fb_conv2d_wgrad", C.byref(args(o, gs)))

    got = confined(fn, ins, outs)["dw"].double()
    keys = _launched()
    if want is not None:
        assert {kk[1] for kk in keys} == {want}, (keys, want)
    got = got if gap else got.sum(1)
    dy64 = dy.double()
    if bn:                                              # dy' = c_dy * (dy masked) + c_x * bn_x + c_0, rounded to the storage type (fb_bn_bwd_apply's dx)
        cf = ins["bn_coef"].double().repeat_interleave(ipg, 0)[:, None, None]
        dym = dy64 * keep.view(dy.shape) if keep is not None else dy64
        dy64 = (cf[..., 0] * dym + cf[..., 1] * ins["bn_x"].double() + cf[..., 2]).to(dtype).double()
    worst = 0.0
    for g in range(groups):
        sl = slice(g * ipg, (g + 1) * ipg)
        ref = torch.nn.grad.conv2d_weight(_nchw64(x[sl]), (cout, cin, k, k), dy64[sl].permute(0, 3, 1, 2), stride, pad)
        worst = max(worst, rel(got[g].view(cout, k, k, cin).permute(0, 3, 1, 2), ref))
    assert worst < (1.5e-6 if amax else 1e-5), worst
    return keys


@pytest.mark.parametrize("dtype,amax", [(BF16, False), (F32, False), (F32, True)])
@pytest.mark.parametrize("cin,cout,stride,hw,ipg,groups", [(64, 64, 1, 32, 4, 2), (128, 64, 1, 16, 6, 2), (64, 128, 1, 8, 6, 2), (128, 64, 1, 4, 12, 2), (64, 64, 1, 4, 10, 1),
                                                           (64, 128, 2, 32, 4, 2), (128, 64, 2, 16, 5, 1), (64, 64, 2, 8, 8, 2), (64, 64, 1, 14, 7, 2), (128, 128, 1, 28, 2, 2),
                                                           (64, 64, 1, 2, 32, 2), (64, 128, 2, 4, 32, 2)])                  # 2 x 2 maps: no all-taps kernel
@pytest.mark.parametrize("split_k", SPLITS)
def test_conv_wgrad_3x3(dtype, amax, cin, cout, stride, hw, ipg, groups, split_k):
    """bf16: wgrad3x3_v2 (id 18); fp32: wgrad3x3 (id 17: bf16x6, fp16x2 planes; stride 2 with planes only) or the generic kernel (id 16); split_k = 1, 5 and
    more slices than a chunk has images (empty slices contribute zeros); split_k = 1 also in the arena form with a gap between the groups' slabs"""
    W = (hw + 2 - 3) // stride + 1
    if dtype == BF16:
        want = 18 if (W in (32, 16, 8, 4, 14, 28) and not (stride == 2 and W == 32) and not (W in (14, 28) and stride == 2) and not (W == 4 and ipg % 2)) else 16
    else:
        want = 17 if (W in (32, 16, 8, 4) and (stride == 1 or amax)) else 16
    _wgrad_case(dtype, cin, cout, 3, stride, hw, ipg, groups, split_k, amax=amax, want=want)
    if split_k == 1:
        _wgrad_case(dtype, cin, cout, 3, stride, hw, ipg, groups, 1, amax=amax, gap=40, want=want)


def test_conv_wgrad_3x3_padded_4x4_layout(monkeypatch):
    monkeypatch.setenv("FB_WGRAD3_COMPACT", "0")
    for split_k in (1, 3):
        _wgrad_case(BF16, 128, 64, 3, 1, 4, 12, 2, split_k, want=18)
    _wgrad_case(BF16, 128, 64, 3, 1, 4, 12, 2, 1, gap=8, want=18)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("cin,cout,hw,ipg,groups", [(64, 128, 8, 4, 2), (128, 64, 7, 3, 2), (256, 1024, 7, 4, 2), (2048, 512, 7, 2, 1), (512, 128, 14, 2, 2), (64, 64, 8, 4, 2),
                                                    (128, 128, 8, 5, 2), (256, 512, 4, 4, 1)])
@pytest.mark.parametrize("split_k", SPLITS)
def test_conv_wgrad_1x1(dtype, cin, cout, hw, ipg, groups, split_k):
    """Cs = 64 ... 2048: bf16 wgrad1x1 (id 19; 64 -> 64 stays generic), fp32 the generic kernel; ragged pixel ranges (7 x 7 maps), empty slices"""
    want = 19 if dtype == BF16 and (cin >= 128 or cout >= 128) else 16
    _wgrad_case(dtype, cin, cout, 1, 1, hw, ipg, groups, split_k, want=want)
    if split_k == 1:
        _wgrad_case(dtype, cin, cout, 1, 1, hw, ipg, groups, 1, gap=24, want=want)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("bn", [None, "mask", "nomask"])
@pytest.mark.parametrize("cin_pad,hw,ipg,groups,split_k", [(32, 32, 4, 2, 1), (32, 16, 8, 3, 4), (160, 16, 4, 2, 2), (32, 8, 6, 2, 64), (32, 32, 4, 2, 16), (32, 32, 4, 2, 256),
                                                           (160, 16, 4, 2, 16), (160, 16, 4, 2, 1)])
def test_conv_wgrad_stem(dtype, bn, cin_pad, hw, ipg, groups, split_k):
    """the stem on its patches (Cs = 32, and the ImageNet stem's 160): 64 x 32 tiles, the wide 64 x 160 tile (bf16), with the BatchNorm backward apply in the loader"""
    _wgrad_case(dtype, cin_pad, 64, 1, 1, hw, ipg, groups, split_k, bn=bn, want=16)
    if split_k == 1:
        _wgrad_case(dtype, cin_pad, 64, 1, 1, hw, ipg, groups, 1, bn=bn, gap=16, want=16)


@pytest.mark.parametrize("cin_pad,hw,ipg,groups,split_k", [(32, 32, 4, 2, 1), (32, 8, 6, 2, 5)])
def test_conv_wgrad_stem_fp16x2(cin_pad, hw, ipg, groups, split_k):
    """(the loader form takes no fp16x2 planes: fb_wgrad_bn_fused_supported)"""
    _wgrad_case(F32, cin_pad, 64, 1, 1, hw, ipg, groups, split_k, amax=True, want=16)


@pytest.mark.parametrize("groups,split_k,cd,taps,cs_pad,cs_real,gap", [(2, 3, 64, 9, 32, 27, 40), (3, 1, 64, 1, 160, 147, 8), (1, 5, 128, 9, 64, 64, 0), (2, 2, 64, 9, 64, 64, 100)])
def test_wgrad_reduce(groups, split_k, cd, taps, cs_pad, cs_real, gap):
    """the fixed-order sum of the split_k slabs with the channel padding dropped, into rows out_group_stride apart: the gap stays untouched"""
    gen = _gen(groups + cs_real)
    part = _randn(gen, groups, split_k, cd * taps, cs_pad)
    width = cd * taps * cs_real

    def fn(o):
        _call("fb_wgrad_reduce", o["part"], o["out"], width + gap, groups, split_k, cd, taps, cs_pad, cs_real)
    got = confined(fn, {"part": part}, {"out": Strided(groups, width, width + gap)})
    ref = part.double().sum(1)[..., :cs_real].reshape(groups, -1)
    assert rel(got["out"], ref) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ BatchNorm --
BN_SHAPES = [(64, 32), (128, 16), (256, 8), (512, 4), (64, 7)]           # (C, map width)


def _bn_images(W, groups):
    """images per group that fill whole 128-pixel blocks (7 x 7 maps: 128 images)"""
    for ipg in (2, 4, 8, 16, 32, 64, 128):
        if ipg * W * W % 128 == 0 and ipg * W * W >= 256:
            return ipg
    raise AssertionError


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C_,W", BN_SHAPES)
def test_bn_fwd_finalize(dtype, C_, W):
    """mean / var into columns [ch_off, ch_off + C) of [n_groups][ch_total] tables (the other columns are gaps), gamma / beta from parameter rows with a stride
    above 2C, scale / shift / invstd rows; float64 from the same partial sums"""
    groups = 3
    ipg = _bn_images(W, groups)
    ppg = ipg * W * W
    nblk = groups * ppg // 128
    gen = _gen(C_ + W)
    x = _randn(gen, nblk, 128, C_, dtype=dtype, scale=1.5).float() + 0.3
    part = torch.stack([x.sum(1), (x * x).sum(1)]).contiguous()
    ch_total, ch_off, pstride = C_ + 96, 32, 2 * C_ + 64
    params = torch.cat([torch.rand(groups, C_, device="cuda", generator=gen) + 0.5, _randn(gen, groups, C_, scale=0.1)], 1)

    def fn(o):
        _call("fb_bn_fwd_finalize", o["part"], nblk, groups, C_, float(ppg), o["params"], o["params"].data_ptr() + 4 * C_, pstride, 1e-5,
              o["mean"].data_ptr() - 4 * ch_off, o["var"].data_ptr() - 4 * ch_off, ch_total, ch_off, o["scale"], o["shift"], o["invstd"])
    got = confined(fn, {"part": part, "params": Strided(groups, 2 * C_, pstride, data=params)},
                   {"mean": Strided(groups, C_, ch_total), "var": Strided(groups, C_, ch_total), "scale": ((groups, C_), F32), "shift": ((groups, C_), F32),
                    "invstd": ((groups, C_), F32)})
    s = part.double().view(2, groups, -1, C_).sum(2)
    mean = s[0] / ppg
    var = s[1] / ppg - mean * mean
    inv = (var + 1e-5).rsqrt()
    assert rel(got["mean"], mean) < 1e-5 and rel(got["var"], var) < 1e-5 and rel(got["invstd"], inv) < 1e-5
    assert rel(got["scale"], params[:, :C_].double() * inv) < 1e-5 and rel(got["shift"], params[:, C_:].double() - mean * params[:, :C_].double() * inv) < 1e-5


def _bn_apply_forms():
    out = []
    for dtype in (F32, BF16):
        for C_, W in BN_SHAPES:
            for form in ("plain", "res", "rscale", "nomask-norelu", "valid") + (("pool",) if dtype == BF16 and W * C_ == 2048 and C_ <= 256 else ()):
                out.append(pytest.param(dtype, C_, W, form, id=f"{'f32' if dtype == F32 else 'bf16'}-{C_}-W{W}-{form}"))
    return out


@pytest.mark.parametrize("dtype,C_,W,form", _bn_apply_forms())
def test_bn_apply(dtype, C_, W, form):
    """y = relu?(x * scale + shift + residual): without / with residual / residual * rscale + rshift, mask bytes, fp32 amax (with its scratch at
    fb_ws_bn_amax_floats), the pooled output where fb_bn_apply_can_pool, zero padding pixels (valid_pixels_per_group)"""
    lib = _lib()
    groups = 3
    ipg = _bn_images(W, groups)
    n, ppg = groups * ipg, ipg * W * W
    px = n * W * W
    dtc = lib.dtype_code(dtype)
    # (the pooling pairs horizontal neighbours inside a wave: 64@32, 128@16, 256@8; at 512@4 the neighbour is in the next wave and the call is refused)
    assert lib.load().fb_bn_apply_can_pool(C_, W, ppg, dtc) == (1 if dtype == BF16 and W * C_ == 2048 and C_ <= 256 else 0)
    gen = _gen(C_ + W + len(form))
    x = _randn(gen, n, W, W, C_, dtype=dtype, scale=1.5)
    ins = {"x": x, "scale": torch.rand(groups, C_, device="cuda", generator=gen) + 0.5, "shift": _randn(gen, groups, C_, scale=0.3)}
    if form in ("res", "rscale", "pool", "valid"):
        ins["res"] = _randn(gen, n, W, W, C_, dtype=dtype)
    if form == "rscale":
        ins["rscale"], ins["rshift"] = torch.rand(groups, C_, device="cuda", generator=gen) + 0.5, _randn(gen, groups, C_, scale=0.3)
    relu = form != "nomask-norelu"
    valid = (ipg - 1) * W * W if form == "valid" else 0
    outs = {"y": ((n, W, W, C_), dtype)}
    scratch = {}
    if relu:
        outs["mask"] = ((x.numel() * x.element_size() // 16,), torch.uint8)
    if form == "pool":
        outs["pool"] = ((n, W // 2, W // 2, C_), dtype)
    if dtype == F32:
        outs["amax"] = ((groups,), F32)
        scratch["amax_ws"] = ((int(lib.load().fb_ws_bn_amax_floats(px, C_, ppg)),), F32)

    def fn(o):
        _call("fb_bn_apply", o["x"], o["y"], o["scale"], o["shift"], _p(o.get("res")), _p(o.get("rscale")), _p(o.get("rshift")), px, C_, ppg, valid, 1 if relu else 0,
              _p(o.get("mask")), _p(o.get("pool")), W if form == "pool" else 0, dtc, _p(o.get("amax")), _p(o.get("amax_ws")))
    got = confined(fn, ins, outs, scratch=scratch)
    xg = x.double().view(groups, -1, C_)
    ref = xg * ins["scale"].double()[:, None] + ins["shift"].double()[:, None]
    if "res" in ins:
        r = ins["res"].double().view(groups, -1, C_)
        ref = ref + (r * ins["rscale"].double()[:, None] + ins["rshift"].double()[:, None] if form == "rscale" else r)
    if relu:
        ref = torch.relu(ref)
    if valid:
        ref[:, valid:] = 0
        assert float(got["y"].view(groups, -1, C_)[:, valid:].abs().max()) == 0
    assert rel(got["y"].view(groups, -1, C_), ref) < tol(dtype, 0.5)
    if relu:
        vec = 16 // x.element_size()
        want = ((got["y"].float().reshape(-1, vec) > 0).to(torch.int32) << torch.arange(vec, device="cuda", dtype=torch.int32)).sum(1).to(torch.uint8)
        assert torch.equal(got["mask"], want)
    if dtype == F32:
        assert torch.equal(got["amax"], got["y"].reshape(groups, -1).abs().max(1).values)
    if form == "pool":
        pr = got["y"].double().view(n, W // 2, 2, W // 2, 2, C_).mean(dim=(2, 4))
        assert rel(got["pool"], pr) < tol(dtype, 0.5)


def test_bn_apply_refuses_to_pool_where_the_horizontal_neighbour_is_in_another_wave():
    """512 @ 4x4 and 1024 @ 2x2 have W * C == 2048 too, but a pixel's 64 (128) vectors fill a whole wave: the shuffle that fetches the neighbour cannot reach it"""
    lib = _lib()
    for C_, W in ((512, 4), (1024, 2)):
        assert lib.load().fb_bn_apply_can_pool(C_, W, 16 * W * W, lib.dtype_code(BF16)) == 0
    x = torch.zeros(16, 4, 4, 512, dtype=BF16, device="cuda")
    y, pool = torch.empty_like(x), torch.zeros(16, 2, 2, 512, dtype=BF16, device="cuda")
    sc = torch.ones(1, 512, device="cuda")
    with pytest.raises(lib.EngineError, match="average pooling"):
        lib.call("fb_bn_apply", x.data_ptr(), y.data_ptr(), sc.data_ptr(), sc.data_ptr(), None, None, None, 256, 512, 256, 0, 1, None, pool.data_ptr(), 4, lib.dtype_code(BF16), None, None)


def _bn_bwd_inputs(dtype, C_, W, groups, seed=0):
    ipg = _bn_images(W, groups)
    n = groups * ipg
    gen = _gen(C_ + W + seed)
    x, dout = _randn(gen, n, W, W, C_, dtype=dtype, scale=1.5), _randn(gen, n, W, W, C_, dtype=dtype)
    bits, keep = _bits(gen, x.numel(), dtype)
    return ipg, n, gen, x, dout, bits, keep.view(x.shape)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C_,W", BN_SHAPES)
@pytest.mark.parametrize("masked", ["mask", "y", "none"])
def test_bn_bwd_reduce_finalize_apply(dtype, C_, W, masked):
    """fb_bn_bwd_reduce (partial rows at 2 * fb_bn_bwd_reduce_rows * C, within fb_ws_bn_partial_floats; statistics read at ch_off of a wider table),
    fb_bn_bwd_finalize (dgamma / dbeta into parameter-stride rows: the rest of the row is a gap) and fb_bn_bwd_apply with dy_out and fp32 amax"""
    lib = _lib()
    groups = 3
    ipg, n, gen, x, dout, bits, keep = _bn_bwd_inputs(dtype, C_, W, groups)
    px, ppg = n * W * W, ipg * W * W
    dtc = lib.dtype_code(dtype)
    ch_total, ch_off, gstride = C_ + 96, 32, 2 * C_ + 64
    xg = x.double().view(groups, -1, C_)
    mean, inv = xg.mean(1), (xg.var(1, unbiased=False) + 1e-5).rsqrt()
    scale = (torch.rand(groups, C_, device="cuda", generator=gen) + 0.5)                  # (gamma * invstd as fb_bn_fwd_finalize writes it; any positive row serves)
    rows = int(lib.load().fb_bn_bwd_reduce_rows(px, ppg))
    assert 2 * rows * C_ <= int(lib.load().fb_ws_bn_partial_floats(px, C_))
    y = torch.where(keep, torch.ones_like(x), -torch.ones_like(x)) if masked == "y" else None
    ins = {"dout": dout, "x": x, "mean": Strided(groups, C_, ch_total, data=mean.float()), "invstd": inv.float().contiguous()}
    if masked == "mask":
        ins["mask"] = bits
    if masked == "y":
        ins["y"] = y

    def reduce(o):
        _call("fb_bn_bwd_reduce", o["dout"], _p(o.get("y")), _p(o.get("mask")), o["x"], o["mean"].data_ptr() - 4 * ch_off, o["invstd"], ch_total, ch_off, o["part"], px, C_, ppg, dtc)
    part = confined(reduce, ins, {"part": ((2, rows, C_), F32)})["part"]
    dy = dout.double() * keep if masked != "none" else dout.double()
    dyg = dy.view(groups, -1, C_)
    xhat = (xg - mean[:, None]) * inv[:, None]
    dbeta, dgamma = dyg.sum(1), (dyg * xhat).sum(1)
    sums = part.double().view(2, groups, -1, C_).sum(2)
    assert rel(sums[0], dbeta) < 1e-4 and rel(sums[1], dgamma) < 1e-4

    def finalize(o):
        _call("fb_bn_bwd_finalize", o["part"], rows, groups, C_, float(ppg), o["scale"], o["mean"].data_ptr() - 4 * ch_off, o["invstd"], ch_total, ch_off,
              o["grad"], o["grad"].data_ptr() + 4 * C_, gstride, o["coef"], 0)
    fin = confined(finalize, {"part": part, "scale": scale, "mean": ins["mean"], "invstd": ins["invstd"]},
                   {"grad": Strided(groups, 2 * C_, gstride), "coef": ((groups, C_, 3), F32)})
    assert rel(fin["grad"][:, :C_], dgamma) < 1e-4 and rel(fin["grad"][:, C_:], dbeta) < 1e-4
    outs = {"dx": (x.shape, dtype), "dy_out": (x.shape, dtype)}
    scratch = {}
    if dtype == F32:
        outs["amax"] = ((groups,), F32)
        scratch["amax_ws"] = ((int(lib.load().fb_ws_bn_amax_floats(px, C_, ppg)),), F32)
    ains = {k_: v for k_, v in ins.items() if k_ in ("dout", "x", "mask", "y")} | {"coef": fin["coef"]}

    def apply(o):
        _call("fb_bn_bwd_apply", o["dout"], _p(o.get("y")), _p(o.get("mask")), o["x"], o["coef"], o["dx"], o["dy_out"], px, C_, ppg, dtc, _p(o.get("amax")), _p(o.get("amax_ws")))
    got = confined(apply, ains, outs, scratch=scratch)
    dx = scale.double()[:, None] * (dyg - dbeta[:, None] / ppg - xhat * dgamma[:, None] / ppg)
    assert rel(got["dx"].view(groups, -1, C_), dx) < tol(dtype, 0.5)
    assert rel(got["dy_out"], dy) < tol(dtype, 0.5)
    if dtype == F32:
        assert torch.equal(got["amax"], got["dx"].reshape(groups, -1).abs().max(1).values)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C_,W", BN_SHAPES)
def test_bn_bwd_reduce2_apply2(dtype, C_, W):
    """two BatchNorms that share the incoming gradient: both partial tables, both dx tensors; float64 per BatchNorm"""
    lib = _lib()
    groups = 3
    ipg, n, gen, xa, dout, bits, keep = _bn_bwd_inputs(dtype, C_, W, groups, seed=1)
    xb = _randn(gen, *xa.shape, dtype=dtype)
    px, ppg = n * W * W, ipg * W * W
    dtc = lib.dtype_code(dtype)
    rows = int(lib.load().fb_bn_bwd_reduce_rows(px, ppg))
    mean_tab = _randn(gen, groups, 2 * C_, scale=0.1)
    inv = [torch.rand(groups, C_, device="cuda", generator=gen) + 0.5 for _ in range(2)]

    def reduce2(o):
        _call("fb_bn_bwd_reduce2", o["dout"], o["mask"], o["xa"], o["inv_a"], 0, o["part_a"], o["xb"], o["inv_b"], C_, o["part_b"], o["mean"], 2 * C_, px, C_, ppg, dtc)
    got = confined(reduce2, {"dout": dout, "mask": bits, "xa": xa, "xb": xb, "inv_a": inv[0], "inv_b": inv[1], "mean": mean_tab},
                   {"part_a": ((2, rows, C_), F32), "part_b": ((2, rows, C_), F32)})
    dyg = (dout.double() * keep).view(groups, -1, C_)
    for k_, x_ in enumerate((xa, xb)):
        xhat = (x_.double().view(groups, -1, C_) - mean_tab[:, k_ * C_:(k_ + 1) * C_].double()[:, None]) * inv[k_].double()[:, None]
        sums = got["part_a" if k_ == 0 else "part_b"].double().view(2, groups, -1, C_).sum(2)
        assert rel(sums[0], dyg.sum(1)) < 1e-4 and rel(sums[1], (dyg * xhat).sum(1)) < 1e-4
    coef = [_randn(gen, groups, C_, 3, scale=0.5) for _ in range(2)]

    def apply2(o):
        _call("fb_bn_bwd_apply2", o["dout"], o["mask"], o["xa"], o["coef_a"], o["dx_a"], o["xb"], o["coef_b"], o["dx_b"], px, C_, ppg, dtc)
    got = confined(apply2, {"dout": dout, "mask": bits, "xa": xa, "xb": xb, "coef_a": coef[0], "coef_b": coef[1]}, {"dx_a": (xa.shape, dtype), "dx_b": (xa.shape, dtype)})
    for k_, x_ in enumerate((xa, xb)):
        cf = coef[k_].double()[:, None]
        ref = cf[..., 0] * dyg + cf[..., 1] * x_.double().view(groups, -1, C_) + cf[..., 2]
        assert rel(got["dx_a" if k_ == 0 else "dx_b"].view(groups, -1, C_), ref) < tol(dtype, 0.5)


def test_bn_running_update_and_eval_coeffs():
    """C = 100 is no multiple of a wave; the running statistics are read-modify-write by definition (inout)"""
    from tests.helpers import bn_eval_coeffs_ref, bn_running_ref, within_bound
    gen = _gen(5)
    G, ch, passes = 3, 100, 2
    rm, rv = _randn(gen, ch), torch.rand(ch, device="cuda", generator=gen) + 0.5
    mt, vt = _randn(gen, passes, G, ch), torch.rand(passes, G, ch, device="cuda", generator=gen)
    ub = torch.full((ch,), 128.0 / 127.0, device="cuda")

    def upd(o):
        _call("fb_bn_running_update", o["rm"], o["rv"], o["mt"], o["vt"], passes, G * ch, o["ub"], G, ch, 0.1)
    got = confined(upd, {"mt": mt, "vt": vt, "ub": ub}, {}, inout={"rm": rm, "rv": rv})
    m, v, bm, bv = bn_running_ref(rm, rv, [(mt[p, g], vt[p, g], ub) for g in range(G) for p in range(passes)])
    assert within_bound(got["rm"], m, bm)[0] <= 1 and within_bound(got["rv"], v, bv)[0] <= 1
    gamma, beta = _randn(gen, ch), _randn(gen, ch)

    def ev(o):
        _call("fb_bn_eval_coeffs", o["gamma"], o["beta"], o["rm"], o["rv"], 1e-5, o["scale"], o["shift"], ch)
    got = confined(ev, {"gamma": gamma, "beta": beta, "rm": rm, "rv": rv}, {"scale": ((ch,), F32), "shift": ((ch,), F32)})
    s, sh, bs, bsh = bn_eval_coeffs_ref(gamma, beta, rm, rv)
    assert within_bound(got["scale"], s, bs)[0] <= 1 and within_bound(got["shift"], sh, bsh)[0] <= 1


# ---------------------------------------------------------------------------------------------------------- other entry points --
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("k,stride,pad,hw,cin_pad", [(3, 1, 1, 32, 32), (7, 2, 3, 64, 160), (3, 1, 1, 16, 64)])
@pytest.mark.parametrize("aug", ["none", "top-left", "bottom-right-flip", "mixed"])
def test_stem_patches(dtype, k, stride, pad, hw, cin_pad, aug):
    """the patch gather with the augmentation offsets at their extremes: the largest crop shift in each direction plus a flip is where it would read outside
    the image; bit for bit torch's unfold of the augmented image"""
    lib = _lib()
    n, c, cp = 9, 3, 4
    gen = torch.Generator().manual_seed(12 + hw)
    x = torch.randn(n, c, hw, hw, generator=gen)
    pv = [-0.49 / 0.25, -0.48 / 0.24, -0.45 / 0.26]
    ins = {"x": x}
    ref_img = x
    if aug != "none":
        if aug == "top-left":
            oy, ox, fl = torch.zeros(n, dtype=torch.int8), torch.zeros(n, dtype=torch.int8), torch.zeros(n, dtype=torch.int8)
        elif aug == "bottom-right-flip":
            oy, ox, fl = torch.full((n,), 2 * cp, dtype=torch.int8), torch.full((n,), 2 * cp, dtype=torch.int8), torch.ones(n, dtype=torch.int8)
        else:
            oy, ox = torch.tensor([0, 2 * cp] * 5, dtype=torch.int8)[:n], torch.tensor([2 * cp, 0, 0] * 3, dtype=torch.int8)[:n]
            fl = torch.tensor([1, 0] * 5, dtype=torch.int8)[:n]
        ins.update(oy=oy, ox=ox, fl=fl)
        padded = torch.empty(n, c, hw + 2 * cp, hw + 2 * cp)
        for ch in range(c):
            padded[:, ch] = pv[ch]
        padded[:, :, cp:cp + hw, cp:cp + hw] = x
        ref_img = torch.stack([padded[i, :, int(oy[i]):int(oy[i]) + hw, int(ox[i]):int(ox[i]) + hw] for i in range(n)])
        ref_img = torch.stack([im.flip(-1) if int(fl[i]) else im for i, im in enumerate(ref_img)])
    ho = (hw + 2 * pad - k) // stride + 1
    pvc = (lib.c_float * c)(*pv) if aug != "none" else None

    def fn(o):
        _call("fb_stem_patches", o["x"], o["patches"], n, c, hw, hw, k, stride, pad, cin_pad, _p(o.get("oy")), _p(o.get("ox")), _p(o.get("fl")), cp if aug != "none" else 0,
              pvc, lib.dtype_code(dtype))
    got = confined(fn, ins, {"patches": ((n, ho, ho, cin_pad), dtype)})["patches"]
    cols = F.unfold(ref_img.double(), kernel_size=k, padding=pad, stride=stride).view(n, c, k * k, ho * ho).permute(0, 3, 2, 1).reshape(n, ho, ho, k * k * c)
    ref = torch.zeros(n, ho, ho, cin_pad, dtype=torch.float64)
    ref[..., : k * k * c] = cols
    assert torch.equal(got.cpu().double(), ref.to(dtype).double())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n,hw,C_", [(3, 8, 64), (5, 16, 128), (2, 32, 64), (9, 4, 256)])
def test_avgpool2(dtype, n, hw, C_):
    x = _randn(_gen(hw + C_), n, hw, hw, C_, dtype=dtype)

    def fn(o):
        _call("fb_avgpool2_fwd", o["x"], o["y"], n, hw, hw, C_, _lib().dtype_code(dtype))
    got = confined(fn, {"x": x}, {"y": ((n, hw // 2, hw // 2, C_), dtype)})["y"]
    assert rel(got, x.double().view(n, hw // 2, 2, hw // 2, 2, C_).mean(dim=(2, 4))) < tol(dtype, 0.5)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("hw,n,C_", [(7, 2, 64), (14, 5, 128), (112, 2, 64), (8, 3, 64)])
def test_maxpool(dtype, hw, n, C_):
    """MaxPool2d(3, 2, 1) on odd maps (7 -> 4, 14 -> 7, 112 -> 56), post-ReLU input (whole windows tie): all four entry points against torch in float64"""
    lib = _lib()
    dtc = lib.dtype_code(dtype)
    gen = _gen(hw + n)
    x = torch.relu(_randn(gen, n, hw, hw, C_) - 0.3).to(dtype)
    ho = (hw + 1) // 2
    dy = _randn(gen, n, ho, ho, C_, dtype=dtype)
    xr = _nchw64(x).cpu().requires_grad_(True)               # (torch's CPU tie rule: the first maximum in row-major window order)
    mp, tidx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    mp.backward(_nchw64(dy).cpu())
    want_y, want_dx = mp.detach().permute(0, 2, 3, 1).cuda(), xr.grad.permute(0, 2, 3, 1).cuda()

    y0 = confined(lambda o: _call("fb_maxpool3s2_fwd", o["x"], o["y"], n, hw, hw, C_, dtc), {"x": x}, {"y": ((n, ho, ho, C_), dtype)})["y"]
    assert torch.equal(y0.double(), want_y)
    g1 = confined(lambda o: _call("fb_maxpool3s2_fwd_idx", o["x"], o["y"], o["idx"], n, hw, hw, C_, dtc), {"x": x}, {"y": ((n, ho, ho, C_), dtype), "idx": ((n, ho, ho, C_), torch.uint8)})
    assert torch.equal(g1["y"], y0) and int(g1["idx"].max()) <= 8
    pos = g1["idx"].permute(0, 3, 1, 2).long().cpu()
    oy, ox = torch.arange(ho).view(1, 1, ho, 1), torch.arange(ho).view(1, 1, 1, ho)
    assert torch.equal((2 * oy - 1 + pos // 3) * hw + (2 * ox - 1 + pos % 3), tidx)
    dx0 = confined(lambda o: _call("fb_maxpool3s2_bwd", o["x"], o["dy"], o["dx"], n, hw, hw, C_, dtc), {"x": x, "dy": dy}, {"dx": ((n, hw, hw, C_), dtype)})["dx"]
    dx1 = confined(lambda o: _call("fb_maxpool3s2_bwd_idx", o["idx"], o["dy"], o["dx"], n, hw, hw, C_, dtc), {"idx": g1["idx"], "dy": dy}, {"dx": ((n, hw, hw, C_), dtype)})["dx"]
    assert torch.equal(dx0, dx1) and rel(dx0, want_dx) < tol(dtype, 0.5)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("groups,ipg", [(1, 1), (1, 257), (3, 32)])
@pytest.mark.parametrize("smoothing,only_incorrect", [(0.0, 0), (0.1, 0), (0.05, 1)])
def test_head(dtype, groups, ipg, smoothing, only_incorrect):
    """fb_head_pool, fb_head_loss (the three loss variants, negative labels = padding rows at the fill 0xFF's own value), fb_head_bwd into arena rows with a gap"""
    lib = _lib()
    n, C_, hw, classes = groups * ipg, 64, 4, 10
    gen = _gen(n + int(100 * smoothing))
    a = _randn(gen, n, hw, hw, C_, dtype=dtype)
    feat = confined(lambda o: _call("fb_head_pool", o["a"], o["feat"], n, hw * hw, C_, lib.dtype_code(dtype)), {"a": a}, {"feat": ((n, C_), F32)})["feat"]
    assert rel(feat, a.double().mean((1, 2))) < 1e-5
    boff, P = classes * C_, classes * C_ + classes + 54
    theta = _randn(gen, groups, boff + classes, scale=0.2)
    labels = torch.randint(0, classes, (n,), device="cuda", generator=gen)
    if ipg > 4:
        labels[-2:] = -1                                                                   # padding rows

    def loss(o):
        _call("fb_head_loss", o["feat"], o["theta"], o["theta"].data_ptr() + 4 * boff, P, o["labels"], o["logits"], o["dlogits"], o["loss"], o["correct"], groups, ipg, C_,
              classes, smoothing, only_incorrect)
    got = confined(loss, {"feat": feat, "theta": Strided(groups, boff + classes, P, data=theta), "labels": labels},
                   {"logits": ((n, classes), F32), "dlogits": ((n, classes), F32), "loss": ((groups,), F32), "correct": ((groups,), F32)})
    dl_ref = []
    for g in range(groups):
        sl = slice(g * ipg, (g + 1) * ipg)
        Wm, b = theta[g, :boff].double().view(classes, C_), theta[g, boff:].double()
        z = (feat[sl].double() @ Wm.t() + b).requires_grad_(True)
        yl = labels[sl]
        real = yl >= 0
        logp = torch.log_softmax(z, -1)
        wgt = torch.full_like(z, smoothing / (classes - 1.0))
        wgt.scatter_(-1, yl.clamp_min(0).unsqueeze(-1), 1.0 - smoothing)
        per = (-wgt * logp).sum(-1)
        hit = (z.argmax(1) == yl) & real
        if only_incorrect:
            per = per * (1 - hit.double())
        ref = (per * real).sum() / real.sum()
        ref.backward()
        assert abs(float(got["loss"][g]) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
        assert float(got["correct"][g]) == float(hit.sum())
        assert rel(got["logits"][sl], z.detach()) < 1e-5
        dl_ref.append(z.grad)
    dl_ref = torch.cat(dl_ref)
    assert rel(got["dlogits"], dl_ref) < 1e-5

    def bwd(o):
        _call("fb_head_bwd", o["feat"], o["dlogits"], o["theta"], P, o["grad"], o["grad"].data_ptr() + 4 * boff, P, o["d_a"], groups, ipg, hw * hw, C_, classes, lib.dtype_code(dtype))
    gb = confined(bwd, {"feat": feat, "dlogits": got["dlogits"], "theta": Strided(groups, boff + classes, P, data=theta)},
                  {"grad": Strided(groups, boff + classes, P), "d_a": ((n, hw, hw, C_), dtype)})
    dl = got["dlogits"].double().view(groups, ipg, classes)
    fg = feat.double().view(groups, ipg, C_)
    assert rel(gb["grad"][:, :boff], torch.einsum("gik,gic->gkc", dl, fg).reshape(groups, -1)) < 1e-5 and rel(gb["grad"][:, boff:], dl.sum(1)) < 1e-5
    da = torch.einsum("gik,gkc->gic", dl, theta[:, :boff].double().view(groups, classes, C_)).reshape(n, 1, 1, C_) / (hw * hw)
    assert rel(gb["d_a"], da.expand(n, hw, hw, C_)) < tol(dtype, 0.5)


@pytest.mark.parametrize("n,classes", [(257, 10), (64, 1000), (1, 10)])
def test_head_tta(n, classes):
    gen = _gen(n + classes)
    za, zb = _randn(gen, n, classes, scale=3.0), _randn(gen, n, classes, scale=3.0)
    y = torch.randint(0, classes, (n,), device="cuda", generator=gen)

    def fn(o):
        _call("fb_head_tta", o["za"], o["zb"], o["y"], n, classes, o["ws"], o["loss"], o["correct"])
    got = confined(fn, {"za": za, "zb": zb, "y": y}, {"loss": ((1,), F32), "correct": ((1,), F32)}, scratch={"ws": ((2 * n,), F32)})
    outputs = torch.softmax(za.double(), 1) + torch.softmax(zb.double(), 1)
    loss_sum = F.cross_entropy(outputs, y, reduction="sum")
    assert abs(float(got["loss"]) - float(loss_sum)) < 1e-5 * max(1.0, float(loss_sum))
    assert float(got["correct"]) == float((outputs.argmax(1) == y).sum())


@pytest.mark.parametrize("dtype,planes", [(F32, False), (BF16, False), (F32, True)])
@pytest.mark.parametrize("with_dgrad", [True, False])
@pytest.mark.parametrize("co,taps,ci,cip", [(64, 9, 27, 32), (64, 1, 147, 160), (128, 9, 64, 64), (64, 1, 100, 128)])
def test_weight_prep(dtype, planes, with_dgrad, co, taps, ci, cip):
    """master KRSC rows of several sets (a stride gap on both sides) -> w_fwd / w_dgrad in bf16, fp32 and fp16x2 planes (amax), Cin_real < Cin_pad zero-padded"""
    lib = _lib()
    sets = 3
    gen = _gen(co + taps + ci)
    master = _randn(gen, sets, co * taps * ci)
    n_out = co * taps * cip
    am = master.abs().max(1).values.contiguous()
    ins = {"master": Strided(sets, co * taps * ci, co * taps * ci + 100, data=master)}
    if planes:
        ins["amax"] = am
    outs = {"wf": Strided(sets, n_out, n_out + 64, dtype)}
    if with_dgrad:
        outs["wd"] = Strided(sets, n_out, n_out + 64, dtype)

    def fn(o):
        _call("fb_weight_prep", o["master"], co * taps * ci + 100, n_out + 64, sets, co, taps, ci, cip, o["wf"], _p(o.get("wd")), lib.dtype_code(dtype), _p(o.get("amax")))
    got = confined(fn, ins, outs)
    ref = torch.zeros(sets, co, taps, cip, dtype=torch.float64, device="cuda")
    ref[..., :ci] = master.double().view(sets, co, taps, ci)
    for name, r in (("wf", ref), ("wd", ref.permute(0, 3, 2, 1))):
        if name not in got:
            continue
        g = got[name]
        if planes:
            # per 32 values: 32 scaled fp16 high pieces, then 32 low pieces.  Two pieces of 11 significand bits each under one power-of-two scale per set hold
            # 22 bits below the set's largest magnitude: |high + low - scale * w| <= 2^-21 * scale * amax (2^-20 allowed)
            # (the scale brings amax into [2^14, 2^15); value j of a group sits at slot 8 * (j % 16 / 4) + 4 * (j / 16) + j % 4: csrc/conv_wgrad.hip)
            h = g.contiguous().view(torch.float16).view(sets, -1, 2, 32).double()
            slot = torch.tensor([8 * (j % 16 // 4) + 4 * (j // 16) + j % 4 for j in range(32)], device="cuda")
            val = (h[:, :, 0] + h[:, :, 1])[:, :, slot].reshape(sets, -1)
            flat = r.reshape(sets, -1)
            scale = 2.0 ** (14 - torch.floor(torch.log2(am.double())))
            assert float(((val / scale[:, None] - flat).abs().amax(1) / am.double()).max()) <= 2.0 ** -20
        else:
            assert torch.equal(g.double().view(r.shape), r.contiguous().to(dtype).double())


# ---------------------------------------------------------------------------------------------------------------- completeness --
EXCLUDED = {
    "fb_absmax": "guarded at arena size in tests/test_gpu_update_production.py",
    **{name: "fb_mt_*: guard columns checked at arena size in tests/test_gpu_update_production.py (padding_untouched)" for name in (
        "fb_mt_sqnorm", "fb_mt_accumulate", "fb_mt_fd_perturb", "fb_mt_fd_combine_accumulate", "fb_mt_fd_combine", "fb_mt_chunk_clip", "fb_mt_norms2", "fb_mt_clip_sgd",
        "fb_mt_scale", "fb_mt_sam_ascent", "fb_mt_sam_restore", "fb_mt_absmax2", "fb_mt_pnorm2", "fb_mt_norm_bias", "fb_mt_ema", "fb_mt_clip_scale", "fb_mt_grad_noise")},
}


ELSEWHERE = {name: "run through ``confined`` by tests/test_gpu_downsample_b.py::test_subsample_kernels_against_torch_slicing (dx of fb_subsample2_bwd_add as inout)"
             for name in ("fb_subsample2_fwd", "fb_subsample2_bwd_add")}


def test_every_entry_point_has_a_confinement_case():
    """(runs after the cases above: they file the entry points they call inside ``confined`` in module state, so this test and the next one are for runs of the
    whole file and say so when run alone)  The event and command-list calls launch no kernel and are not in
    ``lib._SIGS``.  A kernel added later without a case here fails this test."""
    lib = _lib()
    assert _N_CASES[0] > 100, "run the whole file: the cases above file what they launch"
    assert not set(EXCLUDED) & _DECLARED, "an excluded entry point has a case: drop the exclusion"
    assert all(name.startswith("fb_mt_") or name == "fb_absmax" for name in EXCLUDED)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_downsample_b.py")) as handle:
        other = handle.read()
    assert all(f'confined(lambda o: lib.call("{name}"' in other for name in ELSEWHERE) and not set(ELSEWHERE) & _DECLARED
    missing = set(lib._SIGS) - _DECLARED - set(EXCLUDED) - set(ELSEWHERE)
    assert not missing, f"entry points without a confinement case: {sorted(missing)}"
    # every kernel id the default dispatch can return (csrc/profile.h; 1 and 8 are never selected by default)
    ids = {k[1] for k in _KEYS if k[0] in ("igemm_fwd", "igemm_dgrad", "wgrad")}
    assert ids >= {2, 3, 4, 5, 6, 7, 9, 10, 16, 17, 18, 19}, sorted(ids)
    print(f"{_N_CASES[0]} cases, {len(_KEYS)} distinct launch keys, {len(_DECLARED)} entry points")


def _engine_keys(over, pixels, chunk, G, dtype, split=None, per_chunk=False):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Engine, stem_patches
    from fullbatchtraining_amd.models import construct_model
    from tests.helpers import make_data

    lib = _lib()
    cfg = compose(list(over))
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, 10)
    eng = Engine(model, pixels, chunk, G, compute_dtype=dtype, fd_sets=1 if per_chunk else 0, f32_split=split)
    x, y = make_data(G * chunk, pixels, 10)
    patches, y_dev = stem_patches(x.cuda(), eng.plan.stem, eng.dt), y.cuda()
    _launched()
    eng.prep_weights(eng.theta, 1)
    eng.group_gradient(patches, y_dev, G, eng.g)
    if per_chunk:
        for g in range(G):
            eng.theta_k[g] = eng.theta * (1 + 0.01 * (g + 1))
        eng.prep_weights(eng.theta_k, G, per_chunk=True)
        eng.group_gradient(patches, y_dev, G, eng.g_fd[0], 2, eng.theta_k, 1)
    eng.evaluate_batch(patches[:chunk + 3], y_dev[:chunk + 3])
    torch.cuda.synchronize()
    keys = {_key(cls, w) for cls, w, _ in lib.profile_read_launches()}
    lib.profile_read()
    return keys


ENGINES = [
    pytest.param(("model=resnet18",), 32, 128, 2, BF16, None, False, id="resnet18-bf16"),
    pytest.param(("model=resnet18",), 32, 128, 2, F32, "bf16x6", False, id="resnet18-f32-bf16x6"),
    pytest.param(("model=resnet18",), 32, 128, 2, F32, "f16x2", True, id="resnet18-f32-f16x2-per-chunk-sets"),
    pytest.param(("model=resnet50", "model.stem=standard"), 64, 32, 2, BF16, None, False, id="resnet50-standard-64px-bf16"),
    pytest.param(("model=resnet20",), 32, 128, 2, BF16, None, False, id="resnet20-B-bf16"),
]


@pytest.mark.parametrize("over,pixels,chunk,G,dtype,split,per_chunk", ENGINES)
def test_every_launch_form_of_the_engines_has_a_confinement_case(over, pixels, chunk, G, dtype, split, per_chunk):
    """One group_gradient (and the regulariser's per-chunk-weight-set pass) plus one evaluation of a small engine: every launch key (class, kernel id, R, stride,
    flags word) it makes must have been made by a case above.  Shape words are left out of the key on purpose: the per-width instantiations are in the cases'
    lists, the production sizes in the walks of tests/test_gpu_bf16_structural.py.  The key constrains the convolutions and weight gradients (kernel id, addend /
    mask / fused-reduction / storage-type bits, split_k); of a BatchNorm pass the profiler files residual, mask, dy_out and dual in words the key leaves out, so
    there it tells the pooled apply from the plain one and no more -- the BatchNorm forms are held by the parameter lists of their tests above."""
    assert _N_CASES[0] > 100, "run the whole file: the cases above file what they launch"
    cases = set(_KEYS)
    want = _engine_keys(over, pixels, chunk, G, dtype, split, per_chunk)
    print(f"{len(cases)} distinct launch keys from {_N_CASES[0]} cases; this engine makes {len(want)}")
    missing = want - cases
    assert not missing, f"launch forms of the engine without a confinement case: {sorted(missing)}"
