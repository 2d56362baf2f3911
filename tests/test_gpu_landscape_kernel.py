"""``fb_mt_landscape_point`` (csrc/landscape.hip): one grid point of the loss landscape, theta = base + (dx x + dy y), and the forward
compute-dtype weight copies of theta in the same launch.

  * theta bit for bit against tests/landscape_ref.py (the float32 form the reference's ``_set_parameter_offset`` was recorded to have), on the
    golden offset vectors and on random operands;
  * the copies bit for bit against ``fb_weight_prep`` applied to the theta THE KERNEL WROTE, for FB_F32 and FB_BF16 (and against torch's own
    cast; at the largest sizes against the cast alone), also where the destination is not 16-byte aligned; padding columns and everything of w_fwd outside the layers keep the
    marker they held; layers: stem-like (Cin 3, padded), patches-like (Cin 27 of 32), 16 -> 16 3x3, 16 -> 32 1x1, a wide row (Cin 64), an
    offset that is not 16-byte aligned, gaps between layers, a layer that ends at n;
  * n = 1, one short of / exactly / one past a lane's vector, a wave's span, a workgroup's span and the grid's span (spans as the LIBRARY
    reports them), one vector and one element past the grid's span, the ResNet-20 arena and once the arena of the benchmark with the engine's
    own layer tables (declared to tests/test_gpu_update_production.py through ``exercises``);
  * two launches give the same bits; base, dx, dy and the SENTINEL columns behind n stay untouched; (0, 0) returns base; layer_tab = NULL gives the
    same theta and leaves w_fwd alone; a shared and a mixed misalignment of the arena operands; bad arguments are refused without a launch; a
    recorded list replayed after a new (x, y) gives the bits of the direct call."""
import os

import numpy as np
import pytest
import torch

from tests import landscape_ref
from tests.helpers import SENTINEL, padding_untouched
from tests.test_gpu_update_production import N18, exercises

pytestmark = pytest.mark.gpu

FB_ERR_ARG = -1
PAD = 64
MARK = 7.0                      # what w_fwd holds before a launch (exact in bf16)
XY = (0.3217, -0.7)             # non-dyadic
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
#          Cout taps Cin Cin_pad  gap in front
SMALL = ((16, 9, 3, 32, 5),      # stem-like; w_off = 5: not 16-byte aligned
         (16, 1, 27, 32, 0),     # the patches form of the CIFAR stem, right behind it (no gap)
         (16, 9, 16, 32, 7),     # 16 -> 16 3x3 (w_off again unaligned: rows start at every residue of 8)
         (32, 1, 16, 32, 13),    # 16 -> 32 1x1
         (8, 9, 64, 64, 64))     # a wide row without padding: whole 16-byte stores


def _lib():
    from fullbatchtraining_amd import lib
    lib.load()
    return lib


def _spans():
    h = _lib().load()
    vec, block, blocks = (h.fb_abi_constant(k) for k in (b"FB_LANDSCAPE_VEC", b"FB_LANDSCAPE_BLOCK", b"FB_LANDSCAPE_BLOCKS"))
    assert vec > 0 and block > 0 and blocks > 0
    return vec, block, blocks


def _sizes():
    vec, block, blocks = _spans()
    spans = (vec, 64 * vec, block * vec, blocks * block * vec)
    return sorted({1} | {s + d for s in spans for d in (-1, 0, 1)} | {spans[-1] + vec + 1})


def _rows_for(n, last_at_end=True, wc_shift=0):
    """Layer rows [w_off, Cout, taps, Cin, Cin_pad, wc_off, has_dgrad, 0] of SMALL that fit into [0, n), plus a wide layer that ends exactly at n."""
    rows, off, wc = [], 0, wc_shift
    for cout, taps, cin, cinp, gap in SMALL:
        off += gap
        if off + cout * taps * cin > n:
            break
        rows.append([off, cout, taps, cin, cinp, wc, len(rows) % 2, 0])
        off, wc = off + cout * taps * cin, wc + cout * taps * cinp
    tail = 4 * 9 * 64
    if last_at_end and rows and n - tail >= off + 3:
        rows.append([n - tail, 4, 9, 64, 64, wc, 1, 0])
        wc += tail
    return rows, wc


def _plan_rows(model_over, pixels):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Plan
    from fullbatchtraining_amd.models import construct_model
    plan = Plan(construct_model(compose(model_over).model, 3, 10), pixels)
    rows = [[L.w_off, L.cout, L.taps, L.cin_real, L.cin_pad, L.wc_off, 0 if L is plan.stem else 1, 0] for L in sorted(plan.layers, key=lambda L: L.w_off)]
    return plan, rows, plan.wc_total


def _operands(n, seed, shift=(0, 0, 0, 0)):
    """theta / base / dx / dy of n elements with SENTINEL columns behind them; ``shift``: elements each view starts behind a 16-byte boundary."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ops = {}
    for name, s in zip(("theta", "base", "dx", "dy"), shift):
        buf = torch.full((n + PAD + 4,), SENTINEL, device="cuda", dtype=torch.float32)
        ops[name] = buf[s:s + n + PAD]
        assert ops[name].data_ptr() % 16 == 4 * s
        if name != "theta":
            ops[name][:n].normal_(generator=gen)
            ops[name][:n].mul_(0.1 if name == "base" else 1.0)
    return ops


def _launch(ops, n, xy, tab, w_fwd, dtype):
    lib = _lib()
    lib.call("fb_mt_landscape_point", ops["theta"].data_ptr(), ops["base"].data_ptr(), ops["dx"].data_ptr(), ops["dy"].data_ptr(), n, xy.data_ptr(),
             None if tab is None else tab.data_ptr(), 0 if tab is None else tab.shape[0], None if w_fwd is None else w_fwd.data_ptr(), lib.dtype_code(dtype))


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    view = torch.int32 if a.element_size() == 4 else torch.int16
    return a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def _check(n, rows, wc_total, dtype, seed=0, xy=XY, shift=(0, 0, 0, 0), prep=True):
    lib = _lib()
    ops = _operands(n, seed, shift)
    before = {k: v.clone() for k, v in ops.items()}
    xy_t = torch.tensor(xy, device="cuda", dtype=torch.float32)
    tab = torch.tensor(rows, dtype=torch.int32, device="cuda") if rows else None
    w_fwd = torch.full((wc_total + PAD,), MARK, device="cuda", dtype=dtype)
    _launch(ops, n, xy_t, tab, w_fwd, dtype)
    torch.cuda.synchronize()
    tag = f"[landscape n={n} {dtype} layers={len(rows)} shift={shift}]"
    # ---- theta: the reference's float32 form, bit for bit; inputs and the columns behind n untouched
    want = landscape_ref.offset(before["base"][:n].cpu().numpy(), before["dx"][:n].cpu().numpy(), before["dy"][:n].cpu().numpy(), *xy)
    got = ops["theta"][:n].cpu().numpy()
    diff = int((got.view(np.int32) != want.view(np.int32)).sum())
    print(f"{tag} theta: {diff} of {n} elements differ in their bits")
    assert diff == 0
    for k in ("base", "dx", "dy"):
        assert _bits(ops[k], before[k]), f"{k} is read only"
    assert padding_untouched(ops["theta"], n)
    assert float(xy_t[0]) == np.float32(xy[0]) and float(xy_t[1]) == np.float32(xy[1])
    # ---- the copies: fb_weight_prep on the theta the kernel wrote (real columns), torch's cast, and the marker everywhere else
    touched = torch.zeros(wc_total + PAD, dtype=torch.bool, device="cuda")
    for w_off, cout, taps, cin, cinp, wc_off, _, _ in rows:
        view = w_fwd[wc_off:wc_off + cout * taps * cinp].view(cout * taps, cinp)
        touched[wc_off:wc_off + cout * taps * cinp].view(cout * taps, cinp)[:, :cin] = True
        cast = ops["theta"][w_off:w_off + cout * taps * cin].view(cout * taps, cin).to(dtype)
        assert _bits(view[:, :cin], cast), (tag, w_off, "copy != cast of theta")
        if prep:
            ref = torch.full((cout * taps * cinp,), MARK, device="cuda", dtype=dtype)
            lib.call("fb_weight_prep", ops["theta"].data_ptr() + 4 * w_off, 0, 0, 1, cout, taps, cin, cinp, ref.data_ptr(), None, lib.dtype_code(dtype), None)
            torch.cuda.synchronize()
            assert _bits(view[:, :cin], ref.view(cout * taps, cinp)[:, :cin]), (tag, w_off, "copy != fb_weight_prep")
    assert bool((w_fwd[~touched] == MARK).all()), f"{tag} padding columns / the rest of w_fwd were written"
    # ---- the same launch again: the same bits
    again = {k: v.clone() for k, v in before.items()}
    w_again = torch.full_like(w_fwd, MARK)
    _launch(again, n, xy_t, tab, w_again, dtype)
    torch.cuda.synchronize()
    assert _bits(again["theta"], ops["theta"]) and _bits(w_again, w_fwd), "two launches differ"
    # ---- layer_tab = NULL: the same theta, w_fwd left alone
    alone = {k: v.clone() for k, v in before.items()}
    w_alone = torch.full_like(w_fwd, MARK)
    _launch(alone, n, xy_t, None, w_alone, dtype)
    torch.cuda.synchronize()
    assert _bits(alone["theta"], ops["theta"]) and bool((w_alone == MARK).all())
    # ---- (0, 0): base, bit for bit
    zero = {k: v.clone() for k, v in before.items()}
    _launch(zero, n, torch.zeros(2, device="cuda"), tab, w_again, dtype)
    torch.cuda.synchronize()
    assert _bits(zero["theta"][:n], before["base"][:n]) and padding_untouched(zero["theta"], n)
    return ops, w_fwd


def test_point_on_the_golden_offset_vectors():
    """The reference's own operands and results (tests/golden/landscape.npz), every tensor at every recorded position."""
    vectors = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landscape.npz"))
    assert str(vectors["offset_form"]) == landscape_ref.FORM
    positions = vectors["offset/positions"]
    i = 0
    while f"offset/base/{i}" in vectors:
        base, dx, dy = (torch.from_numpy(vectors[f"offset/{k}/{i}"].reshape(-1).copy()).cuda() for k in ("base", "dx", "dy"))
        n = base.numel()
        for k, (x, y) in enumerate(positions):
            theta = torch.full((n + PAD,), SENTINEL, device="cuda")
            _launch(dict(theta=theta, base=base, dx=dx, dy=dy), n, torch.tensor([x, y], device="cuda", dtype=torch.float32), None, None, torch.float32)
            torch.cuda.synchronize()
            assert landscape_ref.same_bits(theta[:n].cpu().numpy(), vectors[f"offset/theta/{k}/{i}"].reshape(-1)), (i, k)
            assert padding_untouched(theta, n)
        i += 1
    assert i == 4 and n == 259


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_point_at_the_span_edges(dtype):
    vec, block, blocks = _spans()
    sizes = _sizes()
    assert sizes[0] == 1 and blocks * block * vec + vec + 1 in sizes and len(sizes) == 14
    for n in sizes:
        rows, wc = _rows_for(n)
        _check(n, rows, wc, DTYPES[dtype], seed=n, prep=n < 100_000)
    rows, _ = _rows_for(sizes[-1])
    assert len(rows) == len(SMALL) + 1 and rows[-1][0] + 4 * 9 * 64 == sizes[-1] and rows[0][0] % 4 == 1, "all layers, the last one ends at n"


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_point_with_misaligned_operands_and_destinations(dtype):
    n = 70_001
    rows, wc = _rows_for(n)
    _check(n, rows, wc, DTYPES[dtype], seed=1, shift=(1, 1, 1, 1))          # one misalignment shared by the four operands: a scalar head, then vectors
    _check(n, rows, wc, DTYPES[dtype], seed=2, shift=(3, 3, 3, 3))
    _check(n, rows, wc, DTYPES[dtype], seed=3, shift=(1, 0, 2, 0))          # mixed: element by element
    rows, wc = _rows_for(n, wc_shift=3)                                      # destinations that are not 16-byte aligned
    _check(n, rows, wc, DTYPES[dtype], seed=4)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_point_at_the_resnet20_arena(dtype):
    plan, rows, wc = _plan_rows(["model=resnet20"], 16)
    assert plan.n_params == 4_327_754 and len(rows) == len(plan.layers) == 21
    _check(plan.P, rows, wc, DTYPES[dtype])


@exercises("fb_mt_landscape_point")
def test_point_at_production_size():
    """ResNet-18's arena with the engine's own layer table (bf16 copies): 2.7 passes of the grid-stride loop."""
    plan, rows, wc = _plan_rows(["model=resnet18"], 32)
    assert plan.n_params == N18 and plan.P >= N18
    _check(plan.P, rows, wc, torch.bfloat16, prep=False)


def test_point_refuses_bad_arguments_without_a_launch():
    lib = _lib()
    h = lib.load()
    n = 4099
    rows, wc = _rows_for(n, last_at_end=False)
    ops = _operands(n, 2)
    w_fwd = torch.full((wc + PAD,), MARK, device="cuda", dtype=torch.bfloat16)
    xy = torch.tensor(XY, device="cuda", dtype=torch.float32)
    good = torch.tensor(rows, dtype=torch.int32, device="cuda")
    before = {k: v.clone() for k, v in ops.items()}
    stream = torch.cuda.current_stream().cuda_stream
    P = {k: v.data_ptr() for k, v in ops.items()}

    def point(**kw):
        a = dict(theta=P["theta"], base=P["base"], dx=P["dx"], dy=P["dy"], n=n, xy=xy.data_ptr(), tab=good.data_ptr(), n_layers=good.shape[0],
                 w_fwd=w_fwd.data_ptr(), dtype=lib.FB_BF16) | kw
        return h.fb_mt_landscape_point(*a.values(), stream)

    for k in ("theta", "base", "dx", "dy", "xy"):
        assert point(**{k: None}) == FB_ERR_ARG, k
        assert b"fb_mt_landscape_point" in h.fb_last_error_string()
    for k in ("theta", "base", "dx", "dy"):
        assert point(**{k: P[k] + 2}) == FB_ERR_ARG, (k, "misaligned")
    assert point(w_fwd=w_fwd.data_ptr() + 4) == FB_ERR_ARG
    assert point(w_fwd=None) == FB_ERR_ARG and point(n=-1) == FB_ERR_ARG and point(n_layers=-1) == FB_ERR_ARG and point(n_layers=513) == FB_ERR_ARG
    for bad in (7, -1, 2):
        assert point(dtype=bad) == FB_ERR_ARG
        assert point(dtype=bad, tab=None, n_layers=0, w_fwd=None) == FB_ERR_ARG, "an unknown dtype is refused with or without a table"

    def table(edit):
        t = [list(r) for r in rows]
        edit(t)
        return torch.tensor(t, dtype=torch.int32, device="cuda")

    bad_tables = dict(unsorted=table(lambda t: t.reverse()), overlapping=table(lambda t: t[1].__setitem__(0, t[1][0] - 1)),
                      outside=table(lambda t: t[-1].__setitem__(0, n - 5)), negative=table(lambda t: t[0].__setitem__(0, -4)),
                      cin_beyond_pad=table(lambda t: t[0].__setitem__(3, t[0][4] + 1)), no_taps=table(lambda t: t[0].__setitem__(2, 0)),
                      negative_copy=table(lambda t: t[0].__setitem__(5, -32)))
    for name, t in bad_tables.items():
        assert point(tab=t.data_ptr()) == FB_ERR_ARG, name
        assert b"layer table" in h.fb_last_error_string()
    assert point(n=rows[-1][0] + 5) == FB_ERR_ARG, "the same table against a shorter arena"
    torch.cuda.synchronize()
    assert all(_bits(ops[k], before[k]) for k in ops) and bool((w_fwd == MARK).all()), "a refused call launched something"
    assert point(n=0, tab=None, n_layers=0) == 0 and point() == 0
    torch.cuda.synchronize()
    assert not _bits(ops["theta"][:n], before["theta"][:n]) and not bool((w_fwd == MARK).all())


def test_point_through_a_recorded_command_list():
    """Recordable, with (x, y) on the device: the list recorded at one point, replayed after a two-float write, gives the bits of a direct call there."""
    lib = _lib()
    n = 70_001
    rows, wc = _rows_for(n)
    tab = torch.tensor(rows, dtype=torch.int32, device="cuda")
    ops, want = _operands(n, 3), _operands(n, 3)
    w_fwd, w_want = (torch.full((wc + PAD,), MARK, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    xy = torch.tensor(XY, device="cuda", dtype=torch.float32)
    streams = [torch.cuda.current_stream()]
    with lib.Recorder(streams) as rec:
        _launch(ops, n, xy, tab, w_fwd, torch.bfloat16)
    cl = rec.finish()
    assert len(cl) == 1
    first = ops["theta"].clone()
    for point in ((-0.25, 0.9), (0.0, 0.0), XY):
        xy.copy_(torch.tensor(point))
        cl.replay(streams)
        _launch(want, n, torch.tensor(point, device="cuda", dtype=torch.float32), tab, w_want, torch.bfloat16)
        torch.cuda.synchronize()
        assert _bits(ops["theta"], want["theta"]) and _bits(w_fwd, w_want), point
    assert _bits(ops["theta"], first), "back at the recorded point: the recorded bits"
