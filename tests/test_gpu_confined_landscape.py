"""The confinement cases of the landscape point kernel (csrc/landscape.hip: ``fb_mt_landscape_point``), filed with the cases of
tests/test_gpu_confinement.py through that file's own ``_call``, so that its completeness check -- every launch entry point of the library has a
case that ran inside ``helpers.confined`` -- counts the entry point; this file sorts, and therefore runs, before it.  Guard bands around every
operand, three fills, n = 4099 (three trailing elements next to the guard): reads and writes confined, base / dx / dy / (x, y) / the layer table
unchanged, every element of theta defined whatever it held before, the weight copy an in-out operand (its padding columns are neither read nor
written, so they keep what they held), and results equal, bit for bit, to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests.test_gpu_landscape_kernel import DTYPES, MARK, XY, _launch, _operands, _rows_for
from tests.helpers import confined

pytestmark = pytest.mark.gpu

N = 4099
F32 = torch.float32


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_landscape_point_is_confined(dtype):
    dt = DTYPES[dtype]
    code = cases._lib().dtype_code(dt)
    rows, wc = _rows_for(N)
    assert len(rows) == 4 and rows[0][0] % 4 == 1 and rows[-1][0] + 32 * 16 < N, "four small layers, gaps around them, an unaligned offset"
    ops = _operands(N, 5)
    data = {k: ops[k][:N].clone() for k in ("base", "dx", "dy")}
    data["xy"], data["tab"] = torch.tensor(XY, device="cuda", dtype=F32), torch.tensor(rows, dtype=torch.int32, device="cuda")
    copy = torch.full((wc,), MARK, device="cuda", dtype=dt)

    def fn(o):
        cases._call("fb_mt_landscape_point", o["theta"], o["base"], o["dx"], o["dy"], N, o["xy"], o["tab"], len(rows), o["w_fwd"], code)

    got = confined(fn, inputs=data, outputs=dict(theta=((N,), F32)), inout=dict(w_fwd=copy))
    w_want = copy.clone()
    _launch(ops, N, data["xy"], data["tab"], w_want, dt)
    torch.cuda.synchronize()
    assert torch.equal(got["theta"].reshape(-1).view(torch.int32), ops["theta"][:N].view(torch.int32))
    view = torch.int32 if dt == F32 else torch.int16
    assert torch.equal(got["w_fwd"].reshape(-1).view(view), w_want.view(view)) and not torch.equal(w_want, copy)
    assert "fb_mt_landscape_point" in cases._DECLARED


def test_landscape_point_without_a_table_is_confined():
    ops = _operands(N, 6)
    data = {k: ops[k][:N].clone() for k in ("base", "dx", "dy")}
    data["xy"] = torch.tensor(XY, device="cuda", dtype=F32)

    def fn(o):
        cases._call("fb_mt_landscape_point", o["theta"], o["base"], o["dx"], o["dy"], N, o["xy"], None, 0, None, 0)

    got = confined(fn, inputs=data, outputs=dict(theta=((N,), F32)))
    _launch(ops, N, data["xy"], None, None, F32)
    torch.cuda.synchronize()
    assert torch.equal(got["theta"].reshape(-1).view(torch.int32), ops["theta"][:N].view(torch.int32))
