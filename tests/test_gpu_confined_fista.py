"""The confinement case of the FISTA update (csrc/fista.hip: ``fb_mt_fista``), filed with the cases of tests/test_gpu_confinement.py through that
file's own ``_call``, so that its completeness check -- every launch entry point of the library has a case that ran inside ``helpers.confined`` --
counts the entry point; this file sorts, and therefore runs, before it.  Guard bands around every operand, three fills, both clip forms, n = 4099
with the operands 1 float off a 16-byte boundary (scalar head and tail next to the guards): reads and writes confined, the norm unchanged (and
the gradient, in the torch form), results independent of what surrounds the operands and equal, bit for bit, to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests.helpers import confined, f32r
from tests.test_gpu_fista_kernel import _AK3, NAMES, _carve, _launch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("torch_clip", [False, True], ids=["full-batch-clip", "torch-clip"])
def test_fista_entry_point_is_confined(torch_clip):
    n, lr = 4099, 0.1
    ops = _carve(n, (0,) * 3)
    data = {k: torch.cat([torch.zeros(1, device="cuda"), ops[k][:n]]) for k in NAMES}          # the operand starts at element 1 of its slab: 4 bytes off
    gnorm2 = ops["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)

    def fn(o):
        cases._call("fb_mt_fista", *[o[k].data_ptr() + 4 for k in NAMES], n, o["gnorm2"], clip, 1 if torch_clip else 0, lr, float(_AK3),
                    float(1 + _AK3))

    inputs, inout = dict(gnorm2=gnorm2), {k: data[k] for k in NAMES}
    if torch_clip:                               # the gradient is read only
        inputs["grad"] = inout.pop("grad")
    out = confined(fn, inputs=inputs, outputs={}, inout=inout)
    _launch(ops, n, gnorm2, clip, torch_clip, lr, _AK3)
    torch.cuda.synchronize()
    for k in inout:
        got = out[k].reshape(-1)
        assert float(got[0]) == 0.0, k          # the element in front of the range is not the kernel's
        assert torch.equal(got[1:].view(torch.int32), ops[k][:n].view(torch.int32)), k
    assert "fb_mt_fista" in cases._DECLARED
