"""The confinement case of the AdamW update (csrc/adamw.hip: ``fb_mt_adamw``), filed with the cases of tests/test_gpu_confinement.py through that
file's own ``_call``, so that its completeness check -- every launch entry point of the library has a case that ran inside ``helpers.confined`` --
counts the entry point; this file sorts, and therefore runs, before it.  Guard bands around every operand, three fills, both clip forms, operands
1 float off a 16-byte boundary and n % 4 != 0 (scalar head and tail next to the guards): reads and writes confined, the norm unchanged (and the
gradient, in the torch form), results independent of what surrounds the operands and equal to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests import adam_ref
from tests.helpers import confined, f32r
from tests.test_gpu_adam_kernel import HYP, NAMES, _carve, _launch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("torch_clip", [False, True], ids=["full-batch-clip", "torch-clip"])
def test_adamw_entry_point_is_confined(torch_clip):
    n = 64 * 1024 + 7
    hyp = dict(HYP, torch_clip=torch_clip)
    ops = _carve(n, (0,) * 4)
    data = {k: torch.cat([torch.zeros(1, device="cuda"), ops[k][:n]]) for k in NAMES}          # the operand starts at element 1 of its slab: 4 bytes off
    gnorm2 = ops["grad"][:n].double().pow(2).sum().float().reshape(1)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)
    hs = adam_ref.host_scalars(hyp, 7)

    def fn(o):
        cases._call("fb_mt_adamw", *[o[k].data_ptr() + 4 for k in NAMES], n, o["gnorm2"], clip, 1 if torch_clip else 0, hyp["lr"],
                    hyp["weight_decay"], hyp["betas"][0], hyp["betas"][1], hyp["eps"], hs["step_size"], hs["bc2s"])

    inputs, inout = dict(gnorm2=gnorm2), {k: data[k] for k in NAMES}
    if torch_clip:                               # the gradient is read only
        inputs["grad"] = inout.pop("grad")
    out = confined(fn, inputs=inputs, outputs={}, inout=inout)
    _launch(ops, n, gnorm2, clip, hyp, 7)
    torch.cuda.synchronize()
    for k in inout:
        got = out[k].reshape(-1)
        assert float(got[0]) == 0.0, k          # the element in front of the range is not the kernel's
        assert torch.equal(got[1:].view(torch.int32), ops[k][:n].view(torch.int32)), k
    assert "fb_mt_adamw" in cases._DECLARED
