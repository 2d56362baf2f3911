"""The confinement case of the GD-AGC update (csrc/agc_sgd.hip: ``fb_mt_agc_sgd``), filed with the cases of tests/test_gpu_confinement.py through
that file's own ``_call``, so that its completeness check -- every launch entry point of the library has a case that ran inside
``helpers.confined`` -- counts the entry point; this file sorts, and therefore runs, before it.  Guard bands around every operand, three fills,
both clip forms, operands 1 float off a 16-byte boundary, the unit table an input of its own; the gaps between the tensors (4 and 12 bytes) and
the elements behind the last unit are part of what must be left alone: reads and writes confined, the norm and the table unchanged (and the
gradient, in the torch form), results independent of what surrounds the operands and equal to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests.helpers import SENTINEL, confined, f32r
from tests.test_gpu_agc_kernel import HYP, MANY, NAMES, _carve, _gnorm2, _launch, _rows, _tab
from tests import agc_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("torch_clip", [False, True], ids=["full-batch-clip", "torch-clip"])
def test_agc_sgd_entry_point_is_confined(torch_clip):
    rows, n = _rows(MANY)
    n += 5
    hyp = dict(HYP, torch_clip=torch_clip)
    ops = _carve(rows, n)
    data = {k: torch.cat([torch.zeros(1, device="cuda"), ops[k][:n]]) for k in NAMES}          # the operand starts at element 1 of its slab: 4 bytes off
    gnorm2 = _gnorm2(ops, rows, n)
    clip = f32r(0.5 * float(gnorm2) ** 0.5)

    def fn(o):
        cases._call("fb_mt_agc_sgd", *[o[k].data_ptr() + 4 for k in NAMES], n, o["gnorm2"], clip, 1 if torch_clip else 0, hyp["lr"],
                    hyp["weight_decay"], hyp["momentum"], hyp["dampening"], 1, 0, hyp["clipping"], hyp["eps"], o["table"], len(rows))

    inputs, inout = dict(gnorm2=gnorm2, table=_tab(rows)), {k: data[k] for k in NAMES}
    if torch_clip:                               # the gradient is read only
        inputs["grad"] = inout.pop("grad")
    out = confined(fn, inputs=inputs, outputs={}, inout=inout)
    _launch(ops, n, _tab(rows), gnorm2, clip, hyp, False)
    torch.cuda.synchronize()
    gaps = agc_ref.unit_ids(rows, n, "cuda")[0] < 0
    assert int(gaps.sum()) >= 20
    for k in inout:
        got = out[k].reshape(-1)
        assert float(got[0]) == 0.0, k          # the element in front of the range is not the kernel's
        assert torch.equal(got[1:].view(torch.int32), ops[k][:n].view(torch.int32)), k
        assert bool((got[1:][gaps] == SENTINEL).all()), k
    assert "fb_mt_agc_sgd" in cases._DECLARED
