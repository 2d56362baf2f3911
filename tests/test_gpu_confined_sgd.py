"""The confinement case of the mini-batch SGD update (csrc/sgd_prep.hip: ``fb_mt_sgd_prep``, ``fb_mt_sgd_torch``), filed with the cases of
tests/test_gpu_confinement.py through that file's own ``_call``, so that its completeness check -- every launch entry point of the library has
a case that ran inside ``helpers.confined`` -- counts the two entry points; this file sorts, and therefore runs, before it.  Guard bands around
every operand, three fills: reads and writes confined, the gradient, the norm and the layer table unchanged, results independent of what
surrounds the operands and equal to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests.helpers import confined
from tests.test_gpu_sgd_kernel import BF16, F32, _bits, _copies, _hyp_args, _lib, _prepare, _run_fused

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_sgd_update_entry_points_are_confined(dtype):
    lib = _lib()
    s, h = _prepare("synthetic", dtype, "clip-far-below-norm-plain-momentum")
    wf0, wd0 = _copies(s)
    code = lib.dtype_code(dtype)
    out = confined(lambda o: cases._call("fb_mt_sgd_prep", o["theta"], o["grad"], o["mom"], s["n"], o["gnorm2"], *_hyp_args(h), o["tab"], len(s["rows"]),
                                         o["w_fwd"], o["w_dgrad"], code),
                   inputs=dict(grad=s["grad"], gnorm2=s["gnorm2"], tab=s["tab"]), outputs={},
                   inout=dict(theta=s["theta"], mom=s["mom"], w_fwd=wf0, w_dgrad=wd0))
    want = _run_fused(s, h)
    for name, ref in zip(("theta", "mom", "w_fwd", "w_dgrad"), want):
        assert torch.equal(_bits(out[name].reshape(-1)), _bits(ref)), name
    out = confined(lambda o: cases._call("fb_mt_sgd_torch", o["theta"], o["grad"], o["mom"], s["n"], o["gnorm2"], *_hyp_args(h)),
                   inputs=dict(grad=s["grad"], gnorm2=s["gnorm2"]), outputs={}, inout=dict(theta=s["theta"], mom=s["mom"]))
    assert torch.equal(_bits(out["theta"].reshape(-1)), _bits(want[0])) and torch.equal(_bits(out["mom"].reshape(-1)), _bits(want[1]))
    assert {"fb_mt_sgd_prep", "fb_mt_sgd_torch"} <= cases._DECLARED
