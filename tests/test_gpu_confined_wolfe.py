"""The confinement cases of the line-search kernels (csrc/wolfe.hip: ``fb_mt_wolfe_direction``, ``fb_mt_wolfe_trial``, ``fb_mt_wolfe_phi_grad``),
filed with the cases of tests/test_gpu_confinement.py through that file's own ``_call``, so that its completeness check -- every launch entry point
of the library has a case that ran inside ``helpers.confined`` -- counts the entry points; this file sorts, and therefore runs, before it.  Guard
bands around every operand, three fills, n = 4099 (three trailing elements next to the guard): reads and writes confined, inputs unchanged, every
output element defined whatever it held before (p, theta0, the scalar; on the first step the momentum too), the workspace a scratch area, and
results equal, bit for bit, to the unconfined run."""
import pytest
import torch

import tests.test_gpu_confinement as cases
from tests.test_gpu_wolfe_kernel import CONFIGS, LR, _direction, _inputs, _lib
from tests.helpers import confined

pytestmark = pytest.mark.gpu

N = 4099
F32 = torch.float32


def _ws():
    return {"ws": ((_lib().load().fb_ws_mt_floats(1),), F32)}


@pytest.mark.parametrize("name", ["nesterov", "nesterov-first", "no-momentum-decay"])
def test_wolfe_direction_is_confined(name):
    mu, damp, nesterov, wd, first = cfg = CONFIGS[name]
    ops = _inputs(N, 5)
    data = {k: ops[k][:N].clone() for k in ("theta", "grad", "mom")}

    def fn(o):
        cases._call("fb_mt_wolfe_direction", o["theta"], o["grad"], o["mom"] if mu != 0 else None, o["p"], o["theta0"], N, wd, mu, damp,
                    1 if nesterov else 0, 1 if first else 0, o["out"], o["ws"])

    inputs, outputs, inout = dict(theta=data["theta"], grad=data["grad"]), dict(p=((N,), F32), theta0=((N,), F32), out=((1,), F32)), {}
    if mu == 0:
        inputs["mom"] = data["mom"]              # (not even passed)
    elif first:
        outputs["mom"] = ((N,), F32)             # the first step reads no momentum: whatever the buffer held
    else:
        inout["mom"] = data["mom"]
    got = confined(fn, inputs=inputs, outputs=outputs, inout=inout, scratch=_ws())
    _direction(ops, N, cfg)
    torch.cuda.synchronize()
    for k in list(outputs) + list(inout):
        want = ops[k][:1] if k == "out" else ops[k][:N]
        assert torch.equal(got[k].reshape(-1).view(torch.int32), want.view(torch.int32)), k
    assert "fb_mt_wolfe_direction" in cases._DECLARED


def test_wolfe_trial_is_confined():
    ops = _inputs(N, 6)
    data = dict(theta0=ops["theta"][:N].clone(), p=ops["grad"][:N].clone())

    def fn(o):
        cases._call("fb_mt_wolfe_trial", o["theta"], o["theta0"], o["p"], N, LR * 2.5)

    got = confined(fn, inputs=data, outputs=dict(theta=((N,), F32)))
    out = torch.empty(N, device="cuda")
    _lib().call("fb_mt_wolfe_trial", out.data_ptr(), data["theta0"].data_ptr(), data["p"].data_ptr(), N, LR * 2.5)
    torch.cuda.synchronize()
    assert torch.equal(got["theta"].reshape(-1).view(torch.int32), out.view(torch.int32))
    assert "fb_mt_wolfe_trial" in cases._DECLARED


def test_wolfe_phi_grad_is_confined():
    ops = _inputs(N, 7)
    data = dict(theta=ops["theta"][:N].clone(), grad=ops["grad"][:N].clone(), p=ops["grad2"][:N].clone())

    def fn(o):
        cases._call("fb_mt_wolfe_phi_grad", o["theta"], o["grad"], o["p"], N, 5e-4, o["out"], o["ws"])

    got = confined(fn, inputs=data, outputs=dict(out=((1,), F32)), scratch=_ws())
    out = torch.empty(1, device="cuda")
    _lib().call("fb_mt_wolfe_phi_grad", data["theta"].data_ptr(), data["grad"].data_ptr(), data["p"].data_ptr(), N, 5e-4, out.data_ptr(),
                ops["ws"].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(got["out"].reshape(-1).view(torch.int32), out.view(torch.int32))
    assert "fb_mt_wolfe_phi_grad" in cases._DECLARED
