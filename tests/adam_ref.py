"""float64 reference of ``fb_mt_adamw`` (csrc/adamw.hip) -- ``torch.optim.AdamW``, single-tensor form, amsgrad=False -- with ELEMENTWISE error
bounds in the style of ``tests/helpers.sgd_ref``, and the fp32 emulation of the kernel that tests/test_cpu_adam.py uses to show that the
checker bites.  Works on tensors of any device.  Host scalars enter ROUNDED TO fp32 (``f32r``), as the kernel receives them; the two bias
corrections are formed in double from the update count ``t`` first, like ``Engine.adamw_step`` does.
"""
import math

import numpy as np
import torch

from tests.helpers import COEF_ROUNDINGS, U32, f32r

DEN = 2.0 ** -149        # spacing of fp32 in the denormal range: a rounding there is absolute, not relative


def host_scalars(hyp, t, rounded=True):
    """What the kernel computes with: every scalar as the fp32 value it arrives as; 1 - beta as the kernel forms it (one fp32 subtraction).
    ``rounded=False``: the scalars as they are (the plain float64 formulas of torch.optim.AdamW)."""
    if not rounded:
        b1, b2 = float(hyp["betas"][0]), float(hyp["betas"][1])
        return dict(lr=float(hyp["lr"]), wd=float(hyp["weight_decay"]), b1=b1, b2=b2, eps=float(hyp["eps"]), omb1=1.0 - b1, omb2=1.0 - b2,
                    step_size=float(hyp["lr"]) / (1.0 - b1 ** t), bc2s=math.sqrt(1.0 - b2 ** t))
    b1, b2 = f32r(hyp["betas"][0]), f32r(hyp["betas"][1])
    return dict(lr=f32r(hyp["lr"]), wd=f32r(hyp["weight_decay"]), b1=b1, b2=b2, eps=f32r(hyp["eps"]),
                omb1=float(np.float32(1.0) - np.float32(b1)), omb2=float(np.float32(1.0) - np.float32(b2)),
                step_size=f32r(float(hyp["lr"]) / (1.0 - float(hyp["betas"][0]) ** t)), bc2s=f32r(math.sqrt(1.0 - float(hyp["betas"][1]) ** t)))


def adamw_ref(p, g, m, v, coef, hit, hyp, t, rounded=True):
    """One update, number ``t`` (>= 1), in float64 -> {"param" | "exp_avg" | "exp_avg_sq" | "grad": (reference, bound)}.

    ``coef`` / ``hit``: the clip coefficient in float64 and whether it scales (``helpers.clip_coef_ref`` for the full-batch form; for
    ``hyp["torch_clip"]`` the form of ``clip_grad_norm_``, min(1, clip / (norm + 1e-6)), hit = coef < 1).  ``hyp``: lr, weight_decay, betas, eps,
    torch_clip (default False).  ``rounded=False``: host scalars in double (to compare the formulas with torch's own float64 AdamW).

    The kernel, u = 2^-24 per rounding:
        g' = fl(coef g)                                   (only where the clip hits; otherwise the bits of g)
        p1 = fl(p fl(1 - lr wd))                          2 roundings
        m' = fl((1 - b1) g' + fl(b1 m))                   the fma and one product; g' carries its own
        v' = fl(fl((1 - b2) g') g' + fl(b2 v))            the fma and two products; g' enters twice
        d  = fl(fl(sqrtf(v') / bc2s) + eps)               sqrt, division, sum: three roundings of non-negative partial results <= d
        p' = fl(p1 - step_size fl(m' / d))                the division and the fma
    Bounds = u x the terms x the roundings on the longest path, as in ``sgd_ref``:
      * grad (full-batch form, hit): u |g'| + ce with ce = COEF_ROUNDINGS u |g'|, the allowance on coef; otherwise 0: the bits of g.
      * exp_avg: with S = (1 - b1) |g'| + b1 |m|: 3 u S (g', the product, the fma) + (1 - b1) ce.
      * exp_avg_sq: a sum of NON-NEGATIVE terms, so the error is relative: the first term carries g' twice, its product and the fma (4 u), the
        second its product and the fma: (4 + 2 COEF_ROUNDINGS [hit]) u v'.
      * both: + 3 DEN, because a rounding in the denormal range is absolute (2^-149 apart).
      * param: 2 u |p1| + u |p'| + step_size E_q, where q = m' / d carries its own rounding, the error of m' divided by d, and the error of d:
            E_q = |q| (u + E_d / d) + E_m / d,   E_d = 3 u d + (sqrt(v') - sqrt(max(v' - E_v, 0))) / bc2s
        (the square root written as a difference, not as E_v / (2 sqrt(v')): v' may be 0 or denormal while eps dominates d).
        So the error of m reaches p multiplied by step_size / d, that of v by step_size |q| / d times the slope of the root."""
    h = host_scalars(hyp, t, rounded)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    cg = g * coef
    ce = COEF_ROUNDINGS * U32 * cg.abs() if hit else torch.zeros_like(cg)
    write_back = hit and not hyp.get("torch_clip", False)
    out = {"grad": (cg, U32 * cg.abs() + ce) if write_back else (g, torch.zeros_like(g))}
    p1 = p * (1.0 - h["lr"] * h["wd"])
    mn = h["omb1"] * cg + h["b1"] * m
    Em = 3 * U32 * (h["omb1"] * cg.abs() + h["b1"] * m.abs()) + h["omb1"] * ce + 3 * DEN
    vn = h["omb2"] * cg * cg + h["b2"] * v
    Ev = (4 + (2 * COEF_ROUNDINGS if hit else 0)) * U32 * vn + 3 * DEN
    d = vn.sqrt() / h["bc2s"] + h["eps"]
    Ed = 3 * U32 * d + (vn.sqrt() - (vn - Ev).clamp_(min=0).sqrt()) / h["bc2s"]
    q = mn / d
    Eq = q.abs() * (U32 + Ed / d) + Em / d
    pn = p1 - h["step_size"] * q
    out["exp_avg"], out["exp_avg_sq"] = (mn, Em), (vn, Ev)
    out["param"] = (pn, 2 * U32 * p1.abs() + U32 * pn.abs() + h["step_size"] * Eq)
    return out


def torch_clip_coef_ref(norm2, clip):
    """(coef, hit) of ``clip_grad_norm_`` from the fp32 device scalar ``norm2``, in float64: min(1, clip / (norm + 1e-6))."""
    if clip is None or clip < 0:
        return 1.0, False
    norm = float(np.sqrt(np.float64(np.float32(norm2))))
    coef = min(1.0, f32r(clip) / (norm + f32r(1e-6)))
    return coef, coef < 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
def _r32(x64):
    return x64.to(torch.float32)


def _fma(a, b, c):
    """fl32(a b + c) of fp32 tensors / scalars: the product of two fp32 values is exact in double, the sum is rounded once more there."""
    return _r32(torch.as_tensor(a).double() * torch.as_tensor(b).double() + torch.as_tensor(c).double())


def emulate_fp32(p, g, m, v, norm2, clip, hyp, t, plant=None):
    """The kernel's operations in its order in fp32 torch ops (fp32 CPU tensors in, fp32 out) -> dict(param, grad, exp_avg, exp_avg_sq).
    ``clip``: None or the threshold; the coefficient is formed in fp32 from ``norm2`` like the kernel does.  ``plant``: one of the errors
    tests/test_cpu_adam.py plants."""
    f32 = torch.float32
    h = {k: torch.tensor(x, dtype=f32) for k, x in host_scalars(hyp, t).items()}
    torch_clip = bool(hyp.get("torch_clip", False))
    if plant == "other-clip-form":
        torch_clip = not torch_clip
    coef = torch.tensor(1.0, dtype=f32)
    if clip is not None:
        norm = torch.tensor(norm2, dtype=f32).sqrt()
        c = torch.tensor(clip, dtype=f32) / (norm + torch.tensor(1e-6, dtype=f32))
        if torch_clip:
            coef = torch.minimum(c, torch.tensor(1.0, dtype=f32))
        elif bool(norm > torch.tensor(clip, dtype=f32)):
            coef = c
    scaled = float(coef) != 1.0
    gp = coef * g if scaled else g.clone()
    decay = _fma(-h["lr"], h["wd"], torch.tensor(1.0, dtype=f32))
    p1 = p * decay
    mn = _fma(h["omb1"], gp, h["b1"] * m)
    if plant == "beta2-on-g":
        vn = _fma(h["omb2"], gp, h["b2"] * v)
    else:
        vn = _fma(h["omb2"] * gp, gp, h["b2"] * v)
    bc2s = torch.tensor(1.0, dtype=f32) if plant == "no-bias-correction-2" else h["bc2s"]
    if plant == "eps-inside-sqrt":
        d = (vn + h["eps"]).sqrt() / bc2s
    else:
        d = vn.sqrt() / bc2s + h["eps"]
    q = mn / d
    if plant == "decay-after-step":
        pn = _fma(-h["step_size"], q, p) * decay
    else:
        pn = _fma(-h["step_size"], q, p1) if float(h["step_size"]) != 0.0 else p1
    return dict(param=pn, grad=gp if (scaled and not torch_clip) else g.clone(), exp_avg=mn, exp_avg_sq=vn)


def describe(obj):
    """Key structure of a checkpoint part: tensors as shape + dtype, long lists as length + first entry (tests/golden/make_golden_adam.py records
    the reference's own with it; tests/test_gpu_adam_training.py compares the engine's)."""
    if torch.is_tensor(obj):
        return {"tensor": list(obj.shape), "dtype": str(obj.dtype)}
    if isinstance(obj, dict):
        return {str(k): describe(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [describe(v) for v in obj] if len(obj) < 8 else {"list_len": len(obj), "first": describe(obj[0])}
    return repr(obj) if not isinstance(obj, (int, float, bool, type(None), str)) else obj
