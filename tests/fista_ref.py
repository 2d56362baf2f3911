"""Float32 numpy restatement of the reference's ``FISTA.step`` (additional_optimizers/fista.py:44-82, projection None) and of the clip in front
of it, the yardstick of ``fb_mt_fista``: every operation is one numpy float32 operation, rounded on its own, in the order the reference's tensor
arithmetic has them.  tests/test_cpu_fista.py holds it against recorded steps of the reference itself (tests/golden/fista_optimizer.npz) bit for
bit; the GPU tests hold the kernel against it bit for bit -- there is no tolerance anywhere.

    x+    = param - grad * lr
    tk'   = (p + sqrt(q + r * tk * tk)) / 2         fista_mod = (p, q, r) cast to float32 first
    ak    = (tk - 1) / tk'
    param = x+ * (1 + ak) - x- * ak
    x-    = x+ ;  tk = tk'
"""
import numpy as np

F = np.float32


def coefficients_ref(tk, fista_mod):
    """One advance of the overrelaxation sequence: (tk', ak, 1 + ak), numpy.float32 each, every operation correctly rounded (IEEE).  The
    reference's torch expression agrees except in ``sqrt``, which torch's CPU kernel rounds faithfully but not always correctly: from one
    ``tk`` the two differ by at most 1 / 2 / 2 ulp (tests/test_cpu_fista.py), and the recorded steps of the reference are met bit for bit."""
    p, q, r = (F(v) for v in fista_mod)
    tk = F(tk)
    tk_new = (p + np.sqrt(q + r * (tk * tk), dtype=F)) / F(2)
    ak = (tk - F(1)) / tk_new
    return tk_new, ak, F(1) + ak


def clip_coef_f32(norm2, clip, torch_clip=False):
    """(coef as numpy.float32, hit) of the clip by the fp32 device scalar ``norm2``, in float32 the way the update kernels state it (the float64
    form is ``tests/helpers.clip_coef_ref`` / ``tests/adam_ref.torch_clip_coef_ref``): norm = sqrt(norm2), c = clip / (norm + 1e-6); the
    full-batch form takes c where norm > clip, ``clip_grad_norm_``'s form min(1, c).  ``clip`` None or negative: no clip."""
    if clip is None or clip < 0:
        return F(1), False
    norm = np.sqrt(F(norm2), dtype=F)
    c = F(clip) / (norm + F(1e-6))
    if torch_clip:
        return (c, True) if c < F(1) else (F(1), False)
    return (c, True) if norm > F(clip) else (F(1), False)


def fista_ref(theta, grad, x_minus, coef, lr, ak, one_plus_ak):
    """-> (theta', clipped gradient, x_minus') as float32 numpy arrays; inputs are float32 arrays, the scalars become float32 as they do when
    they are handed to the kernel.  The caller decides whether the clipped gradient is what the gradient buffer has to hold afterwards (the
    full-batch form with coef != 1) or the buffer has to keep its bits (every other case)."""
    theta, grad, x_minus = (np.asarray(a, dtype=F) for a in (theta, grad, x_minus))
    coef, lr, ak, one_plus_ak = F(coef), F(lr), F(ak), F(one_plus_ak)
    g = coef * grad if coef != F(1) else grad
    step = g * lr
    xp = theta - step
    a = xp * one_plus_ak
    b = x_minus * ak
    return a - b, g, xp


def reference_steps(p0, grads, lrs, fista_mod):
    """The reference's optimizer over several steps on one tensor from its first use (x- = p0, tk = 1): yields (param, x-, tk) after each."""
    p, xm, tk = np.asarray(p0, dtype=F), np.asarray(p0, dtype=F).copy(), F(1)
    for g, lr in zip(grads, lrs):
        tk, ak, opak = coefficients_ref(tk, fista_mod)
        p, _, xm = fista_ref(p, g, xm, F(1), lr, ak, opak)
        yield p, xm, tk
