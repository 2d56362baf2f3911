"""Restatements of the three line-search kernels (csrc/wolfe.hip: fb_mt_wolfe_direction, fb_mt_wolfe_trial, fb_mt_wolfe_phi_grad).

``*_f32`` (numpy): the float32 arithmetic operation by operation, every product-and-sum ONE fused multiply-add -- the form of torch's
``add(other, alpha=)`` on a CPU with FMA units and of the kernels.  Held bit for bit to recorded steps of the reference
(tests/golden/wolfe_optimizer.npz) by tests/test_cpu_wolfe.py.  ``fma`` is emulated in double: the product of two float32 is exact there, the
sum is rounded to 53 bits and then to 24, which differs from one rounding only where the 53-bit sum lands exactly on a float32 tie (about one
operation in 2^29).

``*_f64`` (torch, any device): the same expressions in float64 with the elementwise bound each float32 result is allowed, in the style of
tests/adam_ref.py: ``k u (sum of the magnitudes of the terms)`` with u = 2^-24 and k counted from the roundings on the longest path:

  d    = fma(wd, theta, g)                       1 rounding                                   S_d   = |g| + wd |theta|
  mom' = fma(1 - damp, d, round(mu mom))         d, 1 - damp, mu mom, the fma: 4              S_buf = (1 - damp) S_d + mu |mom|      (first step: d, 1)
  p    = -fma(mu, mom', d)    (Nesterov)         mom' (4), d (1), the fma: 6                  S_p   = S_d + mu S_buf
         -mom'                (heavy ball)       4                                            S_p   = S_buf
         -d                   (mu = 0)           1                                            S_p   = S_d
  theta = fma(step, p, theta0)                   1 rounding                                   |theta0| + |step p|

The reductions: a term a_i b_i passes through at most L + 10 roundings, L = the lane's chain of fused multiply-adds (4 per 16-byte vector and pass
of the grid-stride loop, + 1 for a trailing element), 6 levels of the wave's shuffle tree, 3 additions across the four waves, the cast of the
double second stage (whose own error, 2^-53 per addition, is nothing) -- and the factor a_i = d_i arrives with 1 rounding, in the direction pass
b_i = p_i with k_p more.  So |got - sum a_i b_i| <= c u sum S_d,i S_p,i with c = L + 10 + 1 (+ k_p), ``phi_c``; (1 + u)^c - 1 <= 1.001 c u for
every c below 10^4, which the factor SLACK covers.

The magnitude is sum S_d,i S_p,i, not sum |a_i b_i| of the computed factors: the two are equal unless g_i and wd theta_i cancel (or, in the
direction pass, the terms of p_i do), and where they cancel the rounding of a_i = fma(wd, theta_i, g_i) is relative to S_d,i, not to |a_i|, so a
bound in |a_i b_i| alone would not hold for a correct kernel.  For wd = 0 and an input p (fb_mt_wolfe_phi_grad without decay) it IS
sum |a_i b_i|.  The golden generator's margin rule uses sum |a_i b_i| of the reference's own factors with the same constant; see there."""
import numpy as np
import torch

U32 = 2.0 ** -24
SLACK = 1.001
K_MOM, K_P = 4, {"nesterov": 6, "heavy-ball": 4, "none": 1}


def f32(x):
    return np.float32(x)


def fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def direction_f32(theta, g, mom, wd, mu, damp, nesterov, first):
    """-> (mom' | None, p, d) as float32 arrays; the scalars are rounded to float32 as a kernel argument is, 1 - damp is formed in float32."""
    wd, mu, omd = f32(wd), f32(mu), f32(1) - f32(damp)
    d = fma32(wd, theta, g)
    if mu == 0:
        return None, -d, d
    buf = d.copy() if first else fma32(omd, d, mu * mom.astype(np.float32))
    return buf, -(fma32(mu, buf, d) if nesterov else buf), d


def trial_f32(theta0, p, lr, alpha, form="fma"):
    step = f32(float(lr) * float(alpha))
    return fma32(step, p, theta0) if form == "fma" else theta0 + step * p


def phi_grad_terms_f32(theta, g, p, wd):
    """The float32 factors (d, p) of phi' = sum d p (the order of the sum is the kernel's, or torch's: a bound holds it, not bits)."""
    return fma32(f32(wd), theta, g), p


def chain_length(n, vec, block, max_blocks):
    n4 = n // vec
    nb = max(1, min(max_blocks, -(-n4 // block)))
    return vec * -(-n4 // (nb * block)) + (1 if n % vec else 0)


def phi_c(n, direction=False, mode="nesterov", vec=4, block=256, max_blocks=1024):
    """The constant of the reduction bound for a launch over n floats (see the module docstring)."""
    return chain_length(n, vec, block, max_blocks) + 10 + 1 + (K_P[mode] if direction else 0)


def _r(x):
    return float(np.float32(x))


def direction_f64(theta, g, mom, wd, mu, damp, nesterov, first):
    """-> dict: mom, p = (reference, bound) tensors (mom only for mu != 0); dphi = (sum d p, sum S_d S_p), python floats; mode."""
    wd, mu, damp = _r(wd), _r(mu), _r(damp)
    theta, g = theta.double(), g.double()
    d, S_d = g + wd * theta, g.abs() + wd * theta.abs()
    out = {}
    if mu == 0:
        mode, p, S_p = "none", -d, S_d
    else:
        if first:
            buf, S_buf, k = d, S_d, 1
        else:
            buf, S_buf, k = (1.0 - damp) * d + mu * mom.double(), (1.0 - damp) * S_d + mu * mom.double().abs(), K_MOM
        out["mom"] = (buf, k * U32 * SLACK * S_buf)
        mode = "nesterov" if nesterov else "heavy-ball"
        p, S_p = (-(d + mu * buf), S_d + mu * S_buf) if nesterov else (-buf, S_buf)
    out["p"] = (p, K_P[mode] * U32 * SLACK * S_p)
    out["dphi"] = (float((d * p).sum()), float((S_d * S_p).sum()))
    out["mode"] = mode
    return out


def trial_f64(theta0, p, lr, alpha):
    step = _r(float(lr) * float(alpha))
    t = theta0.double() + step * p.double()
    return t, U32 * SLACK * (theta0.double().abs() + (step * p.double()).abs())


def phi_grad_f64(theta, g, p, wd):
    """-> (sum (g + wd theta) p, sum S_d |p|), python floats."""
    wd = _r(wd)
    theta, g, p = theta.double(), g.double(), p.double()
    return float(((g + wd * theta) * p).sum()), float(((g.abs() + wd * theta.abs()) * p.abs()).sum())
