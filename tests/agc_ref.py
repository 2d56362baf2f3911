"""float64 reference of ``fb_mt_agc_sgd`` (csrc/agc_sgd.hip) -- the reference's ``SGD_AGC.step`` after the global clip -- with ELEMENTWISE error
bounds in the style of ``tests/helpers.sgd_ref`` / ``tests/adam_ref.adamw_ref``, and the fp32 emulation of the kernel (its summation order
included) that tests/test_cpu_agc.py uses to show that the checker bites.  Works on flat fp32 / fp64 vectors of any device and on the kernel's
unit table: rows [offset, unit_len, n_units, clip_on], sorted by offset.  Host scalars enter ROUNDED TO fp32 (``f32r``), as the kernel receives
them.  Two constants are fp32 values EVEN IN THE REFERENCE'S float64 RUNS: ``eps`` and the floor 1e-6 enter ``SGD_AGC.step`` as
``torch.tensor(eps)`` / ``torch.tensor(1e-6)``, float32 scalars that type promotion widens; so they are ``f32r`` here whatever ``rounded`` says.
"""
import numpy as np
import torch

from tests.helpers import COEF_ROUNDINGS, U32, f32r

FLOOR = f32r(1e-6)


def unit_ids(rows, n, device="cpu"):
    """-> (uid [n] int64: the unit every element belongs to, -1 for elements in none; per unit: its length, its clip_on flag; its tensor)."""
    uid = torch.full((int(n),), -1, dtype=torch.int64, device=device)
    lens, clip_on, tensor_of, base = [], [], [], 0
    for r, (off, unit_len, units, on) in enumerate(rows):
        off, unit_len, units = int(off), int(unit_len), int(units)
        uid[off:off + unit_len * units] = base + torch.arange(units, device=device).repeat_interleave(unit_len)
        lens += [unit_len] * units
        clip_on += [bool(on)] * units
        tensor_of += [r] * units
        base += units
    return uid, torch.tensor(lens, device=device), torch.tensor(clip_on, device=device), torch.tensor(tensor_of, device=device)


WAVE_L = 1024            # AGC_WAVE_L of csrc/agc_sgd.hip: units up to this length are summed by one wave (64 threads), longer ones by 256 threads


def sum_roundings(unit_len):
    """Roundings on the longest path of the kernel's sum of squares of a unit: thread t of a team of T (64 up to WAVE_L floats, 256 above) adds the
    squares of its 16-byte chunks t, t + T, ... with one fma each (4 ceil(len / 4T) roundings, the products are exact inside the fma), then six
    levels of the butterfly and, for T = 256, three sums over the four waves.  All terms are >= 0, so the sum carries at most that many u,
    relative."""
    return 4 * ((unit_len + 255) // 256) + 6 if unit_len <= WAVE_L else 4 * ((unit_len + 1023) // 1024) + 9


def host_scalars(hyp, rounded=True):
    r = f32r if rounded else float
    damp = r(hyp.get("dampening", 0.0))
    clipping = hyp.get("clipping")
    return dict(lr=r(hyp["lr"]), wd=r(hyp["weight_decay"]), mu=r(hyp["momentum"]), damp=damp, nesterov=bool(hyp.get("nesterov", True)),
                omd=float(np.float32(1.0) - np.float32(damp)) if rounded else 1.0 - damp,
                clipping=None if clipping is None or clipping < 0 else r(clipping), eps=f32r(hyp.get("eps", 1e-3)))


def agc_ref(p, g, m, rows, coef, hit, hyp, first, rounded=True):
    """One update in float64 -> {"param" | "mom" | "grad": (reference, bound), "triggered": [units] bool, "near": [units] bool, "clipped": [units]
    bool (units the clip applies to)}.

    ``coef`` / ``hit``: the global clip coefficient in float64 and whether it scales (``helpers.clip_coef_ref``, or
    ``adam_ref.torch_clip_coef_ref`` for ``hyp["torch_clip"]``).  ``hyp``: lr, weight_decay, momentum, dampening, nesterov, clipping (None or < 0:
    none), eps, torch_clip.  ``m`` may be None with momentum 0.  Elements in no unit keep their values, bound 0.

    The kernel, u = 2^-24 per rounding:
        g'   = fl(coef g)                            only where the global clip hits (otherwise the bits of g); coef carries COEF_ROUNDINGS u
        pn   = max(sqrtf(SUM p^2), eps);  gn = sqrtf(SUM g'^2);  maxn = fl(pn clipping);  f = fl(maxn / max(gn, 1e-6))   where gn > maxn
        d    = fl(g' f)                              where the unit triggers, else g'
        then the update of fb_mt_clip_sgd on d:  d1 = fl(wd p + d); buf = fl((1 - damp) d1 + fl(mu m)); d2 = fl(mu buf + d1); p' = fl(p - lr d2)
    The factor f, relative: SUM is a sum of non-negative terms with R = sum_roundings(len) roundings on its longest path, the root halves a relative
    error and adds its own: pn and gn carry (R / 2 + 1) u each, gn also the error of g' (u + COEF_ROUNDINGS u where the global clip hits: the root
    of a sum of squares is homogeneous of degree 1); the product with clipping and the division add one each.  With one more of slack:
        delta = (R + 5 + [hit] (1 + COEF_ROUNDINGS)) u.
    A unit is NEAR the trigger when |gn / maxn - 1| <= delta: the kernel may have taken either branch.  Both give d within |g'| |r - 1| of each
    other (r = maxn / max(gn, 1e-6), which is within delta of 1 there: the update is continuous across the trigger), so the same comparison
    covers the unit with
        E_d = |g'| (|r - 1| + delta + u) + E_g             near
        E_d = |g' r| (delta + u) + r E_g                   triggered, not near            E_d = E_g     not triggered, not near (the bits of g')
    where E_g = u |g'| + COEF_ROUNDINGS u |g'| is the error g' arrives with (0 without a global clip).  E_d then passes through the update like
    the allowance on coef does in ``sgd_ref``: momentum 4 u S + E_d, parameters u (|p| + |p'| + 8 lr S) + lr (1 + mu) E_d, S = |d| + wd |p| +
    mu |m|.  grad: (g', E_g) where the full-batch clip hit (written back: the global clip only, never the unit clip), else the bits of g."""
    h = host_scalars(hyp, rounded)
    n = p.numel()
    uid, lens, clip_on, _ = unit_ids(rows, n, p.device)
    cov = uid >= 0
    p64, g64 = p.double(), g.double()
    m64 = m.double() if m is not None else torch.zeros_like(p64)
    cg = g64 * coef
    Eg = (1 + COEF_ROUNDINGS) * U32 * cg.abs() if hit else torch.zeros_like(cg)
    nu = lens.numel()
    idx = uid[cov]
    clipped = clip_on & (h["clipping"] is not None)
    r_elem, Ed = torch.ones_like(cg), Eg.clone()
    triggered = torch.zeros(nu, dtype=torch.bool, device=p.device)
    near = torch.zeros_like(triggered)
    if h["clipping"] is not None:
        sp = torch.zeros(nu, dtype=torch.float64, device=p.device).index_add_(0, idx, p64[cov] ** 2)
        sg = torch.zeros(nu, dtype=torch.float64, device=p.device).index_add_(0, idx, cg[cov] ** 2)
        pn, gn = sp.sqrt().clamp(min=h["eps"]), sg.sqrt()
        maxn = pn * h["clipping"]
        r = maxn / gn.clamp(min=FLOOR)
        triggered = (gn > maxn) & clipped
        R = torch.where(lens <= WAVE_L, 4 * ((lens + 255) // 256) + 6, 4 * ((lens + 1023) // 1024) + 9)          # sum_roundings(len)
        delta = (R.double() + 5 + ((1 + COEF_ROUNDINGS) if hit else 0)) * U32
        near = ((gn / maxn - 1).abs() <= delta) & clipped
        f_unit = torch.where(triggered, r, torch.ones_like(r))
        r_elem[cov] = f_unit[idx]
        far_trig = triggered & ~near
        e_near = cg.abs()[cov] * ((r - 1).abs() + delta + U32)[idx] + Eg[cov]
        e_trig = (cg.abs()[cov] * r[idx]) * (delta + U32)[idx] + r[idx] * Eg[cov]
        Ed[cov] = torch.where(near[idx], e_near, torch.where(far_trig[idx], e_trig, Eg[cov]))
    d = cg * r_elem
    write_back = hit and not hyp.get("torch_clip", False)
    out = {"triggered": triggered, "near": near, "clipped": clipped}
    grad_ref, grad_b = (cg.clone(), Eg.clone()) if write_back else (g64.clone(), torch.zeros_like(g64))
    grad_ref[~cov], grad_b[~cov] = g64[~cov], 0.0
    out["grad"] = (grad_ref, grad_b)
    S = d.abs() + h["wd"] * p64.abs()
    d1 = d + h["wd"] * p64
    if h["mu"] != 0.0:
        if first:
            buf = d1
        else:
            buf = h["mu"] * m64 + (1.0 - h["damp"]) * d1
            S = S + h["mu"] * m64.abs()
        mom_b = 4 * U32 * S + Ed
        buf = torch.where(cov, buf, m64)
        mom_b[~cov] = 0.0
        out["mom"] = (buf, mom_b)
        d1 = d1 + h["mu"] * buf if h["nesterov"] else buf
    pn_ = p64 - h["lr"] * d1
    par_b = U32 * (p64.abs() + pn_.abs() + 8 * h["lr"] * S) + h["lr"] * (1 + h["mu"]) * Ed
    pn_ = torch.where(cov, pn_, p64)
    par_b[~cov] = 0.0
    out["param"] = (pn_, par_b)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a b + c) of fp32 arrays: the product of two fp32 values is exact in double, the sum is rounded once more there."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_sumsq(x):
    """The kernel's sum of squares of one unit (fp32 numpy vector) in its order: a team of T threads (64 up to WAVE_L floats, else 256), thread t
    takes the chunks of four t, t + T, ..., one fma per element in address order; per wave the xor butterfly 32, 16, ..., 1; for T = 256 the
    four wave sums as ((s0 + s1) + s2) + s3."""
    n = x.shape[0]
    T = 64 if n <= WAVE_L else 256
    iters = (n + 4 * T - 1) // (4 * T)
    buf = np.zeros(iters * 4 * T, dtype=np.float32)
    buf[:n] = x
    buf = buf.reshape(iters, T, 4)
    acc = np.zeros(T, dtype=np.float32)
    for it in range(iters):
        for j in range(4):
            acc = _fma(buf[it, :, j], buf[it, :, j], acc)
    thread = np.arange(T)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[thread ^ off]).astype(np.float32)
    waves = acc.reshape(-1, 64)
    assert np.all(waves == waves[:, :1])
    total = waves[0, 0]
    for w in range(1, T // 64):
        total = np.float32(total + waves[w, 0])
    return total


def emulate_fp32(p, g, m, rows, norm2, clip, hyp, first, plant=None):
    """The kernel's operations in its order in fp32 (fp32 CPU tensors in) -> dict(param, grad, mom).  ``clip``: None or the global threshold; the
    coefficient is formed in fp32 from ``norm2`` like the kernel does.  ``plant``: one of the errors tests/test_cpu_agc.py plants."""
    f = np.float32
    h = {k: (f(v) if isinstance(v, float) else v) for k, v in host_scalars(hyp).items()}
    p, g = p.numpy().astype(f), g.numpy().astype(f)
    m = np.zeros_like(p) if m is None else m.numpy().astype(f)
    torch_clip = bool(hyp.get("torch_clip", False))
    coef = f(1.0)
    if clip is not None:
        norm = np.sqrt(f(norm2))
        c = f(clip) / (norm + f(1e-6))
        if torch_clip:
            coef = min(c, f(1.0))
        elif norm > f(clip):
            coef = c
    scaled = float(coef) != 1.0
    gp = (coef * g).astype(f) if scaled else g.copy()
    po, mo, go = p.copy(), m.copy(), g.copy()
    for off, unit_len, units, on in rows:
        whole = slice(off, off + unit_len * units)
        for k in range(units):
            s = slice(off + k * unit_len, off + (k + 1) * unit_len)
            pu, gu, mu_ = p[s], gp[s], m[s]
            d = gu
            if plant == "agc-after-weight-decay":
                d = _fma(np.full_like(pu, h["wd"]), pu, d)
            if on and h["clipping"] is not None:
                sp, sg = (kernel_sumsq(p[whole]), kernel_sumsq(gp[whole])) if plant == "whole-tensor-norm" else (kernel_sumsq(pu), kernel_sumsq(d if plant == "agc-after-weight-decay" else gu))
                pn = np.sqrt(sp) if plant == "no-eps-floor" else max(np.sqrt(sp), h["eps"])
                gn = np.sqrt(sg)
                maxn = f(pn * h["clipping"])
                if gn > maxn or plant == "trigger-ignored":
                    d = (d * f(maxn / max(gn, f(1e-6)))).astype(f)
            if plant == "clipped-gradient-written-back":
                go[s] = d
            elif scaled and not torch_clip:
                go[s] = gu
            if plant != "agc-after-weight-decay":
                d = _fma(np.full_like(pu, h["wd"]), pu, d)
            if float(h["mu"]) != 0.0:
                buf = d if first else _fma(np.full_like(d, h["omd"]), d, (h["mu"] * mu_).astype(f))
                mo[s] = buf
                d = _fma(np.full_like(d, h["mu"]), buf, d) if h["nesterov"] else buf
            po[s] = _fma(np.full_like(d, -h["lr"]), d, pu)
    return dict(param=torch.from_numpy(po), grad=torch.from_numpy(go), mom=torch.from_numpy(mo))
