"""Golden vectors of the reference with ``hyp.optim.line_search=wolfe`` (``WolfeGradientDescent``, reference optimizers.py:29-30 ->
additional_optimizers/sgd_linesearch.py:183-381).

Runs the real reference on CPU through the harness of ``make_golden.py`` / ``make_golden_adam.py`` (imported, left as they are) and writes

  tests/golden/wolfe_search.npz      SEARCH CASES: the reference's optimizer on tiny analytic problems (one or two float64 tensors, closures
                                     built from quadratics of several curvatures and non-convex functions).  Per search: phi(0), phi'(0), every
                                     evaluated alpha in order with its (val, grad), the returned alpha, the last evaluated alpha -- or the type
                                     of the exception it ended with.  tests/test_cpu_wolfe.py replays them through training.WolfeSearch, exactly.
  tests/golden/wolfe_optimizer.npz   STEP VECTORS: the reference's direction, trial and phi' arithmetic in float32 on three small tensors plus one
                                     of 259 elements (long enough for the vectorised path of torch's CPU kernels), and which rounding form the
                                     trial points have (``trial_form``: ``fma`` or ``two-roundings``).
  tests/golden/scenarios_wolfe.npz   TRAINING SCENARIOS (``python make_golden_wolfe.py scenarios [NAME ...]``; named scenarios are measured alone and
                                     merged into the files): fp32 runs and ``@f64`` twins of the reference's own ``train()`` on ResNet-20 at 16 px,
                                     with a log per closure evaluation (alpha, loss, phi', sum |a_i b_i|) and both sides of every inequality the
                                     search decided.  tests/test_gpu_wolfe_training.py holds the engine to them.
  tests/golden/meta_wolfe.json       the tables, the coverage of the search cases, the reference's checkpoint key structure

COVERAGE of the search cases is asserted (the generator stops if an exit is missing): accepted at alpha = 1, rule-1 zoom, rule-2 zoom, growth to
alpha_max, outer max_iter exhausted, the zoom's 1e-4 exit, zoom exhausted (the returned alpha was never evaluated), a table hit, the ValueError
of a negative discriminant, phi'(0) > 0.  The cases have momentum 0 except ``uphill``: with p = -d, phi'(0) = -|d|^2 cannot be positive, so that
case takes two steps with heavy-ball momentum across a sign change of the gradient.  Each search is classified by replaying its record through
training.WolfeSearch, whose replay must reproduce the reference's evaluations and result exactly -- otherwise the generator stops.

ADMISSIBILITY of a training scenario, on top of ``make_golden_adam.py``'s spread rule; the generator stops after measuring every scenario:
  1. the fp32 and the float64 run of the reference take the identical alpha sequence;
  2. every inequality the search decided (replayed from the recorded values) is decided by a margin of at least 4 x the tolerance its operands
     are judged at: JUDGED_AT relative for losses; for phi' the LARGER of JUDGED_AT relative and phi_c * 2^-24 * sum |a_i b_i|, with
     a_i = g_i + wd theta_i as the reference formed it.  (tests/wolfe_ref.py bounds the kernels' reductions by the same constant times the looser
     sum (|g_i| + wd |theta_i|) |p_i|, which also covers the rounding of a_i itself; the two differ only where g_i and wd theta_i cancel, and
     either is four orders of magnitude below the JUDGED_AT term that decides the maximum in every recorded inequality.)
Learning rates and seeds are tried in the fixed order of LADDER; meta_wolfe.json keeps what every rung tried gave (``tried``).

Usage:  python tests/golden/make_golden_wolfe.py [scenarios]
"""
import fcntl
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_adam as mga  # noqa: E402
from make_golden_fista import OPT_SHAPES  # noqa: E402
from tests.adam_ref import describe  # noqa: E402  (make_golden put the repository root on the path)
from fullbatchtraining_amd.training import WolfeSearch  # noqa: E402

SPREAD_LIMIT, SPREAD_KEYS, NORM_KEYS, THREADS = mga.SPREAD_LIMIT, mga.SPREAD_KEYS, mga.NORM_KEYS, mga.THREADS

# ---------------------------------------------------------------------------------------------------------------------- search cases
# f(x) = sum_i f_i(x_i) over the elements of the tensors; (value, derivative) elementwise
FAMILIES = {
    "quad": lambda x, c: (0.5 * c * x * x, c * x),
    "quartic": lambda x, c: (0.25 * x ** 4 - 0.5 * c * x * x, x ** 3 - c * x),                     # double well
    "cosine": lambda x, c: (torch.cos(c * x) + 0.05 * x * x, -c * torch.sin(c * x) + 0.1 * x),     # many wells
    "kink": lambda x, c: (torch.sqrt(x * x + c), x / torch.sqrt(x * x + c)),                       # |x| smoothed: gradient saturates
}
DEFAULTS = dict(c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10)
# name: family, per-tensor (start values, per-element constants), lr, momentum, steps, overrides of the four search constants
SEARCH_CASES = {}


def case(name, family, x0, c, lr, momentum=0.0, steps=1, **constants):
    SEARCH_CASES[name] = dict(family=family, x0=x0, c=c, lr=lr, momentum=momentum, steps=steps, constants={**DEFAULTS, **constants})


case("accept", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 1.0)
case("accept_two_tensors", "quad", [[1.0, -2.0], [0.5]], [[1.0, 2.0], [0.5]], 0.6)
case("zoom1", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 3.0)
case("zoom1_curvatures", "quad", [[1.0, -2.0], [0.5, 3.0]], [[1.0, 10.0], [0.1, 4.0]], 0.5)
case("zoom2", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 1.96)
case("grow", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 0.01)
case("grow_then_accept", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 0.3)
case("outer_exhausted", "quad", [[1.0, -2.0, 0.5]], [[1.0, 1.0, 1.0]], 0.01, max_iter=2)
case("quartic_two_rounds", "quartic", [[0.3, -0.2]], [[1.0, 1.0]], 40.0, max_iter=2)
case("kink_sharp", "kink", [[1.0, -2.0]], [[1e-6, 1e-6]], 3.0)
case("quartic_far", "quartic", [[2.0, -1.5]], [[1.0, 2.0]], 1.0)
case("cosine", "cosine", [[0.4, -1.3, 2.2]], [[3.0, 5.0, 2.0]], 2.0)
case("cosine_far", "cosine", [[0.4, -1.3, 2.2]], [[3.0, 5.0, 2.0]], 8.0)
case("kink_far", "kink", [[1.0, -2.0]], [[1e-2, 1e-2]], 6.0)
case("uphill", "quad", [[1.0]], [[1.0]], 1.9, momentum=0.9, steps=3)
# (found by a sweep over the families with c1 in {1e-4, 0.1, 0.5}, c2 in {0.9, 0.1}: a large c1 keeps the zoom going where 1e-4 accepts at once)
case("interval_quad", "quad", [[0.44, -0.82]], [[0.1, 0.1]], 0.05, c1=0.5, c2=0.1)
case("interval_kink", "kink", [[1.14]], [[0.01]], 0.05, c1=0.5, c2=0.1)
case("discriminant_quartic", "quartic", [[-2.34]], [[2.0]], 0.7, c1=0.5, c2=0.1)
case("discriminant_kink", "kink", [[-0.96, 2.29]], [[2.0, 3.0]], 0.7, c1=0.5, c2=0.1)
case("hit_quad", "quad", [[-0.36, 1.14]], [[3.0, 0.1]], 1.0, c1=0.5, c2=0.1)
case("hit_quartic", "quartic", [[2.5]], [[5.0]], 1.0, c1=0.5)
# alpha = 1 lands exactly on the stationary point x = 0 (all numbers dyadic): phi'(1) = 0, d_2 = d_1, the interpolation returns alpha_high itself
case("hit_stationary", "quartic", [[0.75]], [[0.0625]], 2.0, c1=0.5)

COVERAGE = ("accepted at alpha = 1", "rule-1 zoom", "rule-2 zoom", "growth to alpha_max", "outer max_iter exhausted", "zoom 1e-4 exit",
            "zoom exhausted", "table hit", "ValueError", "phi'(0) > 0")


def run_search_case(wolfe_cls, spec):
    """-> one record per ``optimizer.step``: phi0 = (val, grad), evaluations [(alpha, val, grad)], returned alpha | None, exception name | None."""
    f = FAMILIES[spec["family"]]
    params = [torch.nn.Parameter(torch.tensor(x, dtype=torch.float64)) for x in spec["x0"]]
    consts = [torch.tensor(c, dtype=torch.float64) for c in spec["c"]]
    opt = wolfe_cls(params, lr=spec["lr"], momentum=spec["momentum"], **spec["constants"])
    records, log = [], {}

    def closure():
        total = 0.0
        for p, c in zip(params, consts):
            val, der = f(p.detach(), c)
            p.grad = der.clone()
            total = total + val.sum()
        return total

    inner = opt._evaluate_phi

    def logged(alpha, p_k_groups, closure, LUT_ref):
        fresh = alpha not in LUT_ref
        res = inner(alpha, p_k_groups, closure, LUT_ref)
        if fresh:
            log["evals"].append((alpha, *res))
        log["phi0"] = (LUT_ref[0]["val"], LUT_ref[0]["grad"])
        return res

    opt._evaluate_phi = logged
    for _ in range(spec["steps"]):
        log.clear()
        log["evals"] = []
        exc = None
        try:
            opt.step(closure)
        except Exception as e:      # noqa: BLE001  (the type is the record)
            exc = type(e).__name__
        records.append(dict(phi0=log.get("phi0"), evals=list(log["evals"]), returned=None if exc else opt.state["alpha"], exception=exc))
        if exc:
            break
    return records


def replay(record, constants):
    """The record through training.WolfeSearch -> (the controller after the search, returned alpha | None, exception name | None); raises if the
    controller asks for another alpha than the reference evaluated."""
    todo = list(record["evals"])
    ctl = WolfeSearch(**constants)

    def evaluate(alpha):
        want = todo.pop(0)
        assert alpha == want[0], (alpha, want)
        return want[1], want[2]

    try:
        got, exc = ctl.search(record["phi0"][0], record["phi0"][1], evaluate), None
    except Exception as e:          # noqa: BLE001
        got, exc = None, type(e).__name__
    assert not todo, ("the controller stopped early", todo)
    return ctl, got, exc


def classify(record, ctl, constants):
    tags = set()
    if record["exception"] == "ValueError":
        tags.add("ValueError")
    if record["phi0"][1] > 0:
        tags.add("phi'(0) > 0")
    if ctl.table_hits:
        tags.add("table hit")
    if record["exception"] is None:
        if ctl.exit == "accepted" and record["returned"] == 1.0:
            tags.add("accepted at alpha = 1")
        if ctl.exit == "alpha_max":
            tags.add("growth to alpha_max")
        if ctl.exit == "max_iter":
            tags.add("outer max_iter exhausted")
        if ctl.exit == "zoom-1":
            tags.add("rule-1 zoom")
        if ctl.exit == "zoom-2":
            tags.add("rule-2 zoom")
        if ctl.zoom_exit == "interval":
            tags.add("zoom 1e-4 exit")
        if ctl.zoom_exit == "exhausted" and record["returned"] not in [e[0] for e in record["evals"]]:
            tags.add("zoom exhausted")
    return tags


def search_cases(fullbatch, cases=None):
    wolfe_cls = fullbatch.training.optimizers.WolfeGradientDescent
    out, table, covered = {}, {}, set()
    for name, spec in (cases or SEARCH_CASES).items():
        for s, record in enumerate(run_search_case(wolfe_cls, spec)):
            if record["phi0"] is None:          # (the exception came before the first evaluation: nothing to replay)
                raise SystemExit(f"{name}: step {s} raised {record['exception']} before the search began")
            ctl, got, exc = replay(record, spec["constants"])
            if exc != record["exception"] or got != record["returned"] or ctl.evaluated != [e[0] for e in record["evals"]]:
                raise SystemExit(f"{name}/{s}: training.WolfeSearch does not replay the reference: {got!r}/{exc} vs {record['returned']!r}/{record['exception']}")
            tags = classify(record, ctl, spec["constants"])
            covered |= tags
            key = f"{name}/{s}"
            out[f"{key}/phi0"] = np.array(record["phi0"], dtype=np.float64)
            out[f"{key}/evals"] = np.array(record["evals"], dtype=np.float64).reshape(-1, 3)
            out[f"{key}/returned"] = np.array([np.nan if record["returned"] is None else record["returned"]], dtype=np.float64)
            table[key] = dict(constants=spec["constants"], exception=record["exception"], n_evals=len(record["evals"]), exits=sorted(tags),
                              outer_exit=ctl.exit, zoom_exit=ctl.zoom_exit, table_hits=ctl.table_hits,
                              returned_is_evaluated=record["returned"] in [e[0] for e in record["evals"]])
            print(key, table[key], [e[0] for e in record["evals"]], record["returned"], flush=True)
    return out, table, covered


# ---------------------------------------------------------------------------------------------------------------------- step vectors
STEP_SHAPES = OPT_SHAPES + ((259,),)
#            momentum  dampening  nesterov  weight_decay
STEP_CONFIGS = ((0.9, 0.0, True, 5e-4), (0.9, 0.25, False, 5e-4), (0.0, 0.0, False, 0.0), (0.5, 0.0, True, 0.0), (0.0, 0.0, False, 1e-2))
STEP_LR, STEP_ALPHAS, STEP_STEPS = 0.07, (1.0, 2.5, 0.3217), 3


def step_vectors(fullbatch):
    """STEP_STEPS steps of the reference's own methods (``_save_initial_state``, ``_find_descent_direction``, ``_attempt_step``, ``_get_phi_grad``)
    in float32 for every row of STEP_CONFIGS; gradient magnitudes span 1e-6 .. 1e2.  Keys ``c{config}/...``: theta0, then per step t: g{t} (the
    gradient of the direction), mom{t}, p{t}, dphi0_{t}, and per trial a: theta{t}_{a}, ga{t}_{a} (the gradient there), dphi{t}_{a}."""
    wolfe_cls = fullbatch.training.optimizers.WolfeGradientDescent
    out = {"configs": np.array([[m, d, float(n), w] for m, d, n, w in STEP_CONFIGS], dtype=np.float64), "lr": np.array([STEP_LR]),
           "alphas": np.array(STEP_ALPHAS, dtype=np.float64)}
    fma_all, two_all = True, True
    for c, (mu, damp, nesterov, wd) in enumerate(STEP_CONFIGS):
        gen = torch.Generator().manual_seed(211 + c)
        params = [torch.nn.Parameter(torch.randn(shape, generator=gen) * 0.3) for shape in STEP_SHAPES]
        opt = wolfe_cls(params, lr=STEP_LR, momentum=mu, dampening=damp, nesterov=nesterov, weight_decay=wd)

        def draw():
            for p in params:
                scale = 10.0 ** (torch.rand(p.shape, generator=gen) * 8 - 6)
                p.grad = torch.randn(p.shape, generator=gen) * scale

        for i, p in enumerate(params):
            out[f"c{c}/theta0/{i}"] = p.detach().numpy().copy()
        with torch.no_grad():
            for t in range(1, STEP_STEPS + 1):
                opt.has_stepped = False
                opt._save_initial_state()
                draw()
                p_k, offset = opt._find_descent_direction()
                out[f"c{c}/dphi0_{t}"] = np.array([float(offset)], dtype=np.float64)
                for i, p in enumerate(params):
                    out[f"c{c}/g{t}/{i}"], out[f"c{c}/p{t}/{i}"] = p.grad.numpy().copy(), p_k[0][i].numpy().copy()
                    if mu != 0:
                        out[f"c{c}/mom{t}/{i}"] = opt.state[p]["momentum_buffer"].numpy().copy()
                for a, alpha in enumerate(STEP_ALPHAS):
                    opt._attempt_step(p_k, alpha)
                    draw()
                    out[f"c{c}/dphi{t}_{a}"] = np.array([float(opt._get_phi_grad(p_k))], dtype=np.float64)
                    step = np.float32(STEP_LR * alpha)
                    for i, p in enumerate(params):
                        out[f"c{c}/theta{t}_{a}/{i}"], out[f"c{c}/ga{t}_{a}/{i}"] = p.detach().numpy().copy(), p.grad.numpy().copy()
                        th0, pk = opt.buffer[p].numpy(), p_k[0][i].numpy()
                        fma = (th0.astype(np.float64) + np.float64(step) * pk.astype(np.float64)).astype(np.float32)   # (the product of two float32 is exact in double)
                        two = th0 + step * pk
                        fma_all &= bool(np.array_equal(fma, p.detach().numpy()))
                        two_all &= bool(np.array_equal(two, p.detach().numpy()))
    if fma_all == two_all:
        raise SystemExit(f"the trial points do not tell the two rounding forms apart (fma {fma_all}, two roundings {two_all})")
    out["trial_form"] = np.array("fma" if fma_all else "two-roundings")
    print("trial points of the reference:", out["trial_form"], flush=True)
    return out


def checkpoint_structure(fullbatch, compose):
    """Key layout of the optimizer part of the reference's 5-list checkpoint for ResNet-20 after one Wolfe step.  The closure gives zero gradients
    and a constant loss 0; with the preset's weight decay the direction is still -1.9 wd theta, so phi'(0) < 0, no trial point has a sufficient
    decrease (the loss never moves), the rule-1 zoom shrinks its interval below 1e-4 and returns alpha_low: the recorded ``alpha`` is the int 0."""
    cfg = compose(["hyp=fb1", "model=resnet20", "hyp.optim.line_search=wolfe", "hyp.warmup=2"])
    torch.manual_seed(0)
    model = fullbatch.models.construct_model(cfg.model, 3, 10)
    optimizer, scheduler = fullbatch.training.optimizers.optim_interface(model, cfg.hyp)

    def closure():
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        return torch.zeros(())

    optimizer.step(closure)
    scheduler.step()

    class Counter:
        step = 1

    path = os.path.join(tempfile.mkdtemp(), "ck.pth")
    fullbatch.training.utils._save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=path)
    optim_state, _, sched_state, scaler_state, step = torch.load(path, weights_only=False)
    tensors = [k for k in optim_state["state"] if k != "alpha"]
    return dict(optimizer=type(optimizer).__name__, param_groups=describe(optim_state["param_groups"]), state0=describe(optim_state["state"][0]),
                state_last=describe(optim_state["state"][tensors[-1]]), n_state=len(optim_state["state"]), alpha=optim_state["state"]["alpha"],
                bare_keys=sorted(k for k in optim_state["state"] if isinstance(k, str)), scheduler_keys=sorted(sched_state),
                scaler_state=scaler_state, step=step)


# ---------------------------------------------------------------------------------------------------------------------- training scenarios
_R20 = ["model=resnet20", "hyp.optim.line_search=wolfe", "hyp.warmup=0"]
# name: (N, pixels, overrides without lr, steps); lr and the model seed come from LADDER.  wolfe_plain in chunks of 64: in chunks of 32 single
# chunks' gradient norms of the reference's own fp32 and float64 runs stayed 6e-4 .. 8e-4 apart down to lr 0.001 (limit 5e-4) on every rung.
SCENARIOS_WOLFE = {
    "wolfe_plain": (128, 16, ["hyp=fb1"] + _R20 + ["data.batch_size=64", "hyp.sub_batch=64"], 2),
    "wolfe_clip": (128, 16, ["hyp=fbclip"] + _R20 + ["data.batch_size=64", "hyp.sub_batch=64"], 2),
    "wolfe_reg": (64, 16, ["hyp=gradreg"] + _R20 + ["data.batch_size=32", "hyp.sub_batch=32"], 2),
}
# (lr, model seed) in the order tried; the first admissible pair is used.  wolfe_clip starts from a larger lr: it is the scenario meant to zoom.
LADDER = {
    "wolfe_plain": ((0.1, 91), (0.1, 92), (0.03, 91), (0.03, 92), (0.01, 91), (0.01, 92), (0.005, 91), (0.003, 91), (0.003, 92), (0.001, 91),
                    (0.005, 92), (0.005, 93), (0.005, 94), (0.003, 93), (0.003, 94), (0.002, 91), (0.002, 92)),
    "wolfe_clip": ((1.0, 93), (1.0, 94), (3.0, 93), (0.3, 93), (0.3, 94), (0.1, 93), (0.1, 94), (0.2, 93), (0.2, 94), (0.15, 93), (0.15, 94), (0.05, 93),
                   (0.15, 95), (0.15, 96), (0.1, 95), (0.1, 96), (0.2, 95), (0.2, 96), (0.05, 94), (0.05, 95)),
    "wolfe_reg": ((0.1, 95), (0.1, 96), (0.03, 95), (0.03, 96), (0.01, 95), (0.01, 96), (0.02, 95), (0.02, 96), (0.015, 95), (0.015, 96), (0.02, 97)),
}
JUDGED_AT = {"wolfe_plain": 2e-4, "wolfe_clip": 2e-4, "wolfe_reg": 3e-3}
# What the scenarios together must contain.  A ZOOM IS NOT AMONG THEM, and cannot be under rule 1: an interpolated alpha is a continuous function of
# the recorded losses and phi', so two runs whose statistics differ in the sixth digit never interpolate the same float -- the reference's own
# fp32 and float64 runs zoom to 0.44083938715763205 vs 0.4408212042526949 (wolfe_plain, lr 0.1, seed 91), 0.4518656017503446 vs
# 0.45182531514749213 (seed 92), 0.00940088497271796 vs 0.009400942949432056 (wolfe_clip, lr 3.0).  Every rung that zooms is refused by rule 1;
# the zoom itself is pinned exactly by the search cases above, where the values the controller sees are the recorded ones.
REQUIRED = ("accepted at alpha = 1", "growth step")
LOSS_NAMES, MARGIN = ("decrease", "zoom-decrease", "zoom-low"), 4.0


def instrument(wolfe_cls, log):
    """Wrap (not replace) three methods of the reference's class so that every ``step`` appends a record to ``log``: phi(0), phi'(0), every
    evaluation (alpha, val, grad, sum |a_i b_i| of the phi' just formed, in float64), the returned alpha.  -> the function that undoes it."""
    inner = {k: getattr(wolfe_cls, k) for k in ("_evaluate_phi", "_find_descent_direction", "step")}

    def abs_sum(self, p_k_groups):
        total = 0.0
        for group, p_k in zip(self.param_groups, p_k_groups):
            for i, param in enumerate(group["params"]):
                g = param.grad.double() + group["weight_decay"] * param.detach().double()
                total += float((g * p_k[i].double()).abs().sum())
        return total

    def _find_descent_direction(self):
        p_k, offset = inner["_find_descent_direction"](self)
        log[-1]["abs0"] = abs_sum(self, p_k)
        return p_k, offset

    def _evaluate_phi(self, alpha, p_k_groups, closure, LUT_ref):
        fresh = alpha not in LUT_ref
        res = inner["_evaluate_phi"](self, alpha, p_k_groups, closure, LUT_ref)
        log[-1]["phi0"] = (LUT_ref[0]["val"], LUT_ref[0]["grad"])
        if fresh:
            log[-1]["evals"].append((alpha, res[0], res[1], abs_sum(self, p_k_groups)))
        return res

    def step(self, closure):
        log.append(dict(evals=[]))
        inner["step"](self, closure)
        log[-1]["returned"] = self.state["alpha"]

    wolfe_cls._evaluate_phi, wolfe_cls._find_descent_direction, wolfe_cls.step = _evaluate_phi, _find_descent_direction, step

    def undo():
        for k, v in inner.items():
            setattr(wolfe_cls, k, v)
    return undo


def margins(log, constants, tol_loss, phi_c):
    """Replay every step through training.WolfeSearch and judge every inequality it decided -> (tags of what the searches did, the worst
    margin / (MARGIN * tolerance) -- admissible from 1 up --, the rows [step, kind, alpha, left, right, tolerance])."""
    tags, worst, rows = set(), float("inf"), []
    for s, rec in enumerate(log):
        ctl, got, exc = replay(dict(phi0=rec["phi0"], evals=[e[:3] for e in rec["evals"]]), constants)
        assert exc is None and got == rec["returned"], (s, got, exc, rec["returned"])
        absum = {0: rec["abs0"], **{e[0]: e[3] for e in rec["evals"]}}
        grads = {0: rec["phi0"][1], **{e[0]: e[2] for e in rec["evals"]}}
        u = 2.0 ** -24
        for kind, name in enumerate(("decrease", "curvature", "sign", "zoom-decrease", "zoom-low", "zoom-curvature", "zoom-sign")):
            for nm, alpha, left, right in ctl.trace:
                if nm != name:
                    continue
                if name in LOSS_NAMES:
                    tol = tol_loss * max(abs(left), abs(right))
                else:     # phi': the reduction bound of the kernels, and no less than the relative tolerance of the statistics
                    scale = abs(left / grads[alpha]) if name == "zoom-sign" and left != 0 else 1.0      # (left = phi'(alpha) (high - low))
                    tol = max(phi_c * u * (absum[alpha] * scale + (constants["c2"] * absum[0] if "curvature" in name else 0.0)),
                              tol_loss * max(abs(left), abs(right)))
                if abs(left - right) / (MARGIN * tol) < worst:
                    worst, margins.worst_row = abs(left - right) / (MARGIN * tol), (s, name, alpha, left, right, tol)
                rows.append([s, kind, alpha, left, right, tol])
        if ctl.exit == "accepted" and got == 1.0:
            tags.add("accepted at alpha = 1")
        if ctl.exit == "zoom-1":
            tags.add("rule-1 zoom")
        if ctl.exit == "zoom-2":
            tags.add("rule-2 zoom")
        if len(ctl.evaluated) > 1 and ctl.evaluated[1] == 2.5:
            tags.add("growth step")
    return tags, worst, rows


def run_one(fullbatch, compose, name, lr, seed, out, dtype, log):
    n, pixels, overrides, steps = SCENARIOS_WOLFE[name]
    mg.ALL_SCENARIOS[name] = (n, pixels, overrides + [f"hyp.optim.lr={lr}", f"hyp.steps={steps}"], seed)
    undo = instrument(fullbatch.training.optimizers.WolfeGradientDescent, log)
    try:
        with open(os.devnull, "w") as null:      # (the reference prints every alpha)
            stdout, sys.stdout = sys.stdout, null
            try:
                cfg, _ = mg.run_scenario(fullbatch, compose, name, out, dtype=dtype)
            finally:
                sys.stdout = stdout
    finally:
        undo()
    return cfg


def main_scenarios(only=None):
    from tests.wolfe_ref import phi_c
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    out, meta_s, refused, seen = {}, {}, [], set()
    for name in SCENARIOS_WOLFE:
        if only and name not in only:
            continue
        tried = []
        for lr, seed in LADDER[name]:
            trial, log32, log64 = {}, [], []
            cfg = run_one(fullbatch, compose, name, lr, seed, trial, torch.float, log32)
            run_one(fullbatch, compose, name, lr, seed, trial, torch.double, log64)
            constants = {k: cfg.hyp.optim.get(k, v) for k, v in DEFAULTS.items()}
            spread = mga.spread(trial, name)
            tol = JUDGED_AT[name]
            why = []
            a32, a64 = [[e[0] for e in r["evals"]] + [r["returned"]] for r in log32], [[e[0] for e in r["evals"]] + [r["returned"]] for r in log64]
            if a32 != a64:
                why.append(f"the fp32 and the float64 run take different alphas: {a32} vs {a64}")
            else:
                n_params = sum(p.numel() for p in fullbatch.models.construct_model(cfg.model, 3, 10).parameters())
                tags, worst, rows = margins(log32, constants, tol, phi_c(n_params, direction=True))
                _, worst64, _ = margins(log64, constants, tol, phi_c(n_params, direction=True))
                if not min(worst, worst64) >= 1.0:
                    why.append(f"an inequality is decided by {min(worst, worst64):.3g} x the required margin of {MARGIN} tolerances "
                               f"(step, inequality, alpha, left, right, tolerance: {margins.worst_row})")
            bad = {k: v for k, v in spread.items() if k in SPREAD_KEYS and not v < min(SPREAD_LIMIT, tol / 2)}
            bad.update({k: spread[k] for k in NORM_KEYS + ("grad_norm_train_max",) if k in spread and not spread[k] < max(tol, 1e-3) / 2})
            if bad:
                why.append(f"the reference's own fp32 run is {bad} from its float64 run")
            tried.append(dict(lr=lr, seed=seed, alphas=a32, refused=why, spread=spread))
            print(name, tried[-1], flush=True)
            if not why:
                break
        if why:
            refused.append(f"{name}: no rung of LADDER is admissible -- extend the ladder (smaller lr, other seeds), never a tolerance: "
                           + "; ".join(f"lr {t['lr']} seed {t['seed']}: {t['refused']}" for t in tried))
            continue
        seen |= tags
        final_runs = {str(THREADS[0]): spread["final_rel_l2"]}
        for threads in THREADS[1:]:
            torch.set_num_threads(threads)
            again = {}
            try:
                run_one(fullbatch, compose, name, lr, seed, again, torch.float, [])
            finally:
                torch.set_num_threads(THREADS[0])
            a, b = again[f"{name}/final_sample"], trial[f"{name}@f64/final_sample"]
            final_runs[str(threads)] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        out.update(trial)
        for tag, log in (("", log32), ("@f64", log64)):
            out[f"{name}{tag}/evals"] = np.array([[s, *e] for s, r in enumerate(log) for e in r["evals"]], dtype=np.float64)
            out[f"{name}{tag}/phi0"] = np.array([[*r["phi0"], r["abs0"], r["returned"]] for r in log], dtype=np.float64)
        out[f"{name}/inequalities"] = np.array(rows, dtype=np.float64)
        n, pixels, overrides, steps = SCENARIOS_WOLFE[name]
        meta_s[name] = dict(n=n, pixels=pixels, overrides=mg.ALL_SCENARIOS[name][2], model_seed=seed, lr=lr, steps=steps, tried=tried,
                            search=sorted(tags), worst_margin=min(worst, worst64), spread=spread, judged_at=tol, final_rel_l2_fp32_runs=final_runs,
                            final_rel_l2_bound=5 * max(final_runs.values()), constants=constants)
    # (``scenarios NAME ...`` measures only those and merges them into the files: the ladders are independent of each other)
    path, npz = os.path.join(HERE, "meta_wolfe.json"), os.path.join(HERE, "scenarios_wolfe.npz")
    lock = open(os.path.join(tempfile.gettempdir(), "make_golden_wolfe.lock"), "w")      # (two ladders may run side by side; held until the process ends)
    fcntl.flock(lock, fcntl.LOCK_EX)
    with open(path) as handle:
        meta = json.load(handle)
    if only and os.path.isfile(npz):
        kept = {k: v for k, v in np.load(npz).items() if k.split("/")[0].split("@")[0] not in only}
        out = {**kept, **out}
        meta_s = {**{k: v for k, v in meta.get("scenarios", {}).items() if k not in only}, **meta_s}
    for sc in meta_s.values():
        seen |= set(sc["search"])
    missing = [t for t in REQUIRED if t not in seen] if set(meta_s) == set(SCENARIOS_WOLFE) else []
    if missing:
        refused.append(f"the scenarios together lack: {missing}")
    if refused:
        raise SystemExit("\n".join(refused))
    out = {k: v for k, v in out.items() if "/chunk" not in k and "/probe_state" not in k}
    np.savez_compressed(npz, **out)
    meta.update(scenarios=meta_s, ladder={k: [list(r) for r in v] for k, v in LADDER.items()}, margin=MARGIN, spread_limit=SPREAD_LIMIT,
                required=list(REQUIRED))
    with open(path, "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote scenarios_wolfe.npz and the scenarios of meta_wolfe.json")


def main_search_and_steps():
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    out, table, covered = search_cases(fullbatch)
    missing = [c for c in COVERAGE if c not in covered]
    if missing:
        raise SystemExit(f"the search cases do not take these exits: {missing}")
    np.savez_compressed(os.path.join(HERE, "wolfe_search.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "wolfe_optimizer.npz"), **step_vectors(fullbatch))
    meta = {}
    if os.path.isfile(os.path.join(HERE, "meta_wolfe.json")):      # (the scenario part of the file is written by ``scenarios``)
        with open(os.path.join(HERE, "meta_wolfe.json")) as handle:
            meta = json.load(handle)
    meta.update(search_cases=table, coverage=list(COVERAGE), search_problems=SEARCH_CASES, reference_defaults=DEFAULTS,
                checkpoint=checkpoint_structure(fullbatch, compose))
    with open(os.path.join(HERE, "meta_wolfe.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote wolfe_search.npz, wolfe_optimizer.npz, meta_wolfe.json")


if __name__ == "__main__":
    if sys.argv[1:2] == ["scenarios"]:
        main_scenarios(only=sys.argv[2:] or None)
    else:
        main_search_and_steps()
