"""Golden vectors of the reference with ``hyp/optim=gd_agc`` (``SGD_AGC``, reference optimizers.py:45-52 -> additional_optimizers/sgd_agc.py),
full-batch and stochastic branch, and of ``SGD_AGC`` itself in float64.

Runs the real reference on CPU through the harness of ``make_golden.py`` (its helpers are imported, that file stays as it is), exactly like
``make_golden_adam.py`` (whose spread / admissibility code is imported), and writes

  tests/golden/scenarios_agc.npz    fp32 runs and ``@f64`` twins of the reference's own ``train()``
  tests/golden/meta_agc.json        the scenario table; per scenario the measured fp32-vs-float64 spread of the reference, the tolerance the
                                    engine tests judge it at and the number of units whose clip triggered at every update; the reference's
                                    preset; the key structure of the reference's own checkpoint
  tests/golden/agc_optimizer.npz    two steps of the reference's ``SGD_AGC`` in float64 on five small tensors (tests/test_cpu_agc.py holds
                                    ``tests/agc_ref.agc_ref`` against them)

Admissibility is the rule of ``make_golden_adam.py``: fp32 and float64 runs of the reference within ``SPREAD_LIMIT`` on the losses and the
parameter norm, and within HALF of the tolerance the engine tests judge at (2e-4; 3e-3 with the regulariser; max(tol, 1e-3) for gradient
norms) -- otherwise the generator stops: lower the lr or the steps, never raise a tolerance.  On top of it a scenario is refused unless, over
its updates, at least one unit's clip triggered and at least one did not (counted with the reference's own ``unitwise_norm`` in a wrapper
around its ``step``): both branches of the unit clip are on every recorded trajectory.  The learning rates are the ones the rule settled
(spreads in meta_agc.json): at lr 0.1 agc_plain is not admissible -- single chunks' gradient norms of the reference's two runs lie 9.5e-4
apart (limit 5e-4); at 0.03 agc_plain (4.0e-4), agc_clip_warm (1.3e-4) and agc_sgd_mode (4.9e-4) are.  agc_reg_r18, judged at 3e-3 (limit
1.5e-3), is not at 0.03 -- the norm of the regularised gradient before the clip lies 2.5e-3 apart -- and is at 0.01 (3.9e-4).

Usage:  python tests/golden/make_golden_agc.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_adam as mga  # noqa: E402
from tests.adam_ref import describe  # noqa: E402  (make_golden put the repository root on the path)

SPREAD_LIMIT, SPREAD_KEYS, NORM_KEYS, THREADS = mga.SPREAD_LIMIT, mga.SPREAD_KEYS, mga.NORM_KEYS, mga.THREADS

_R20 = ["model=resnet20", "hyp/optim=gd_agc"]
SCENARIOS_AGC = {
    # name: (N, pixels, overrides, model_seed)
    "agc_plain": (128, 16, ["hyp=fb1"] + _R20 + ["hyp.optim.lr=0.03", "hyp.steps=3", "hyp.warmup=0", "data.batch_size=32", "hyp.sub_batch=32"], 81),
    "agc_clip_warm": (128, 16, ["hyp=fbclip"] + _R20 + ["hyp.optim.lr=0.03", "hyp.steps=4", "hyp.warmup=2", "data.batch_size=64", "hyp.sub_batch=64"], 83),
    "agc_reg_r18": (64, 16, ["hyp=gradreg", "hyp/optim=gd_agc", "hyp.optim.lr=0.01", "hyp.steps=3", "hyp.warmup=1", "data.batch_size=32",
                             "hyp.sub_batch=32"], 85),
    "agc_sgd_mode": (128, 16, ["hyp=base_sgd"] + _R20 + ["hyp.optim.lr=0.03", "hyp.steps=2", "hyp.warmup=0", "hyp.grad_clip=0.5", "data.batch_size=32"], 87),
}
SHUFFLING = ("agc_sgd_mode",)       # hyp=base_sgd: the RandomSampler pair of make_golden.loaders (run_scenario picks it by name only)
JUDGED_AT = {"agc_plain": 2e-4, "agc_clip_warm": 2e-4, "agc_reg_r18": 3e-3, "agc_sgd_mode": 2e-4}


def count_triggers(fullbatch, log):
    """Wrap the reference's ``SGD_AGC.step``: before every update append [units whose clip triggers, units clipped at all] to ``log``, with the
    reference's own ``unitwise_norm``.  -> the function that removes the wrapper."""
    mod = sys.modules[fullbatch.training.optimizers.SGD_AGC.__module__]
    cls, plain = mod.SGD_AGC, mod.SGD_AGC.step

    def step(self, closure=None):
        loss = None
        if closure is not None:                  # (the reference's step evaluates the closure first: the gradients exist only after it)
            with torch.enable_grad():
                loss = closure()
        hit = total = 0
        with torch.no_grad():
            for group in self.param_groups:
                if group["clipping"] is None:
                    continue
                for p in group["params"]:
                    pn = torch.clamp(mod.unitwise_norm(p), min=group["eps"])
                    gn = mod.unitwise_norm(p.grad)
                    hit += int((gn > pn * group["clipping"]).sum())
                    total += gn.numel()
        log.append([hit, total])
        plain(self, None)
        return loss

    cls.step = step

    def undo():
        cls.step = plain
    return undo


def run(fullbatch, compose, name, out, dtype=torch.float, log=None):
    plain_loaders = mg.loaders
    mg.loaders = (lambda x, y, batch, shuffle=False: plain_loaders(x, y, batch, shuffle=True)) if name in SHUFFLING else plain_loaders
    undo = count_triggers(fullbatch, [] if log is None else log)
    try:
        mg.run_scenario(fullbatch, compose, name, out, dtype=dtype)
    finally:
        undo()
        mg.loaders = plain_loaders


def checkpoint_structure(fullbatch, compose):
    """Key layout of the optimizer part of the reference's 5-list checkpoint (training/utils.py:43-51) for ResNet-20 after one SGD_AGC step."""
    cfg = compose(["hyp=fb1", "model=resnet20", "hyp/optim=gd_agc", "hyp.warmup=2"])
    torch.manual_seed(0)
    model = fullbatch.models.construct_model(cfg.model, 3, 10)
    optimizer, scheduler = fullbatch.training.optimizers.optim_interface(model, cfg.hyp)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    optimizer.step()
    scheduler.step()

    class Counter:
        step = 1

    path = os.path.join(tempfile.mkdtemp(), "ck.pth")
    fullbatch.training.utils._save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=path)
    optim_state, _, sched_state, scaler_state, step = torch.load(path, weights_only=False)
    groups = optim_state["param_groups"]
    return dict(optimizer=type(optimizer).__name__, n_groups=len(groups), group0=describe(groups[0]), group_last=describe(groups[-1]),
                group_names=[g["name"] for g in groups], state0=describe(optim_state["state"][0]),
                state_last=describe(optim_state["state"][len(optim_state["state"]) - 1]), n_state=len(optim_state["state"]),
                scheduler_keys=sorted(sched_state), scaler_state=scaler_state, step=step)


OPT_HYP = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=2e-5, nesterov=True, clipping=0.01, eps=1e-3)
OPT_TENSORS = (("conv.weight", (5, 3, 3, 3)), ("gain.weight", (1, 4, 1, 1)), ("bn.bias", (7,)), ("fc.weight", (4, 6)), ("linear.weight", (3, 5)))


def optimizer_vectors(fullbatch):
    """Two steps of the reference's SGD_AGC in float64 (the first-step buffer, then momentum) on OPT_TENSORS, groups as optim_interface makes them
    (``linear.weight`` unclipped).  Step-1 gradients hold, in conv.weight: unit 0 with a zero gradient, unit 1 with zero PARAMETERS (the eps floor
    decides), unit 2 with |g| = maxn (1 - 1e-9) (just below the trigger), unit 3 with |g| = maxn (1 + 1e-9) (just above); the rest is random, at
    a scale where some units trigger and some do not."""
    mod = sys.modules[fullbatch.training.optimizers.SGD_AGC.__module__]
    gen = torch.Generator().manual_seed(91)
    params = [(name, torch.nn.Parameter(torch.randn(shape, generator=gen, dtype=torch.float64) * 0.3)) for name, shape in OPT_TENSORS]
    g1 = [torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3 * 0.01 / 0.9 for _, p in params]
    g2 = [torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3 * 0.01 / 0.9 for _, p in params]
    w = params[0][1]
    with torch.no_grad():
        w[1] = 0.0
        g1[0][0] = 0.0
        for unit, rel in ((2, 1 - 1e-9), (3, 1 + 1e-9)):
            maxn = max(float(w[unit].norm()), OPT_HYP["eps"]) * OPT_HYP["clipping"]
            g1[0][unit] *= maxn * rel / float(g1[0][unit].norm())
    opt = mod.SGD_AGC(params, **OPT_HYP)
    for group in opt.param_groups:
        if group["name"].startswith("linear"):
            group["clipping"] = None
    out = {"names": np.array([n for n, _ in OPT_TENSORS]), "hyp_keys": np.array(sorted(OPT_HYP)), "hyp_values": np.array([float(OPT_HYP[k]) for k in sorted(OPT_HYP)])}
    for i, (_, p) in enumerate(params):
        out[f"p0/{i}"] = p.detach().numpy().copy()
    for t, grads in ((1, g1), (2, g2)):
        log = []
        for (_, p), g in zip(params, grads):
            p.grad = g.clone()
        undo = count_triggers(fullbatch, log)
        try:
            opt.step()
        finally:
            undo()
        for i, (_, p) in enumerate(params):
            assert torch.equal(p.grad, grads[i])                    # the clipped gradient is never written back
            out[f"g{t}/{i}"], out[f"p{t}/{i}"] = grads[i].numpy().copy(), p.detach().numpy().copy()
            out[f"buf{t}/{i}"] = opt.state[p]["momentum_buffer"].numpy().copy()
        out[f"triggered{t}"] = np.array(log[0])
        assert 0 < log[0][0] < log[0][1], log
    return out


def main(only=None):
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    mg.ALL_SCENARIOS.update(SCENARIOS_AGC)       # (the table run_scenario reads; the module's file is not touched)
    out, spreads, final_runs, triggered = {}, {}, {}, {}
    for name in SCENARIOS_AGC:
        if only and name not in only:
            continue
        triggered[name] = []
        run(fullbatch, compose, name, out, log=triggered[name])
        run(fullbatch, compose, name, out, dtype=torch.double)
        spreads[name] = mga.spread(out, name)
        print(name, "fp32-vs-f64 spread of the reference:", spreads[name])
        print(name, "[triggered units, clipped units] per update:", triggered[name])
        if not any(h > 0 for h, _ in triggered[name]) or not any(h < n for h, n in triggered[name]):
            raise SystemExit(f"{name}: one branch of the unit clip never occurs: {triggered[name]}")
        final_runs[name] = {str(THREADS[0]): spreads[name]["final_rel_l2"]}
        for threads in THREADS[1:]:               # (one fp32 run is one sample of the reference's distance from its float64 run: see make_golden_adam.py)
            torch.set_num_threads(threads)
            again = {}
            try:
                run(fullbatch, compose, name, again)
            finally:
                torch.set_num_threads(THREADS[0])
            a, b = again[f"{name}/final_sample"], out[f"{name}@f64/final_sample"]
            final_runs[name][str(threads)] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(name, "final state, fp32 runs of the reference vs its float64 run, by threads:", final_runs[name])
        bad = {k: v for k, v in spreads[name].items() if k in SPREAD_KEYS and not v < SPREAD_LIMIT}
        if bad:
            raise SystemExit(f"{name} is not admissible: {bad} (limit {SPREAD_LIMIT})")
        tol = JUDGED_AT[name]
        bad = {k: v for k, v in spreads[name].items() if k in SPREAD_KEYS and not v < tol / 2}
        bad.update({k: spreads[name][k] for k in NORM_KEYS + ("grad_norm_train_max",) if k in spreads[name] and not spreads[name][k] < max(tol, 1e-3) / 2})
        if bad:
            raise SystemExit(f"{name} cannot be judged at {tol}: the reference's own fp32 run is {bad} from its float64 run -- lower the lr or the steps")
    if only:
        return
    out = {k: v for k, v in out.items() if "/chunk" not in k and "/probe_state" not in k}
    np.savez_compressed(os.path.join(HERE, "scenarios_agc.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "agc_optimizer.npz"), **optimizer_vectors(fullbatch))
    with open(os.path.join(os.path.dirname(os.path.dirname(fullbatch.__file__)), "config", "hyp", "optim", "gd_agc.yaml")) as handle:
        preset = yaml.safe_load(handle)
    preset = {k: (float(v) if isinstance(v, str) else v) for k, v in preset.items() if k != "name"} | {"name": preset["name"]}
    meta = dict(scenarios={k: dict(n=v[0], pixels=v[1], overrides=v[2], model_seed=v[3], shuffling_loader=k in SHUFFLING) for k, v in SCENARIOS_AGC.items()},
                spread_limit=SPREAD_LIMIT, spread=spreads, judged_at=JUDGED_AT, triggered_units=triggered, final_rel_l2_fp32_runs=final_runs,
                final_rel_l2_bound={k: 5 * max(v.values()) for k, v in final_runs.items()}, reference_preset=preset,
                checkpoint=checkpoint_structure(fullbatch, compose))
    with open(os.path.join(HERE, "meta_agc.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote", os.path.join(HERE, "scenarios_agc.npz"), os.path.join(HERE, "agc_optimizer.npz"), os.path.join(HERE, "meta_agc.json"))


if __name__ == "__main__":
    main(only=sys.argv[1:] or None)
