"""Golden vectors of the reference with ``hyp/optim=adam`` (``torch.optim.AdamW``, reference optimizers.py:39-40), full-batch and stochastic branch.

Runs the real reference on CPU through the harness of ``make_golden.py`` (its helpers are imported, that file stays as it is) and writes, in
the key scheme of the other fixture files,

  tests/golden/scenarios_adam.npz   fp32 runs and ``@f64`` twins of the reference's own ``train()``
  tests/golden/meta_adam.json       the scenario table; per scenario the measured fp32-vs-float64 spread of the reference and the tolerance the
                                    engine tests judge it at; the reference's preset; the key structure of the reference's own checkpoint

Adam divides the first moment by the root of the second, so the rounding noise of a gradient element near zero becomes a step of +-lr: at the
preset's lr 1e-3 the reference's own fp32 and float64 runs end 2.4e-3 apart in the parameters after three steps (9 % of the sampled elements
differ by more than 1e-4).  Trajectories are comparable at small lr only; every scenario overrides it (``fbclip`` / ``gradreg`` set 0.4 / 0.8,
where the loss goes to 43 in three steps).

Admissibility, the rule of ``make_golden_sgd.py``: a scenario is written only if the reference's fp32 and float64 runs agree within
``SPREAD_LIMIT`` on train_loss, full_loss and param_norm at every step.  On top of it, the engine tests judge a scenario at ``JUDGED_AT`` (the
values of the existing tests: 2e-4 plain and clipped, 3e-3 with the regulariser; ``max(tol, 1e-3)`` for grad_norm and the per-chunk norms), and
a tolerance is admissible only where the reference's own spread is below HALF of it -- otherwise the generator stops: lower the scenario's lr
or its steps, never raise the tolerance.  That rule set three of the learning rates here: at the first choices -- adam_plain 1e-4, adam_clip_warm
3e-4, adam_sgd_mode 1e-4 -- losses and parameter norm were far inside (train_loss 4.7e-6 / 2.7e-5 / 2.7e-6) but single chunks' gradient norms of
the reference's own two runs lay 9.1e-4 / 7.3e-4 / 8.9e-4 apart from the second update on (limit 5e-4): the first AdamW update moves EVERY element
by lr sign(g), whatever its size.  At 3e-5: 3.4e-4 / 6e-5 / 1.6e-4 (adam_clip_warm at 1e-4 was still at 5.7e-4).  adam_reg_r18, judged at 3e-3
(limit 1.5e-3), is admissible at 3e-4: 5.0e-4.

Usage:  python tests/golden/make_golden_adam.py
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
from tests.adam_ref import describe  # noqa: E402  (make_golden put the repository root on the path)

SPREAD_LIMIT = 1e-3
SPREAD_KEYS = ("train_loss", "full_loss", "param_norm")
NORM_KEYS = ("grad_norm", "preclip_gradnorm")      # gradient norms: judged at max(tol, 1e-3), like the per-chunk norms grad_norm_train_k
THREADS = (8, 2, 1)            # the runs above use the first; the fp32 run is repeated with the others (another summation order in torch's CPU kernels)

_R20 = ["model=resnet20", "hyp/optim=adam"]
SCENARIOS_ADAM = {
    # name: (N, pixels, overrides, model_seed)
    "adam_plain": (128, 16, ["hyp=fb1"] + _R20 + ["hyp.optim.lr=0.00003", "hyp.steps=3", "hyp.warmup=0", "data.batch_size=32", "hyp.sub_batch=32"], 71),
    "adam_clip_warm": (128, 16, ["hyp=fbclip"] + _R20 + ["hyp.optim.lr=0.00003", "hyp.steps=4", "hyp.warmup=2", "data.batch_size=64", "hyp.sub_batch=64"], 73),
    "adam_reg_r18": (64, 16, ["hyp=gradreg", "hyp/optim=adam", "hyp.optim.lr=0.0003", "hyp.optim.weight_decay=0.1", "hyp.steps=3", "hyp.warmup=1",
                              "data.batch_size=32", "hyp.sub_batch=32"], 75),
    "adam_sgd_mode": (128, 16, ["hyp=base_sgd"] + _R20 + ["hyp.optim.lr=0.00003", "hyp.steps=2", "hyp.warmup=0", "hyp.grad_clip=0.5", "data.batch_size=32"], 77),
}
SHUFFLING = ("adam_sgd_mode",)      # hyp=base_sgd: the RandomSampler pair of make_golden.loaders (run_scenario picks it by name only)
JUDGED_AT = {"adam_plain": 2e-4, "adam_clip_warm": 2e-4, "adam_reg_r18": 3e-3, "adam_sgd_mode": 2e-4}


def spread(out, name):
    """Largest relative fp32-vs-float64 difference of the reference's own runs, per statistic, over the recorded steps; the relative l2 distance
    of the sampled final states."""
    res = {}
    for key in SPREAD_KEYS + NORM_KEYS:
        if f"{name}@f64/stat/{key}" not in out:
            continue
        r32, r64 = out[f"{name}/stat/{key}"], out[f"{name}@f64/stat/{key}"]
        res[key] = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
    chunks = [k.split("/stat/")[1] for k in out if k.startswith(f"{name}@f64/stat/grad_norm_train_")]
    res["grad_norm_train_max"] = max(float(np.max(np.abs(out[f"{name}/stat/{k}"] - out[f"{name}@f64/stat/{k}"]) / out[f"{name}@f64/stat/{k}"])) for k in chunks)
    a, b = out[f"{name}/final_sample"], out[f"{name}@f64/final_sample"]
    res["final_rel_l2"] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    return res


def checkpoint_structure(fullbatch, compose):
    """Key layout of the optimizer part of the reference's 5-list checkpoint (training/utils.py:43-51) for ResNet-20 after one AdamW step."""
    cfg = compose(["hyp=fb1", "model=resnet20", "hyp/optim=adam", "hyp.warmup=2"])
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
    return dict(optimizer=type(optimizer).__name__, param_groups=describe(optim_state["param_groups"]), state0=describe(optim_state["state"][0]),
                state_last=describe(optim_state["state"][len(optim_state["state"]) - 1]), n_state=len(optim_state["state"]),
                scheduler_keys=sorted(sched_state), scaler_state=scaler_state, step=step)


def main(only=None):
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    mg.ALL_SCENARIOS.update(SCENARIOS_ADAM)      # (the table run_scenario reads; the module's file is not touched)
    plain_loaders = mg.loaders
    out, spreads, final_runs = {}, {}, {}
    for name in SCENARIOS_ADAM:
        if only and name not in only:
            continue
        mg.loaders = (lambda x, y, batch, shuffle=False: plain_loaders(x, y, batch, shuffle=True)) if name in SHUFFLING else plain_loaders
        try:
            mg.run_scenario(fullbatch, compose, name, out)
            mg.run_scenario(fullbatch, compose, name, out, dtype=torch.double)
        finally:
            mg.loaders = plain_loaders
        spreads[name] = spread(out, name)
        print(name, "fp32-vs-f64 spread of the reference:", spreads[name])
        # The final state is judged in relative l2 against the float64 run, within 5x what the reference's own fp32 run gets -- and ONE fp32 run is one
        # sample of that: the same reference code with 2 threads instead of 8 ended 1.7e-5 from the float64 run of adam_sgd_mode where the
        # 8-thread run ended 2.3e-6.  So the fp32 run is repeated with other thread counts and the largest distance is the one recorded.
        final_runs[name] = {str(THREADS[0]): spreads[name]["final_rel_l2"]}
        for threads in THREADS[1:]:
            torch.set_num_threads(threads)
            again = {}
            mg.loaders = (lambda x, y, batch, shuffle=False: plain_loaders(x, y, batch, shuffle=True)) if name in SHUFFLING else plain_loaders
            try:
                mg.run_scenario(fullbatch, compose, name, again)
            finally:
                mg.loaders = plain_loaders
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
    np.savez_compressed(os.path.join(HERE, "scenarios_adam.npz"), **out)
    with open(os.path.join(os.path.dirname(os.path.dirname(fullbatch.__file__)), "config", "hyp", "optim", "adam.yaml")) as handle:
        preset = yaml.safe_load(handle)
    preset = {k: (float(v) if isinstance(v, str) else v) for k, v in preset.items() if k != "name"} | {"name": preset["name"]}
    meta = dict(scenarios={k: dict(n=v[0], pixels=v[1], overrides=v[2], model_seed=v[3], shuffling_loader=k in SHUFFLING) for k, v in SCENARIOS_ADAM.items()},
                spread_limit=SPREAD_LIMIT, spread=spreads, judged_at=JUDGED_AT, final_rel_l2_fp32_runs=final_runs,
                final_rel_l2_bound={k: 5 * max(v.values()) for k, v in final_runs.items()}, reference_preset=preset,
                checkpoint=checkpoint_structure(fullbatch, compose))
    with open(os.path.join(HERE, "meta_adam.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote", os.path.join(HERE, "scenarios_adam.npz"), os.path.join(HERE, "meta_adam.json"))


if __name__ == "__main__":
    main(only=sys.argv[1:] or None)
