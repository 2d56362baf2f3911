"""Golden vectors of the reference with ``hyp/optim=fista`` (``FISTA``, reference optimizers.py:43-44 -> additional_optimizers/fista.py:13-82),
full-batch and stochastic branch, and of ``FISTA.step`` itself on CPU.

Runs the real reference on CPU through the harness of ``make_golden.py`` (its helpers are imported, that file stays as it is), exactly like
``make_golden_adam.py`` (whose spread / admissibility code is imported), and writes

  tests/golden/scenarios_fista.npz   fp32 runs and ``@f64`` twins of the reference's own ``train()``
  tests/golden/meta_fista.json       the scenario table; per scenario the measured fp32-vs-float64 spread of the reference, the tolerance the
                                     engine tests judge it at and the final-state distances at 8, 2 and 1 threads; the reference's preset; the
                                     key structure of the reference's own checkpoint after one step
  tests/golden/fista_optimizer.npz   six steps of the reference's ``FISTA.step`` in float32 on three small tensors, for both ``fista_mod``s, lr
                                     including 0 (tests/test_cpu_fista.py holds ``tests/fista_ref`` against them bit for bit)

Admissibility is the rule of ``make_golden_adam.py``: fp32 and float64 runs of the reference within ``SPREAD_LIMIT`` on the losses and the
parameter norm, and within HALF of the tolerance the engine tests judge at (2e-4; 3e-3 with the regulariser; max(tol, 1e-3) for gradient
norms) -- otherwise the generator stops (after measuring every scenario, so that one run names all that have to change): lower the lr or
the steps, never raise a tolerance.  The learning rates start from the preset's 0.1 and go down 0.1, 0.03, 0.01, 0.003 to the first admissible
one: fista_plain 0.003 (single chunks' gradient norms of the reference's own two runs lie 2.3e-3 apart at 0.1, 7.5e-4 at 0.01, 4.9e-4 at 0.003;
limit 5e-4), fista_clip_warm 0.1, fista_reg_r18 0.03 (norm before the clip 4.6e-3 apart at 0.1, limit 1.5e-3), fista_sgd_mode 0.01 (chunk
norms 1.9e-3 at 0.1, 8.3e-4 at 0.03).  LR_NOTES is copied into meta_fista.json next to the measured spreads.

Usage:  python tests/golden/make_golden_fista.py
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

_R20 = ["model=resnet20", "hyp/optim=fista"]
SCENARIOS_FISTA = {
    # name: (N, pixels, overrides, model_seed)
    "fista_plain": (128, 16, ["hyp=fb1"] + _R20 + ["hyp.optim.lr=0.003", "hyp.steps=3", "hyp.warmup=0", "data.batch_size=32", "hyp.sub_batch=32"], 91),
    "fista_clip_warm": (128, 16, ["hyp=fbclip"] + _R20 + ["hyp.optim.lr=0.1", "hyp.optim.fista_mod=[0.02,0.1,4.0]", "hyp.steps=4", "hyp.warmup=2",
                                  "data.batch_size=64", "hyp.sub_batch=64"], 93),
    "fista_reg_r18": (64, 16, ["hyp=gradreg", "hyp/optim=fista", "hyp.optim.lr=0.03", "hyp.steps=3", "hyp.warmup=1", "data.batch_size=32",
                               "hyp.sub_batch=32"], 95),
    "fista_sgd_mode": (128, 16, ["hyp=base_sgd"] + _R20 + ["hyp.optim.lr=0.01", "hyp.steps=2", "hyp.warmup=0", "hyp.grad_clip=0.5", "data.batch_size=32"], 97),
}
SHUFFLING = ("fista_sgd_mode",)     # hyp=base_sgd: the RandomSampler pair of make_golden.loaders (run_scenario picks it by name only)
JUDGED_AT = {"fista_plain": 2e-4, "fista_clip_warm": 2e-4, "fista_reg_r18": 3e-3, "fista_sgd_mode": 2e-4}
LR_NOTES = ("tried in the order 0.1, 0.03, 0.01, 0.003; the first admissible one is used.  fista_plain: 0.003 (single chunks' gradient norms of the "
            "reference's fp32 and float64 runs lie 2.3e-3 apart at 0.1 and 7.5e-4 at 0.01, limit 5e-4; 4.9e-4 at 0.003).  fista_clip_warm: 0.1.  "
            "fista_reg_r18: 0.03 (at 0.1 the norm before the clip lies 4.6e-3 apart, limit 1.5e-3).  fista_sgd_mode: 0.01 (chunk norms 1.9e-3 at 0.1, "
            "8.3e-4 at 0.03, limit 5e-4)")


def run(fullbatch, compose, name, out, dtype=torch.float):
    plain_loaders = mg.loaders
    mg.loaders = (lambda x, y, batch, shuffle=False: plain_loaders(x, y, batch, shuffle=True)) if name in SHUFFLING else plain_loaders
    try:
        mg.run_scenario(fullbatch, compose, name, out, dtype=dtype)
    finally:
        mg.loaders = plain_loaders


def checkpoint_structure(fullbatch, compose):
    """Key layout of the optimizer part of the reference's 5-list checkpoint (training/utils.py:43-51) for ResNet-20 after one FISTA step."""
    cfg = compose(["hyp=fb1", "model=resnet20", "hyp/optim=fista", "hyp.warmup=2"])
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
    last = optim_state["state"][len(optim_state["state"]) - 1]
    return dict(optimizer=type(optimizer).__name__, param_groups=describe(optim_state["param_groups"]), state0=describe(optim_state["state"][0]),
                state_last=describe(last), n_state=len(optim_state["state"]), x_plus_equals_x_minus=bool(torch.equal(last["x+"], last["x-"])),
                scheduler_keys=sorted(sched_state), scaler_state=scaler_state, step=step)


OPT_SHAPES = ((5,), (3, 4), (2, 3, 3, 3))
OPT_LRS = (0.0, 0.05, 0.1, 0.07, 0.1, 0.0)
OPT_MODS = ((1.0, 1.0, 4.0), (1.0 / 50.0, 1.0 / 10.0, 4.0))


def optimizer_vectors(fullbatch):
    """Six steps of the reference's FISTA in float32 on OPT_SHAPES for each of OPT_MODS, the lr of step t being OPT_LRS[t - 1] (0 at both ends).
    Gradient magnitudes span 1e-6 .. 1e2.  Keys ``m{mod}/...``: p0, then per step g, p, xm (x-), xp (x+) per tensor and tk."""
    mod = sys.modules[fullbatch.training.optimizers.FISTA.__module__]
    out = {"lrs": np.array(OPT_LRS, dtype=np.float64), "fista_mods": np.array(OPT_MODS, dtype=np.float64)}
    for m, fista_mod in enumerate(OPT_MODS):
        gen = torch.Generator().manual_seed(101 + m)
        params = [torch.nn.Parameter(torch.randn(shape, generator=gen) * 0.3) for shape in OPT_SHAPES]
        opt = mod.FISTA(params, lr=0.1, fista_mod=fista_mod)
        for i, p in enumerate(params):
            out[f"m{m}/p0/{i}"] = p.detach().numpy().copy()
        for t, lr in enumerate(OPT_LRS, start=1):
            opt.param_groups[0]["lr"] = lr
            for i, p in enumerate(params):
                scale = 10.0 ** (torch.rand(p.shape, generator=gen) * 8 - 6)
                p.grad = torch.randn(p.shape, generator=gen) * scale
                out[f"m{m}/g{t}/{i}"] = p.grad.numpy().copy()
            opt.step()
            for i, p in enumerate(params):
                st = opt.state[p]
                assert st["tk"].dtype == torch.float32 and st["tk"].shape == (1,)
                out[f"m{m}/p{t}/{i}"], out[f"m{m}/xm{t}/{i}"] = p.detach().numpy().copy(), st["x-"].numpy().copy()
                out[f"m{m}/xp{t}/{i}"] = st["x+"].numpy().copy()
                out[f"m{m}/tk{t}"] = st["tk"].numpy().copy()
    return out


def main(only=None):
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    mg.ALL_SCENARIOS.update(SCENARIOS_FISTA)     # (the table run_scenario reads; the module's file is not touched)
    out, spreads, final_runs, refused = {}, {}, {}, []
    for name in SCENARIOS_FISTA:
        if only and name not in only:
            continue
        run(fullbatch, compose, name, out)
        run(fullbatch, compose, name, out, dtype=torch.double)
        spreads[name] = mga.spread(out, name)
        print(name, "fp32-vs-f64 spread of the reference:", spreads[name], flush=True)
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
        print(name, "final state, fp32 runs of the reference vs its float64 run, by threads:", final_runs[name], flush=True)
        bad = {k: v for k, v in spreads[name].items() if k in SPREAD_KEYS and not v < SPREAD_LIMIT}
        if bad:
            refused.append(f"{name} is not admissible: {bad} (limit {SPREAD_LIMIT})")
        tol = JUDGED_AT[name]
        bad = {k: v for k, v in spreads[name].items() if k in SPREAD_KEYS and not v < tol / 2}
        bad.update({k: spreads[name][k] for k in NORM_KEYS + ("grad_norm_train_max",) if k in spreads[name] and not spreads[name][k] < max(tol, 1e-3) / 2})
        if bad:
            refused.append(f"{name} cannot be judged at {tol}: the reference's own fp32 run is {bad} from its float64 run -- lower the lr or the steps")
    if refused:                                   # (every scenario is measured before the generator stops: one run names all that have to change)
        raise SystemExit("\n".join(refused))
    if only:
        return
    out = {k: v for k, v in out.items() if "/chunk" not in k and "/probe_state" not in k}
    np.savez_compressed(os.path.join(HERE, "scenarios_fista.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "fista_optimizer.npz"), **optimizer_vectors(fullbatch))
    with open(os.path.join(os.path.dirname(os.path.dirname(fullbatch.__file__)), "config", "hyp", "optim", "fista.yaml")) as handle:
        preset = yaml.safe_load(handle)
    preset = {k: (float(v) if isinstance(v, str) else v) for k, v in preset.items() if k != "name"} | {"name": preset["name"]}
    meta = dict(scenarios={k: dict(n=v[0], pixels=v[1], overrides=v[2], model_seed=v[3], shuffling_loader=k in SHUFFLING) for k, v in SCENARIOS_FISTA.items()},
                spread_limit=SPREAD_LIMIT, spread=spreads, judged_at=JUDGED_AT, learning_rates=LR_NOTES, final_rel_l2_fp32_runs=final_runs,
                final_rel_l2_bound={k: 5 * max(v.values()) for k, v in final_runs.items()}, reference_preset=preset,
                checkpoint=checkpoint_structure(fullbatch, compose))
    with open(os.path.join(HERE, "meta_fista.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote", os.path.join(HERE, "scenarios_fista.npz"), os.path.join(HERE, "fista_optimizer.npz"), os.path.join(HERE, "meta_fista.json"))


if __name__ == "__main__":
    main(only=sys.argv[1:] or None)
