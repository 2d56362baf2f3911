"""Measurements of the line-search kernels (profiles/wolfe.md), by the protocol of tools/fista_bench.py.

  --kernels   ``fb_mt_wolfe_direction`` / ``fb_mt_wolfe_trial`` / ``fb_mt_wolfe_phi_grad`` on ResNet-18's arena (n = 11 173 962 floats) next to the
              same step composed from torch operations on the same arenas (the A/B: there is no earlier path), and ``fb_mt_fista`` as the
              streaming kernel whose rate profiles/fista.md reports, in one process: device events around every launch (for torch: around the
              whole composition), the candidates alternating, warm-up launches discarded, median (min .. max) of ``--reps``.  Bytes per element
              against the floor of each kernel: direction 24 (theta, grad, mom in; mom, p, theta0 out), trial 12 (theta0, p in; theta out),
              phi_grad 12 (theta, grad, p in).  Twice: on ONE set of operands (resident in the 256 MiB last-level cache) and FROM HBM: a 1 GiB
              buffer is overwritten between two timed launches and the launches rotate over ``--sets`` sets of operands.
  --step      wall time of one Wolfe step of the trainer next to the plain gradient-descent step, ResNet-18, 32 px, ``--images`` synthetic
              images in chunks of 128, bf16: ms per step, closure evaluations per step, and the step's time in evaluations x the plain step's.

    python tools/wolfe_bench.py --kernels --step [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N18 = 11_173_962
FLUSH_BYTES = 1 << 30
WD, MU, STEP = 5e-4, 0.9, 0.1
BYTES = {"direction": 24, "trial": 12, "phi_grad": 12, "fista": 20}


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(reps, warmup, sets):
    from fullbatchtraining_amd import lib
    h = lib.load()
    n = N18
    gen = torch.Generator(device="cuda").manual_seed(0)
    names = ("theta", "grad", "mom", "p", "theta0")
    pool = [{k: torch.randn(n, device="cuda", generator=gen) * 0.1 for k in names} for _ in range(sets)]
    out2, ws = torch.zeros(2, device="cuda"), torch.zeros(h.fb_ws_mt_floats(1), device="cuda")
    flush = torch.empty(FLUSH_BYTES // 4, device="cuda", dtype=torch.float32)

    def direction(o):
        lib.call("fb_mt_wolfe_direction", o["theta"].data_ptr(), o["grad"].data_ptr(), o["mom"].data_ptr(), o["p"].data_ptr(), o["theta0"].data_ptr(), n,
                 WD, MU, 0.0, 1, 0, out2.data_ptr(), ws.data_ptr())

    def trial(o):
        lib.call("fb_mt_wolfe_trial", o["theta"].data_ptr(), o["theta0"].data_ptr(), o["p"].data_ptr(), n, STEP)

    def phi_grad(o):
        lib.call("fb_mt_wolfe_phi_grad", o["theta"].data_ptr(), o["grad"].data_ptr(), o["p"].data_ptr(), n, WD, out2.data_ptr() + 4, ws.data_ptr())

    def fista(o):
        lib.call("fb_mt_fista", o["theta"].data_ptr(), o["grad"].data_ptr(), o["mom"].data_ptr(), n, None, -1.0, 0, 1e-3, 0.4, 1.4)

    # the same steps composed from torch operations (what WolfeGradientDescent does per tensor, here on the whole arena at once)
    def torch_direction(o):
        o["theta0"].copy_(o["theta"])
        d = o["grad"].add(o["theta"], alpha=WD)
        o["mom"].mul_(MU).add_(d)
        torch.neg(d.add(o["mom"], alpha=MU), out=o["p"])
        out2[0] = (d * o["p"]).sum()

    def torch_trial(o):
        o["theta"].copy_(o["theta0"])
        o["theta"].add_(o["p"], alpha=STEP)

    def torch_phi_grad(o):
        out2[1] = (o["grad"].add(o["theta"], alpha=WD) * o["p"]).sum()

    cands = (("direction", direction), ("torch_direction", torch_direction), ("trial", trial), ("torch_trial", torch_trial),
             ("phi_grad", phi_grad), ("torch_phi_grad", torch_phi_grad), ("fista", fista))
    out = {}
    for label, from_hbm in (("resident", False), ("hbm", True)):
        times = {name: [] for name, _ in cands}
        for i in range(warmup + reps):
            order = cands if i % 2 == 0 else cands[::-1]
            for j, (name, fn) in enumerate(order):
                o = pool[(i + j) % sets] if from_hbm else pool[0]
                if from_hbm:
                    flush.fill_(float(i))
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                fn(o)
                end.record()
                end.synchronize()
                if i >= warmup:
                    times[name].append(begin.elapsed_time(end) * 1e3)
        res = {}
        for name, _ in cands:
            s = _stat(times[name])
            b = BYTES[name.replace("torch_", "")]
            res[name] = dict(us=s, floor_bytes_per_element=b, GBps_against_the_floor=b * n / (s["median"] * 1e-6) / 1e9)
        for k in ("direction", "trial", "phi_grad"):
            res[f"torch_over_{k}"] = res[f"torch_{k}"]["us"]["median"] / res[k]["us"]["median"]
            res[f"{k}_rate_over_fista_rate"] = res[k]["GBps_against_the_floor"] / res["fista"]["GBps_against_the_floor"]
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    out.update(n=n, sets=sets, flush_bytes=FLUSH_BYTES, reps=reps, warmup=warmup)
    return out


def step(steps, warmup, images, chunk, pixels):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(images, 3, pixels, pixels, generator=gen)
    y = torch.randint(0, 10, (images,), generator=gen)
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    trainers = {}
    for name, over in (("wolfe", ["hyp.optim.line_search=wolfe"]), ("plain", [])):
        cfg = compose(["hyp=fb1", "model=resnet18", f"data.pixels={pixels}", f"data.batch_size={chunk}", f"hyp.sub_batch={chunk}", "hyp.steps=100000",
                       "hyp.warmup=0", "hyp.scheduler=cosine-4000", "hyp.optim.lr=0.01", "impl.mixed_precision=True",
                       "impl.validate_every_nth_step=1000000"] + over)
        torch.manual_seed(0)
        trainers[name] = FullBatchTrainer(construct_model(cfg.model, 3, 10), (x, y), None, setup, cfg)

    def one(name):
        t = trainers[name]
        before = len(t.stats["train_loss"])
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        t.step()
        end.record()
        end.synchronize()
        t.flush_stats()
        return dict(trainer=name, step_ms=begin.elapsed_time(end), evaluations=len(t.stats["train_loss"]) - before, train_loss=t.stats["train_loss"][-1])

    for _ in range(warmup):
        for name in trainers:
            one(name)
    rows = {name: [] for name in trainers}
    for i in range(steps):
        for name in (("wolfe", "plain") if i % 2 == 0 else ("plain", "wolfe")):
            r = one(name)
            rows[name].append(r)
            print(json.dumps(dict(r, step=i)), flush=True)
    plain = statistics.median(r["step_ms"] for r in rows["plain"])
    out = dict(images=images, chunk=chunk, steps=steps, warmup_steps=warmup, plain_step_ms=_stat([r["step_ms"] for r in rows["plain"]]),
               wolfe_step_ms=_stat([r["step_ms"] for r in rows["wolfe"]]), wolfe_evaluations=[r["evaluations"] for r in rows["wolfe"]],
               wolfe_step_over_evaluations_x_plain=_stat([r["step_ms"] / (r["evaluations"] * plain) for r in rows["wolfe"]]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wolfe_bench: no GPU visible -- nothing is measured without one")
    summary = dict(device=torch.cuda.get_device_name(0))
    if args.kernels:
        summary["kernels"] = kernels(args.reps, args.warmup, args.sets)
    if args.step:
        summary["step"] = step(args.steps, 2, args.images, 128, 32)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            json.dump(summary, handle, indent=1)


if __name__ == "__main__":
    main()
