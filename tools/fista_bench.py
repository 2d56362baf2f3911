"""Measurements of the FISTA update (profiles/fista.md), by the protocol of tools/adam_bench.py.

  --kernels   ``fb_mt_fista`` against ``fb_mt_clip_sgd`` with momentum on ResNet-18's arena (n = 11 173 962 floats), both without a clip, in one
              process: device events around every launch, the two kernels alternating, warm-up launches discarded, median (min .. max) of
              ``--reps``.  Both move the same bytes: 12 B read and 8 B written per element (theta, grad and one state arena in; theta and the
              state arena out).  Twice: on ONE set of operands (resident: 134 MB sit in the 256 MiB last-level cache between launches) and
              FROM HBM: between two timed launches a 1 GiB buffer is overwritten (four times the last-level cache), so every launch finds its
              operands evicted; the launches also rotate over ``--sets`` sets of operands.
  --mode      ms per mini-batch update of ``hyp.train_stochastic`` with ``hyp/optim=fista`` next to SGD mode, by the protocol of
              tools/sgd_mode_bench.py: ResNet-18, 32 px, 49 920 synthetic images in blocks of 128, bf16; one trainer per optimizer in the same
              process, epochs alternating, two warm-up epochs each, the median of ``--epochs`` timed ones; the update section (update + weight
              copies) from one event pair per block.

    python tools/fista_bench.py --kernels --mode [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N18 = 11_173_962
BYTES_PER_ELEMENT = 20           # both kernels: 3 reads + 2 writes of 4 B
FLUSH_BYTES = 1 << 30


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(reps, warmup, sets):
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.engine import fista_coefficients
    lib.load()
    n = N18
    gen = torch.Generator(device="cuda").manual_seed(0)
    pool = [[torch.randn(n, device="cuda", generator=gen) * s for s in (0.1, 0.01, 0.1)] for _ in range(sets)]
    flush = torch.empty(FLUSH_BYTES // 4, device="cuda", dtype=torch.float32)
    tk = np.float32(1)
    for _ in range(7):
        tk, ak, opak = fista_coefficients(tk, (1.0, 1.0, 4.0))

    def fista(o):
        lib.call("fb_mt_fista", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, None, -1.0, 0, 1e-3, float(ak), float(opak))

    def sgd(o):
        lib.call("fb_mt_clip_sgd", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, None, -1.0, 1e-3, 5e-4, 0.9, 0.0, 1, 0)

    out = {}
    for label, from_hbm in (("resident", False), ("hbm", True)):
        times = {"fista": [], "sgd": []}
        for i in range(warmup + reps):
            for name, fn in ((("fista", fista), ("sgd", sgd)) if i % 2 == 0 else (("sgd", sgd), ("fista", fista))):
                o = pool[(2 * i + (name == "sgd")) % sets] if from_hbm else pool[0]
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
        for name in ("fista", "sgd"):
            s = _stat(times[name])
            res[name] = dict(us=s, bytes_per_element=BYTES_PER_ELEMENT, achieved_GBps=BYTES_PER_ELEMENT * n / (s["median"] * 1e-6) / 1e9)
        res["fista_over_sgd"] = res["fista"]["us"]["median"] / res["sgd"]["us"]["median"]
        res["fista_median_inside_sgd_min_max"] = res["sgd"]["us"]["min"] <= res["fista"]["us"]["median"] <= res["sgd"]["us"]["max"]
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    out.update(n=n, sets=sets, set_bytes=12 * n, flush_bytes=FLUSH_BYTES, reps=reps, warmup=warmup)
    return out


def mode(epochs, warmup, images, block, pixels):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(images, 3, pixels, pixels, generator=gen)
    y = torch.randint(0, 10, (images,), generator=gen)
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    trainers = {}
    for name, over in (("fista", ["hyp/optim=fista", "hyp.optim.lr=0.01"]), ("sgd", ["hyp.optim.lr=0.01"])):
        cfg = compose(["hyp=base_sgd", "model=resnet18", f"data.pixels={pixels}", f"data.batch_size={block}", "hyp.steps=100000", "hyp.warmup=0",
                       "hyp.scheduler=cosine-4000", "impl.mixed_precision=True", "impl.validate_every_nth_step=1000000"] + over)
        torch.manual_seed(0)
        trainers[name] = FullBatchTrainer(construct_model(cfg.model, 3, 10), (x, y), None, setup, cfg)

    def epoch(name):
        t = trainers[name]
        t.sgd_section_events = sections = []
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        t.step()
        end.record()
        end.synchronize()
        t.flush_stats()
        ms, sec = begin.elapsed_time(end), sum(b.elapsed_time(e) for b, e in sections)
        return dict(optimizer=name, epoch_ms=ms, ms_per_update=ms / t.num_blocks, update_section_us_per_update=sec / t.num_blocks * 1e3,
                    train_loss=t.stats["train_loss"][-1])

    for _ in range(warmup):
        for name in trainers:
            epoch(name)
    rows = {name: [] for name in trainers}
    for i in range(epochs):
        for name in (("fista", "sgd") if i % 2 == 0 else ("sgd", "fista")):
            r = epoch(name)
            rows[name].append(r)
            print(json.dumps(dict(r, epoch=i)), flush=True)
    out = dict(images=images, block=block, updates_per_epoch=trainers["fista"].num_blocks, epochs=epochs, warmup_epochs=warmup)
    for name, rs in rows.items():
        out[name] = {k: _stat([r[k] for r in rs]) for k in ("epoch_ms", "ms_per_update", "update_section_us_per_update")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--mode", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--images", type=int, default=49920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fista_bench: no GPU visible -- nothing is measured without one")
    summary = dict(device=torch.cuda.get_device_name(0))
    if args.kernels:
        summary["kernels"] = kernels(args.reps, args.warmup, args.sets)
    if args.mode:
        summary["mode"] = mode(args.epochs, 2, args.images, 128, 32)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            json.dump(summary, handle, indent=1)


if __name__ == "__main__":
    main()
