"""Measurements of the AdamW update (profiles/adam.md).

  --kernels   ``fb_mt_adamw`` against ``fb_mt_clip_sgd`` on ResNet-18's arena (n = 11 173 962 floats), both without a clip, in one process:
              device events around every launch, the two kernels alternating, warm-up launches discarded, median (min .. max) of ``--reps``.
              Twice: on ONE set of operands (resident: 179 / 134 MB sit in the 256 MiB last-level cache between launches) and rotating over
              ``--sets`` sets of operands (every launch finds its operands evicted: the HBM figure).  Achieved bytes/s from the bytes the
              algorithm moves: 28 B per element for AdamW (4 reads, 3 writes), 20 B for SGD with momentum (3 reads, 2 writes).
  --mode      ms per mini-batch update of ``hyp.train_stochastic`` with ``hyp/optim=adam`` next to SGD mode, by the protocol of
              tools/sgd_mode_bench.py: ResNet-18, 32 px, 49 920 synthetic images in blocks of 128, bf16; one trainer per optimizer in the same
              process, epochs alternating, two warm-up epochs each, the median of ``--epochs`` timed ones; the update section (update + weight
              copies) from one event pair per block.

    python tools/adam_bench.py --kernels --mode [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N18 = 11_173_962


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(reps, warmup, sets):
    from fullbatchtraining_amd import lib
    lib.load()
    n = N18
    gen = torch.Generator(device="cuda").manual_seed(0)

    def operands():
        return [torch.randn(n, device="cuda", generator=gen) * s for s in (0.1, 0.01, 0.01)] + [(torch.randn(n, device="cuda", generator=gen) * 0.01).pow(2)]

    pool = [operands() for _ in range(sets)]
    step_size, bc2 = 1e-3 / (1 - 0.9 ** 7), (1 - 0.999 ** 7) ** 0.5

    def adam(o):
        lib.call("fb_mt_adamw", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), n, None, -1.0, 0, 1e-3, 0.01, 0.9, 0.999, 1e-8, step_size, bc2)

    def sgd(o):
        lib.call("fb_mt_clip_sgd", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, None, -1.0, 1e-3, 5e-4, 0.9, 0.0, 1, 0)

    out = {}
    for label, rotate in (("resident", False), ("rotating", True)):
        times = {"adamw": [], "sgd": []}
        for i in range(warmup + reps):
            for name, fn in ((("adamw", adam), ("sgd", sgd)) if i % 2 == 0 else (("sgd", sgd), ("adamw", adam))):
                o = pool[(2 * i + (name == "sgd")) % sets] if rotate else pool[0]
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                fn(o)
                end.record()
                end.synchronize()
                if i >= warmup:
                    times[name].append(begin.elapsed_time(end) * 1e3)
        res = {}
        for name, bytes_per in (("adamw", 28), ("sgd", 20)):
            s = _stat(times[name])
            res[name] = dict(us=s, bytes_per_element=bytes_per, achieved_GBps=bytes_per * n / (s["median"] * 1e-6) / 1e9)
        res["adamw_over_sgd"] = res["adamw"]["us"]["median"] / res["sgd"]["us"]["median"]
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    out.update(n=n, sets=sets, set_bytes=16 * n, reps=reps, warmup=warmup)
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
    for name, over in (("adam", ["hyp/optim=adam", "hyp.optim.lr=0.0001"]), ("sgd", ["hyp.optim.lr=0.01"])):
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
        for name in (("adam", "sgd") if i % 2 == 0 else ("sgd", "adam")):
            r = epoch(name)
            rows[name].append(r)
            print(json.dumps(dict(r, epoch=i)), flush=True)
    out = dict(images=images, block=block, updates_per_epoch=trainers["adam"].num_blocks, epochs=epochs, warmup_epochs=warmup)
    for name, rs in rows.items():
        out[name] = {k: _stat([r[k] for r in rs]) for k in ("epoch_ms", "ms_per_update", "update_section_us_per_update")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--mode", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--images", type=int, default=49920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench: no GPU visible -- nothing is measured without one")
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
