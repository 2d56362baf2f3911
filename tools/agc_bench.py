"""Measurements of the GD-AGC update (profiles/agc.md), by the protocol of tools/adam_bench.py.

  --kernels   ``fb_mt_agc_sgd`` on ResNet-18's arena (P = 11 174 016 floats) and its own unit table (62 tensors, 4 851 units) against
              ``fb_mt_clip_sgd`` alone (the same 20 B per element) and against the back-to-back pair ``fb_mt_norms2`` + ``fb_mt_clip_sgd`` (28 B
              per element: the cheapest unfused form the library could offer -- a pass for the norms, a pass for the update), in one process:
              device events around every launch (around both launches of the pair), the three alternating in rotating order, warm-up launches
              discarded, median (min .. max) of ``--reps``.  Twice: on ONE set of operands (resident: 134 MB sit in the 256 MiB last-level cache
              between launches) and rotating over ``--sets`` sets of operands (every launch finds its operands evicted: the HBM figure).
              Achieved bytes/s from the bytes the algorithm moves.  The gradients alternate between units about 0.5 and about 4 times their
              trigger, as in tests/test_gpu_agc_kernel.py.
  --mode      ms per mini-batch update of ``hyp.train_stochastic`` with ``hyp/optim=gd_agc`` next to SGD mode, by the protocol of
              tools/sgd_mode_bench.py: ResNet-18, 32 px, 49 920 synthetic images in blocks of 128, bf16; one trainer per optimizer in the same
              process, epochs alternating, two warm-up epochs each, the median of ``--epochs`` timed ones; the update section (update + weight
              copies) from one event pair per block.

    python tools/agc_bench.py --kernels --mode [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(reps, warmup, sets):
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.engine import Plan, agc_unit_rows
    from fullbatchtraining_amd.models import construct_model
    h = lib.load()
    plan = Plan(construct_model(compose(["model=resnet18", "model.stem=CIFAR"]).model, 3, 10), 32)
    rows, n = agc_unit_rows(plan), plan.P
    tab = torch.tensor(rows, dtype=torch.int64, device="cuda")
    scale = torch.ones(n, device="cuda")
    unit = 0
    for off, unit_len, units, _ in rows:
        scale[off:off + unit_len * units] = torch.tensor([0.5, 4.0], device="cuda")[(unit + torch.arange(units, device="cuda")) % 2].repeat_interleave(unit_len)
        unit += units
    gen = torch.Generator(device="cuda").manual_seed(0)

    def operands():
        return [torch.randn(n, device="cuda", generator=gen) * 0.1, torch.randn(n, device="cuda", generator=gen) * 1e-3 * scale,
                torch.randn(n, device="cuda", generator=gen) * 1e-3]

    pool = [operands() for _ in range(sets)]
    norms2, ws = torch.zeros(2, device="cuda"), torch.zeros(h.fb_ws_mt_floats(1), device="cuda")

    def agc(o):
        lib.call("fb_mt_agc_sgd", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, None, -1.0, 0, 1e-3, 2e-5, 0.9, 0.0, 1, 0, 0.01, 1e-3,
                 tab.data_ptr(), tab.shape[0])

    def sgd(o):
        lib.call("fb_mt_clip_sgd", o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), n, None, -1.0, 1e-3, 2e-5, 0.9, 0.0, 1, 0)

    def pair(o):
        lib.call("fb_mt_norms2", o[1].data_ptr(), o[0].data_ptr(), n, norms2.data_ptr(), ws.data_ptr())
        sgd(o)

    fns = (("agc", agc), ("sgd", sgd), ("pair", pair))
    out = {}
    for label, rotate in (("resident", False), ("rotating", True)):
        times = {name: [] for name, _ in fns}
        for i in range(warmup + reps):
            for j in range(3):
                k = (i + j) % 3
                name, fn = fns[k]
                o = pool[(3 * i + k) % sets] if rotate else pool[0]
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                fn(o)
                end.record()
                end.synchronize()
                if i >= warmup:
                    times[name].append(begin.elapsed_time(end) * 1e3)
        res = {}
        for name, bytes_per in (("agc", 20), ("sgd", 20), ("pair", 28)):
            s = _stat(times[name])
            res[name] = dict(us=s, bytes_per_element=bytes_per, achieved_GBps=bytes_per * n / (s["median"] * 1e-6) / 1e9)
        res["agc_over_sgd"] = res["agc"]["us"]["median"] / res["sgd"]["us"]["median"]
        res["agc_over_pair"] = res["agc"]["us"]["median"] / res["pair"]["us"]["median"]
        # the target: the fused launch beats the pair by more than the min..max spread of the two medians' runs
        res["pair_minus_agc_us"] = res["pair"]["us"]["median"] - res["agc"]["us"]["median"]
        res["spread_us"] = max(res[k]["us"]["max"] - res[k]["us"]["min"] for k in ("agc", "pair"))
        res["beats_the_pair_by_more_than_the_spread"] = res["pair_minus_agc_us"] > res["spread_us"]
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    out.update(n=n, units=sum(r[2] for r in rows), sets=sets, set_bytes=12 * n, reps=reps, warmup=warmup)
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
    for name, over in (("gd_agc", ["hyp/optim=gd_agc", "hyp.optim.lr=0.01"]), ("sgd", ["hyp.optim.lr=0.01"])):
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
        for name in (("gd_agc", "sgd") if i % 2 == 0 else ("sgd", "gd_agc")):
            r = epoch(name)
            rows[name].append(r)
            print(json.dumps(dict(r, epoch=i)), flush=True)
    out = dict(images=images, block=block, updates_per_epoch=trainers["gd_agc"].num_blocks, epochs=epochs, warmup_epochs=warmup)
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
        raise SystemExit("agc_bench: no GPU visible -- nothing is measured without one")
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
