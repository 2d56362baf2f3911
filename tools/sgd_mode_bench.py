"""A/B of the mini-batch SGD mode's update section: ONE fb_mt_sgd_prep launch (update + both weight copies) against the composition it
replaces (fb_mt_sgd_torch + one fb_weight_prep per layer, a replayed launch list).

Workload: ResNet-18, 32 px, 49 920 synthetic images in blocks of 128 (390 updates per epoch), bf16.  Both paths give the same bits, so ONE
trainer runs them alternately, epoch by epoch, in the same process on the same device: two warm-up epochs per path, then ``--epochs`` timed
epochs each.  An epoch is timed with device events around ``FullBatchTrainer.step()``; the update section (gradient norm where a clip is
set, update, weight copies) with one event pair per block inside it, summed.  Reported per path: the median over the epochs of ms per
update, images/s and the update section's time and share.  Prints one JSON line per epoch and a final JSON summary line.

    python tools/sgd_mode_bench.py [--epochs 5] [--images 49920] [--block 128] [--f32] [--clip 1.0] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=49920)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--pixels", type=int, default=32)
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--clip", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_mode_bench: no GPU visible -- nothing is measured without one")

    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer

    over = ["hyp=base_sgd", f"model={args.model}", f"data.pixels={args.pixels}", f"data.batch_size={args.block}", "hyp.steps=100000",
            "hyp.warmup=0", "hyp.scheduler=cosine-4000", "hyp.optim.lr=0.01", f"impl.mixed_precision={not args.f32}",
            "impl.validate_every_nth_step=1000000"]
    if args.clip is not None:
        over.append(f"hyp.grad_clip={args.clip}")
    cfg = compose(over)
    torch.manual_seed(0)
    model = construct_model(cfg.model, 3, 10)
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(args.images, 3, args.pixels, args.pixels, generator=gen)
    y = torch.randint(0, 10, (args.images,), generator=gen)
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    trainer = FullBatchTrainer(model, (x, y), None, setup, cfg)
    if not trainer.engine.sgd_prep_fused() and os.environ.get("FB_SGD_FUSED", "1") != "0":
        raise SystemExit("sgd_mode_bench: fb_mt_sgd_prep does not support this configuration")
    n_updates, images = trainer.num_blocks, trainer.num_blocks * trainer.block

    def epoch(fused):
        trainer.sgd_fused = fused
        trainer.sgd_section_events = sections = []
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        launches0 = trainer.engine.replays
        begin.record()
        trainer.step()
        end.record()
        end.synchronize()
        trainer.flush_stats()
        ms = begin.elapsed_time(end)
        sec = sum(b.elapsed_time(e) for b, e in sections)
        return dict(path="fused" if fused else "composition", epoch_ms=ms, ms_per_update=ms / n_updates, images_per_s=images / ms * 1e3,
                    update_section_ms=sec, update_section_ms_per_update=sec / n_updates, update_section_share=sec / ms,
                    replays=trainer.engine.replays - launches0, train_loss=trainer.stats["train_loss"][-1])

    for _ in range(args.warmup):
        for fused in (True, False):
            epoch(fused)
    rows = {"fused": [], "composition": []}
    for i in range(args.epochs):
        for fused in ((True, False) if i % 2 == 0 else (False, True)):         # alternate, and alternate who goes first
            r = epoch(fused)
            rows[r["path"]].append(r)
            print(json.dumps(dict(r, epoch=i)), flush=True)
    summary = dict(device=torch.cuda.get_device_name(0), model=args.model, pixels=args.pixels, images=images, block=trainer.block, updates_per_epoch=n_updates,
                   dtype="f32" if args.f32 else "bf16", grad_clip=args.clip, epochs=args.epochs, warmup_epochs=args.warmup,
                   parameters=trainer.engine.plan.P, layers=len(trainer.engine.plan.layers))
    for path, rs in rows.items():
        summary[path] = {k: statistics.median(r[k] for r in rs) for k in ("epoch_ms", "ms_per_update", "images_per_s", "update_section_ms",
                                                                         "update_section_ms_per_update", "update_section_share")}
        summary[path]["update_section_ms_min_max"] = [min(r["update_section_ms"] for r in rs), max(r["update_section_ms"] for r in rs)]
    summary["fused_update_section_is_faster"] = summary["fused"]["update_section_ms"] < summary["composition"]["update_section_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            json.dump(dict(summary=summary, epochs=rows), handle, indent=1)


if __name__ == "__main__":
    main()
