"""Measurements of the loss-landscape cruncher (profiles/landscape.md), by the protocol of tools/wolfe_bench.py.

  --kernel     ``fb_mt_landscape_point`` on ResNet-18's arena (n = 11 173 962 parameters, the engine's own layer table; bf16 and fp32 copies, and
               the offset alone) next to ``fb_mt_wolfe_trial``, the other kernel that streams the arena into theta, in one process: device events
               around every launch, the candidates alternating, warm-up launches discarded, median (min .. max) of ``--reps``.  Compared by bytes
               per element against the floor of each kernel: trial 12 (theta0, p in; theta out); point 16 (base, dx, dy in; theta out) plus the
               copy, 2 (bf16) or 4 (fp32) bytes for every element of a convolution layer.  Twice: on ONE set of operands (resident in the last-level
               cache) and FROM HBM (a 1 GiB buffer is overwritten between two timed launches, the launches rotate over ``--sets`` operand sets).
  --positions  ResNet-18, 32 px, ``--images`` synthetic images (default 49 920) in blocks of 128, bf16 and fp32: positions per second and ms per
               position, in one process, alternating,
                 shipped      ``Engine.landscape_point`` (one replayed list: point kernel, BatchNorm coefficients, every forward pass) + one read-back;
                 composition  the building blocks the engine had before: torch operations for the offset, ``prep_weights``, an ``evaluate_batch``
                              loop over passes of the same size (two floats read back after every pass), a torch reduction for |theta|^2;
                 floor        the replayed forward passes alone with the weights left as they are, one read-back;
               each with the host time until the last launch is enqueued (before the wait), which says which bound holds: enqueue or device time.

    python tools/landscape_bench.py --kernel --positions [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N18 = 11_173_962
FLUSH_BYTES = 1 << 30


def _stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def _resnet18():
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    torch.manual_seed(0)
    return construct_model(compose(["model=resnet18"]).model, 3, 10)


def kernel(reps, warmup, sets):
    from fullbatchtraining_amd import lib
    from fullbatchtraining_amd.engine import Plan
    lib.load()
    plan = Plan(_resnet18(), 32)
    n = plan.P
    rows = [[L.w_off, L.cout, L.taps, L.cin_real, L.cin_pad, L.wc_off, 0, 0] for L in sorted(plan.layers, key=lambda L: L.w_off)]
    in_layers = sum(L.w_numel for L in plan.layers)
    tab = torch.tensor(rows, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    pool = [{k: torch.randn(n, device="cuda", generator=gen) * 0.1 for k in ("theta", "base", "dx", "dy")} for _ in range(sets)]
    copies = {torch.bfloat16: torch.zeros(plan.wc_total, device="cuda", dtype=torch.bfloat16), torch.float32: torch.zeros(plan.wc_total, device="cuda")}
    xy = torch.tensor([0.3217, -0.7], device="cuda")
    flush = torch.empty(FLUSH_BYTES // 4, device="cuda", dtype=torch.float32)

    def point(dtype, table):
        def fn(o):
            lib.call("fb_mt_landscape_point", o["theta"].data_ptr(), o["base"].data_ptr(), o["dx"].data_ptr(), o["dy"].data_ptr(), n, xy.data_ptr(),
                     tab.data_ptr() if table else None, tab.shape[0] if table else 0, copies[dtype].data_ptr() if table else None, lib.dtype_code(dtype))
        return fn

    def trial(o):
        lib.call("fb_mt_wolfe_trial", o["theta"].data_ptr(), o["base"].data_ptr(), o["dx"].data_ptr(), n, 0.1)

    def torch_point(o):
        torch.add(o["base"], o["dx"] * xy[0] + o["dy"] * xy[1], out=o["theta"])

    cands = (("point_bf16", point(torch.bfloat16, True)), ("point_f32", point(torch.float32, True)), ("point_offset_only", point(torch.float32, False)),
             ("wolfe_trial", trial), ("torch_offset", torch_point))
    floor = dict(point_bf16=16 + 2 * in_layers / n, point_f32=16 + 4 * in_layers / n, point_offset_only=16, wolfe_trial=12, torch_offset=16)
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
            res[name] = dict(us=s, floor_bytes_per_element=floor[name], GBps_against_the_floor=floor[name] * n / (s["median"] * 1e-6) / 1e9)
        for k in ("point_bf16", "point_f32", "point_offset_only"):
            res[f"{k}_rate_over_trial_rate"] = res[k]["GBps_against_the_floor"] / res["wolfe_trial"]["GBps_against_the_floor"]
        out[label] = res
        print(json.dumps({label: res}), flush=True)
    out.update(n=n, elements_in_layers=in_layers, sets=sets, flush_bytes=FLUSH_BYTES, reps=reps, warmup=warmup)
    return out


def positions(reps, warmup, images, block, pixels):
    from fullbatchtraining_amd.visualization import block_statistics, compute_randomized_directions, staged_engine
    from fullbatchtraining_amd.cfg import compose

    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(images, 3, pixels, pixels, generator=gen)
    y = torch.randint(0, 10, (images,), generator=gen)
    out = {}
    for label, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        model = _resnet18()
        torch.manual_seed(1)
        dx, dy = compute_randomized_directions(model, compose([]).viz)
        eng, patches, labels = staged_engine(model, x, y, block, dtype, torch.device("cuda:0"))
        pieces = eng.landscape_pieces(images, block)
        eng.landscape_begin(dx, dy)
        base, fdx, fdy = eng.ls_base, eng.ls_dx, eng.ls_dy
        grid = [(-0.5 + 0.01 * k, 0.25 - 0.01 * k) for k in range(warmup + reps)]

        def shipped(px, py):
            dev = eng.landscape_point(px, py, patches, labels, block)
            t_enqueued = time.perf_counter()
            host = dev.cpu().numpy()
            return t_enqueued, float(sum(l for l, _ in block_statistics(host, pieces, block, images)))

        def composition(px, py):
            torch.add(base, fdx * px + fdy * py, out=eng.theta)
            total = 0.0
            for i0, n, groups in pieces:           # (evaluate_batch prepares the weights and the BatchNorm coefficients itself, every call)
                loss, _ = eng.evaluate_batch(patches[i0:i0 + n], labels[i0:i0 + n])
                total += loss * groups
            t_enqueued = time.perf_counter()
            float(eng.theta.pow(2).sum())
            return t_enqueued, total

        def forward_only():
            saved = (eng.chunk, eng.valid)
            try:
                for i0, n, groups in pieces:
                    eng.chunk, eng.valid, eng._eval = n, n, True
                    eng.forward(patches[i0:i0 + n], labels[i0:i0 + n], 1, 1, eng.theta, 0)
            finally:
                (eng.chunk, eng.valid), eng._eval = saved, False

        def floor(px, py):
            eng._replayable(("bench-forward", patches.data_ptr(), labels.data_ptr()), forward_only)
            t_enqueued = time.perf_counter()
            return t_enqueued, float(eng.loss[0])

        cands = (("shipped", shipped), ("composition", composition), ("floor", floor))
        times = {name: dict(ms=[], enqueue_ms=[]) for name, _ in cands}
        check = {}
        for i, (px, py) in enumerate(grid):
            for name, fn in (cands if i % 2 == 0 else cands[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t_enqueued, value = fn(px, py)
                t1 = time.perf_counter()
                check.setdefault(i, {})[name] = value
                if i >= warmup:
                    times[name]["ms"].append((t1 - t0) * 1e3)
                    times[name]["enqueue_ms"].append((t_enqueued - t0) * 1e3)
        eng.landscape_end()
        res = {name: dict(ms_per_position=_stat(t["ms"]), enqueue_ms=_stat(t["enqueue_ms"]), positions_per_s=1e3 / statistics.median(t["ms"]))
               for name, t in times.items()}
        res["composition_over_shipped"] = res["composition"]["ms_per_position"]["median"] / res["shipped"]["ms_per_position"]["median"]
        res["shipped_over_floor"] = res["shipped"]["ms_per_position"]["median"] / res["floor"]["ms_per_position"]["median"]
        res["sum_of_block_losses_shipped_vs_composition"] = [[check[i]["shipped"], check[i]["composition"]] for i in (warmup, warmup + reps - 1)]
        res.update(passes=len(pieces), images_per_pass=pieces[0][1], launches_in_the_list=len(next(v for k, v in eng.cmdlists.items() if k[0] == "landscape")))
        out[label] = res
        print(json.dumps({label: res}), flush=True)
        del eng, patches, labels
        torch.cuda.empty_cache()
    out.update(images=images, block=block, pixels=pixels, reps=reps, warmup=warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--positions", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--position-reps", type=int, default=12)
    ap.add_argument("--images", type=int, default=49_920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("landscape_bench: no GPU visible -- nothing is measured without one")
    summary = dict(device=torch.cuda.get_device_name(0))
    if args.kernel:
        summary["kernel"] = kernel(args.reps, args.warmup, args.sets)
    if args.positions:
        summary["positions"] = positions(args.position_reps, 3, args.images, 128, 32)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as handle:
            json.dump(summary, handle, indent=1)


if __name__ == "__main__":
    main()
