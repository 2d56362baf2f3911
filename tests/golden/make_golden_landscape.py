"""Golden vectors of the reference's loss-landscape cruncher (``crunch_loss_landscape.py`` -> ``fullbatch/visualization``), for
``fullbatchtraining_amd/visualization.py`` and ``fb_mt_landscape_point``.

Runs the real reference on CPU through the import harness of ``make_golden.py`` (that file stays as it is).  ``lmdb`` is not installed: an
in-memory stand-in of this file's own goes into ``sys.modules`` (``open`` / ``begin`` / ``get`` / ``put`` / ``replace``, and an empty file at
the path, which is what the reference's ``os.path.isfile`` looks for).  The reference's random start-up sleep is skipped.  Writes

  tests/golden/landscape.npz         direction cases, offset vectors, per-position records of the scenarios
  tests/golden/meta_landscape.json   seeds, case tables, ``offset_form``, the scenario table with the recorded positions and the measured
                                     fp32-vs-float64 figures of the reference itself

Direction cases   every (norm, ignore_layers) pair on the tensors of ``make_golden_agc.OPT_TENSORS``: weights drawn from WEIGHT_SEED, then
                  ``torch.manual_seed(DIRECTION_SEED)`` and the reference's ``compute_randomized_directions``; both directions are stored.
Offset vectors    the reference's ``_set_parameter_offset`` is a closure of ``crunch``: a container of small tensors and one of 259 elements
                  goes through the real ``crunch`` (norm ``weight``, ``ignore_layers`` off, so every direction is dense) on a 3 x 3 grid with
                  non-dyadic coordinates and (0, 0); its ``forward`` files the parameters it is called with.  ``offset_form``: which float32
                  expression reproduces ALL of them bit for bit -- ``mul_mul_add_add`` (four operations, each rounded), ``inner_fma`` (the
                  second product fused into the sum) or ``exact`` (one rounding of the exact value); the generator stops unless exactly the
                  first does.
Scenarios         ResNet-20, 16 px, 128 images in blocks of 64; the checkpoint is written by two full-batch steps of the reference's own
                  ``train()`` (hyp=fb1).  ``landscape_2d``: 3 x 3 over [-r, r]^2, filter / biasbn.  ``landscape_1d``: 5 points,
                  layer / ignore_layers off (the BatchNorm affine parameters move with the point), weight decay 5e-4.  Each has an fp32 run and
                  an ``@f64`` twin that walks the SAME directions (the fp32 run's, cast: ``randn`` draws other numbers in float64).  Per
                  position: train_loss, train_acc, full_loss, the number of correct images, the smallest top-2 logit gap of the float64 run, the
                  largest fp32-vs-float64 logit difference.  Seeds and scalars only.
Admissibility     (a rung of LADDER -- half-width r from 0.5 down, lr of the two steps, model seed -- is refused otherwise and the next one tried;
                  the generator stops when none is left: extend the ladder, never raise a tolerance)  at every position the reference's own
                  fp32-vs-float64 relative spread of train_loss and of full_loss is below JUDGED_AT / 2 = 1e-4, both runs count the same correct
                  images, and the smallest top-2 gap is at least MARGIN x 2 = 8 times the largest logit difference.  On top of the issue's
                  rules: the position of the smallest train_loss leads the runner-up by MARGIN x BF16_LOSS_REL of its value, so that asking a
                  bf16 run for the same argmin is a fair demand too.

Usage:  python tests/golden/make_golden_landscape.py
"""
import io
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_adam import THREADS  # noqa: E402
from make_golden_agc import OPT_TENSORS  # noqa: E402
from make_golden_fista import OPT_SHAPES  # noqa: E402

NORMS = ("filter", "layer", "weight", "dfilter", "dlayer")
IGNORE = ("biasbn", "none")
WEIGHT_SEED, DIRECTION_SEED = 311, 313
OFFSET_SHAPES = OPT_SHAPES + ((259,),)
OFFSET_RANGE = dict(x=(-0.7, 0.7, 3), y=(-0.3, 0.3, 3))
JUDGED_AT, MARGIN = 2e-4, 4.0

_R20 = ["hyp=fb1", "model=resnet20", "hyp.steps=2", "hyp.warmup=0", "data.batch_size=64", "hyp.sub_batch=64"]
# name: (N, pixels, overrides, model seed, direction seed)
SCENARIOS_LANDSCAPE = {
    "landscape_2d": (128, 16, _R20 + ["viz=2d", "viz.norm=filter", "viz.ignore_layers=biasbn"], 101, 401),
    "landscape_1d": (128, 16, _R20 + ["viz=1d", "viz.norm=layer", "viz.ignore_layers=none"], 103, 403),
}
# (min, max, num) of x and of y for a half-width r of the coordinate range
GRIDS = {"landscape_2d": lambda r: dict(x=(-r, r, 3), y=(-r, r, 3)), "landscape_1d": lambda r: dict(x=(-r, r, 5), y=(0, 0, 1))}
# (half-width, lr of the two training steps, model seed) in the order tried; the first admissible rung is used.  The range shrinks from the
# issue's 0.5; a smaller lr brings the reference's own fp32 and float64 checkpoints closer together, as in the other generators.
LADDER = tuple((r, lr, seed) for r in (0.5, 0.25, 0.1) for lr in (0.1, 0.03, 0.01, 0.003, 0.001) for seed in range(6))
# what a bf16 forward pass may move a loss by, relative: the 5e-3 that smoke() allows the bf16 engine on a loss of ln 10
BF16_LOSS_REL = 5e-3 / 2.302585


# ---------------------------------------------------------------------------------------------------------------------- the lmdb stand-in
class _Txn:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def get(self, key, default=None):
        return self.env.data.get(bytes(key), default)

    def put(self, key, value):
        self.env.data[bytes(key)] = bytes(value)
        return True

    replace = put


class _Env:
    def __init__(self):
        self.data = {}

    def begin(self, write=False):
        return _Txn(self)


ENVS = {}


def _open(path, **kwargs):
    if path not in ENVS:
        ENVS[path] = _Env()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "ab").close()
    return ENVS[path]


def install_lmdb():
    sys.modules["lmdb"] = types.SimpleNamespace(open=_open)


def _serialized(obj):
    buffer = io.BytesIO()
    torch.save(obj, buffer)
    return buffer.getvalue()


def _deserialized(data):
    return torch.load(io.BytesIO(data), map_location="cpu", weights_only=False)


def viz_overrides(ranges):
    out = []
    for axis in ("x", "y"):
        lo, hi, num = ranges[axis]
        out += [f"viz.coordinates.{axis}.min={lo}", f"viz.coordinates.{axis}.max={hi}", f"viz.coordinates.{axis}.num={num}"]
    return out


def run_crunch(fullbatch, model, loaders, setup, cfg):
    import time
    sleep, time.sleep = time.sleep, lambda seconds: None
    try:
        fullbatch.visualization.crunch(model, *loaders, setup, cfg)
    finally:
        time.sleep = sleep


def positions_of(cfg):
    c = cfg.viz.coordinates
    xs, ys = torch.linspace(c.x.min, c.x.max, c.x.num), torch.linspace(c.y.min, c.y.max, c.y.num)
    return [[x.item(), y.item()] for x in xs for y in ys]


# ---------------------------------------------------------------------------------------------------------------------- direction cases
class _Bag(torch.nn.Module):
    """Parameters of the given shapes, drawn from ``seed`` (* 0.3), in order."""

    def __init__(self, shapes, seed, dtype=torch.float32):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.tensors = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=gen) * 0.3) for s in shapes])
        self.to(dtype)


def direction_cases(fullbatch):
    from fullbatch.visualization.normalized_directions import compute_randomized_directions
    out, table = {}, []
    for norm in NORMS:
        for ignore in IGNORE:
            bag = _Bag([s for _, s in OPT_TENSORS], WEIGHT_SEED)
            torch.manual_seed(DIRECTION_SEED)
            dx, dy = compute_randomized_directions(bag, types.SimpleNamespace(norm=norm, ignore_layers=ignore))
            for i, (a, b) in enumerate(zip(dx, dy)):
                out[f"dir/{norm}/{ignore}/x/{i}"], out[f"dir/{norm}/{ignore}/y/{i}"] = a.numpy().copy(), b.numpy().copy()
            table.append([norm, ignore])
    return out, table


# ---------------------------------------------------------------------------------------------------------------------- offset vectors
class _Recording(_Bag):
    def __init__(self, shapes, seed, classes=10):
        super().__init__(shapes, seed)
        self.seen, self.classes = [], classes

    def forward(self, inputs):
        self.seen.append([p.detach().clone() for p in self.parameters()])
        total = sum(p.sum() for p in self.parameters())
        return inputs.reshape(inputs.shape[0], -1)[:, :self.classes] * 0 + total


def offset_vectors(fullbatch, compose):
    tmp = tempfile.mkdtemp()
    cfg = compose(["hyp=fb1", "viz=2d", "viz.norm=weight", "viz.ignore_layers=none", "data.batch_size=8"] + viz_overrides(OFFSET_RANGE),
                  original_cwd=tmp, name="offsets", seed=0)
    model = _Recording(OFFSET_SHAPES, WEIGHT_SEED + 1)
    base = [p.detach().clone() for p in model.parameters()]
    x, y = mg.make_data(8, 8)
    torch.manual_seed(DIRECTION_SEED + 1)
    run_crunch(fullbatch, model, mg.loaders(x, y, 8), dict(device=torch.device("cpu"), dtype=torch.float), cfg)
    (env,) = [e for p, e in ENVS.items() if p.startswith(tmp)]
    dx, dy = _deserialized(env.data[b"x_direction"]), _deserialized(env.data[b"y_direction"])
    positions = positions_of(cfg)
    assert len(model.seen) == len(positions) and [0.0, 0.0] in positions
    out = {"offset/positions": np.array(positions, dtype=np.float64)}
    forms = dict(mul_mul_add_add=True, inner_fma=True, exact=True)
    for i, (w, a, b) in enumerate(zip(base, dx, dy)):
        out[f"offset/base/{i}"], out[f"offset/dx/{i}"], out[f"offset/dy/{i}"] = w.numpy().copy(), a.numpy().copy(), b.numpy().copy()
    for k, ((px, py), seen) in enumerate(zip(positions, model.seen)):
        cx, cy = np.float32(px), np.float32(py)
        for i, (w, a, b) in enumerate(zip(base, dx, dy)):
            got = seen[i].numpy()
            out[f"offset/theta/{k}/{i}"] = got.copy()
            w, a, b = w.numpy(), a.numpy(), b.numpy()
            w64, a64, b64 = w.astype(np.float64), a.astype(np.float64), b.astype(np.float64)            # (a product of two float32 is exact in double)
            four = w + ((a * cx) + (b * cy))
            fused = w + ((a * cx).astype(np.float64) + b64 * np.float64(cy)).astype(np.float32)
            exact = (w64 + (a64 * np.float64(cx) + b64 * np.float64(cy))).astype(np.float32)              # (to double precision: the sum is rounded in double first)
            for name, cand in (("mul_mul_add_add", four), ("inner_fma", fused), ("exact", exact)):
                forms[name] &= bool(np.array_equal(cand.view(np.int32), got.view(np.int32)))
    if [k for k, v in forms.items() if v] != ["mul_mul_add_add"]:
        raise SystemExit(f"the offset vectors do not single out the four-operation form: {forms}")
    print("offset form of the reference: mul_mul_add_add", forms, flush=True)
    return out, "mul_mul_add_add"


# ---------------------------------------------------------------------------------------------------------------------- scenarios
def run_scenario(fullbatch, compose, name, dtype, rung, directions=None):
    """Two steps of the reference's train(), then its crunch() from the checkpoint -> (cfg, per-position records, logits [position][image, class],
    the directions the store holds)."""
    n, pixels, overrides, mseed, dseed = SCENARIOS_LANDSCAPE[name]
    half_width, lr, seed_step = rung
    mseed, overrides = mseed + seed_step, overrides + [f"hyp.optim.lr={lr}"]
    tag = name if dtype == torch.float else f"{name}@f64"
    tmp = tempfile.mkdtemp()
    extra = ["impl.accumulation_dtype=double"] if dtype == torch.double else []
    cfg = compose(overrides + viz_overrides(GRIDS[name](half_width)) + extra + ["impl.validate_every_nth_step=1000", f"data.pixels={pixels}",
                                                                    f"impl.checkpoint.name={tag}.pth"], original_cwd=tmp, name=tag, seed=mseed)
    os.makedirs(os.path.join(tmp, "checkpoints"), exist_ok=True)
    x, y = mg.make_data(n, pixels)
    setup = dict(device=torch.device("cpu"), dtype=dtype, memory_format=torch.contiguous_format)
    torch.manual_seed(mseed)
    model = fullbatch.models.construct_model(cfg.model, 3, 10)
    model.to(**setup)
    xs = x.to(dtype)
    fullbatch.training.train(model, *mg.loaders(xs, y, cfg.data.batch_size), setup, cfg)

    fresh = fullbatch.models.construct_model(cfg.model, 3, 10)
    fresh.to(**setup)
    if directions is not None:       # the twin: the store exists already, with the twin's own checkpoint and the fp32 run's directions
        state = torch.load(os.path.join(tmp, "checkpoints", f"{tag}.pth"), map_location="cpu", weights_only=False)[1]
        env = _open(os.path.join(tmp, "checkpoints", f"{tag}_{cfg.viz.ignore_layers}_{cfg.viz.norm}_losses.lmdb"))
        env.data[b"model_state_dict"] = _serialized(state)
        env.data[b"x_direction"] = _serialized([d.to(dtype) for d in directions[0]])
        env.data[b"y_direction"] = _serialized([d.to(dtype) for d in directions[1]])
    logits = []
    handle = fresh.register_forward_hook(lambda module, args, output: logits.append(output.detach().double().clone()))
    torch.manual_seed(dseed)
    try:
        run_crunch(fullbatch, fresh, mg.loaders(xs, y, cfg.data.batch_size), setup, cfg)
    finally:
        handle.remove()
    (env,) = [e for p, e in ENVS.items() if p.startswith(tmp)]
    positions = positions_of(cfg)
    blocks = len(logits) // len(positions)
    assert blocks * len(positions) == len(logits) and blocks == n // cfg.data.batch_size
    records = [pickle.loads(env.data[pickle.dumps([p])]) for p in positions]
    per_position = [torch.cat(logits[k * blocks:(k + 1) * blocks]) for k in range(len(positions))]
    stored = (_deserialized(env.data[b"x_direction"]), _deserialized(env.data[b"y_direction"]))
    return cfg, positions, records, per_position, stored, y


def judge(name, n, positions, rec32, rec64, z32, z64, y):
    rows, why = [], []
    for k, p in enumerate(positions):
        c32, c64 = int((z32[k].argmax(-1) == y).sum()), int((z64[k].argmax(-1) == y).sum())
        top2 = z64[k].topk(2, dim=-1).values
        gap, diff = float((top2[:, 0] - top2[:, 1]).min()), float((z32[k] - z64[k]).abs().max())
        spread = {key: abs(rec32[k][key] - rec64[k][key]) / abs(rec64[k][key]) for key in ("train_loss", "full_loss")}
        assert abs(rec32[k]["train_acc"] * n - c32) < 1e-6 and abs(rec64[k]["train_acc"] * n - c64) < 1e-6
        if not max(spread.values()) < JUDGED_AT / 2:
            why.append(f"position {p}: the reference's own fp32 run is {spread} from its float64 run (limit {JUDGED_AT / 2})")
        if c32 != c64:
            why.append(f"position {p}: {c32} correct images in fp32, {c64} in float64")
        if not gap >= 2 * MARGIN * diff:
            why.append(f"position {p}: smallest top-2 gap {gap:.3e} < {2 * MARGIN} x largest logit difference {diff:.3e}")
        rows.append(dict(position=p, correct=c64, top2_gap=gap, logit_diff=diff, spread=spread,
                         fp32={key: rec32[k][key] for key in ("train_loss", "train_acc", "full_loss")},
                         f64={key: rec64[k][key] for key in ("train_loss", "train_acc", "full_loss")}))
    # the smallest training loss is a position's own, by MARGIN times what a bf16 forward pass may move a loss (BF16_LOSS_REL): the engine tests
    # ask the bf16 run for the same argmin as the fp32 run
    losses = sorted(rec64[k]["train_loss"] for k in range(len(positions)))
    if not losses[1] - losses[0] >= MARGIN * BF16_LOSS_REL * abs(losses[0]):
        why.append(f"the smallest train_loss {losses[0]:.6f} is {losses[1] - losses[0]:.3e} below the runner-up: less than {MARGIN} x {BF16_LOSS_REL:.2e} of it")
    return rows, why


def scenarios(fullbatch, compose):
    out, meta, refused = {}, {}, []
    for name, (n, pixels, overrides, mseed, dseed) in SCENARIOS_LANDSCAPE.items():
        tried = []
        for rung in LADDER:
            cfg, positions, rec32, z32, directions, y = run_scenario(fullbatch, compose, name, torch.float, rung)
            _, positions64, rec64, z64, _, _ = run_scenario(fullbatch, compose, name, torch.double, rung, directions=directions)
            assert positions == positions64
            rows, why = judge(name, n, positions, rec32, rec64, z32, z64, y)
            tried.append(dict(half_width=rung[0], lr=rung[1], model_seed=mseed + rung[2], refused=why))
            print(name, rung, "admissible" if not why else f"refused ({len(why)} reasons, first: {why[0]})", flush=True)
            if not why:
                break
        if why:
            refused.append(f"{name}: no rung of LADDER is admissible -- extend the ladder (smaller range or lr, other seeds), never a tolerance")
            continue
        for row in rows:
            print(name, row, flush=True)
        half_width, lr, seed_step = rung
        for tag, rec in ((name, rec32), (f"{name}@f64", rec64)):
            out[f"{tag}/stats"] = np.array([[r["train_loss"], r["train_acc"], r["full_loss"]] for r in rec], dtype=np.float64)
        out[f"{name}/positions"] = np.array(positions, dtype=np.float64)
        out[f"{name}/correct"] = np.array([r["correct"] for r in rows], dtype=np.int64)
        out[f"{name}/top2_gap"] = np.array([r["top2_gap"] for r in rows], dtype=np.float64)
        out[f"{name}/logit_diff"] = np.array([r["logit_diff"] for r in rows], dtype=np.float64)
        grid = GRIDS[name](half_width)
        meta[name] = dict(n=n, pixels=pixels, overrides=overrides + [f"hyp.optim.lr={lr}"] + viz_overrides(grid), model_seed=mseed + seed_step,
                          direction_seed=dseed, lr=lr, half_width=half_width, ranges=grid, weight_decay=float(cfg.hyp.optim.weight_decay),
                          norm=cfg.viz.norm, ignore_layers=cfg.viz.ignore_layers, judged_at=JUDGED_AT, positions=rows, tried=tried)
    if refused:
        raise SystemExit("\n".join(refused))
    return out, meta


def main():
    torch.set_num_threads(THREADS[0])
    fullbatch = mg.import_reference()
    install_lmdb()
    from fullbatchtraining_amd.cfg import compose

    out, table = direction_cases(fullbatch)
    vectors, form = offset_vectors(fullbatch, compose)
    out.update(vectors)
    records, meta_s = scenarios(fullbatch, compose)
    out.update(records)
    out["offset_form"] = np.array(form)
    np.savez_compressed(os.path.join(HERE, "landscape.npz"), **out)
    meta = dict(threads=THREADS[0], weight_seed=WEIGHT_SEED, direction_seed=DIRECTION_SEED, direction_cases=table,
                direction_tensors=[[k, list(s)] for k, s in OPT_TENSORS], offset_shapes=[list(s) for s in OFFSET_SHAPES],
                offset_weight_seed=WEIGHT_SEED + 1, offset_range=OFFSET_RANGE, offset_form=form, judged_at=JUDGED_AT, margin=MARGIN,
                scenarios=meta_s, ladder=[list(r) for r in LADDER])
    with open(os.path.join(HERE, "meta_landscape.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote landscape.npz, meta_landscape.json")


if __name__ == "__main__":
    main()
