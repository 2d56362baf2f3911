"""The loss-landscape cruncher end to end on the GPU (fullbatchtraining_amd/visualization.py, ``Engine.landscape_point``) against runs of the REAL
reference's ``crunch`` (tests/golden/landscape.npz, written by tests/golden/make_golden_landscape.py).  Per scenario -- ``landscape_2d`` (3 x 3,
filter / biasbn) and ``landscape_1d`` (5 points, layer, the BatchNorm affine parameters move with the point) -- the engine trains the two steps
itself, saves the checkpoint, and a fresh container is crunched from it:

  * at every position train_loss and full_loss within 2e-4 relative of the reference's float64 run, the number of correct images equal (the
    generator admits a scenario only where the reference's own fp32 run is within half of that, counts the same images, and every top-2 logit
    gap is 8 logit differences wide);
  * the bf16 run: finite, and the same argmin position as the fp32 run (admitted only where the minimum leads by 4 bf16 loss tolerances);
  * (0, 0) equals the engine's own evaluation of the checkpoint, block by block, bit for bit;
  * a second run over the finished store evaluates nothing; a run over a half-filled store evaluates only the missing positions and ends with the
    bits of the uninterrupted run;
  * afterwards arena, container and running statistics hold the bits from before; ``Engine.evaluate_batch`` is never called; one replayed list
    serves every position after the first.

One module-scoped run per scenario feeds all of these."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests.helpers import make_data

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETUP = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
SCENARIOS = ("landscape_2d", "landscape_1d")
KEYS = ("train_loss", "train_acc", "full_loss")


@pytest.fixture(scope="module")
def golden_landscape():
    with open(os.path.join(HERE, "golden", "meta_landscape.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "golden", "landscape.npz"))), meta


class Spy:
    """Wraps the engine's landscape methods: counts the evaluated points and replays, keeps the engine and the bits it started from; any call of
    ``Engine.evaluate_batch`` fails the run."""

    def __init__(self):
        from fullbatchtraining_amd.engine import Engine
        self.cls, self.points, self.engines, self.before, self.after, self.replays = Engine, [], [], [], [], []
        self.inner = {k: getattr(Engine, k) for k in ("landscape_begin", "landscape_point", "landscape_end", "evaluate_batch")}

    def __enter__(self):
        spy, inner = self, self.inner

        def snapshot(eng):
            return dict(theta=eng.theta.clone(), running_mean=eng.running_mean.clone(), running_var=eng.running_var.clone(), tracked=eng.num_batches_tracked)

        def begin(eng, dx, dy):
            spy.engines.append(eng)
            spy.before.append(snapshot(eng))
            spy.replays.append(eng.replays)
            return inner["landscape_begin"](eng, dx, dy)

        def point(eng, x, y, *args):
            spy.points.append((float(x), float(y)))
            return inner["landscape_point"](eng, x, y, *args)

        def end(eng):
            out = inner["landscape_end"](eng)
            torch.cuda.synchronize()
            spy.after.append(snapshot(eng))
            spy.replays[-1] = eng.replays - spy.replays[-1]
            return out

        def evaluate_batch(eng, *args):
            raise AssertionError("the cruncher went through Engine.evaluate_batch")

        self.cls.landscape_begin, self.cls.landscape_point, self.cls.landscape_end, self.cls.evaluate_batch = begin, point, end, evaluate_batch
        return self

    def __exit__(self, *exc):
        for k, v in self.inner.items():
            setattr(self.cls, k, v)
        return False


def _crunch(sc, tmp, name, extra=(), seed=None):
    """A fresh container crunched from the checkpoint in ``tmp`` -> (cfg, model, store, spy)."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.visualization import crunch

    cfg = compose(list(sc["overrides"]) + [f"data.pixels={sc['pixels']}", "impl.validate_every_nth_step=1000", f"impl.checkpoint.name={name}.pth"]
                  + list(extra), original_cwd=tmp, name=name)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(sc["n"], sc["pixels"])
    torch.manual_seed(sc["direction_seed"] if seed is None else seed)
    with Spy() as spy:
        store = crunch(model, (x, y), None, SETUP, cfg)
    return cfg, model, store, spy


@pytest.fixture(scope="module")
def runs(golden_landscape, tmp_path_factory):
    """name -> everything the tests below look at, computed once."""
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import train
    from fullbatchtraining_amd.visualization import grid_positions, load_surface

    _, meta = golden_landscape
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        sc = meta["scenarios"][name]
        tmp = str(tmp_path_factory.mktemp(name))
        cfg = compose(list(sc["overrides"]) + [f"data.pixels={sc['pixels']}", "impl.validate_every_nth_step=1000", f"impl.checkpoint.name={name}.pth"],
                      original_cwd=tmp, name=name)
        torch.manual_seed(sc["model_seed"])
        trained = construct_model(cfg.model, 3, 10)
        x, y = make_data(sc["n"], sc["pixels"])
        train(trained, (x, y), (x[:64], y[:64]), SETUP, cfg)
        checkpoint = torch.load(os.path.join(tmp, "checkpoints", f"{name}.pth"), map_location="cpu", weights_only=False)
        assert checkpoint[4] == 2
        cfg, model, store, spy = _crunch(sc, tmp, name)
        positions = grid_positions(cfg.viz)
        out = dict(sc=sc, tmp=tmp, cfg=cfg, model=model, store=store, spy=spy, positions=positions, surface=load_surface(store.path, positions),
                   checkpoint=checkpoint, data=(x, y))
        cache[name] = out
        return out

    return get


@pytest.mark.parametrize("name", SCENARIOS)
def test_landscape_matches_the_reference_f32(golden_landscape, runs, name):
    data, meta = golden_landscape
    run = runs(name)
    sc, surface, positions = run["sc"], run["surface"], run["positions"]
    tol = sc["judged_at"]
    assert tol == 2e-4 and positions == data[f"{name}/positions"].tolist() and run["spy"].points == [tuple(p) for p in positions]
    r64, r32 = data[f"{name}@f64/stats"], data[f"{name}/stats"]
    for k, p in enumerate(positions):
        got = {key: float(surface[key][k]) for key in KEYS}
        correct = got["train_acc"] * sc["n"]
        print(f"{name} {p}: engine {got} ({correct:.0f} correct) ref32 {r32[k].tolist()} ref64 {r64[k].tolist()} ({int(data[f'{name}/correct'][k])} correct); "
              f"relative to ref64: train_loss {abs(got['train_loss'] - r64[k, 0]) / abs(r64[k, 0]):.2e} full_loss {abs(got['full_loss'] - r64[k, 2]) / abs(r64[k, 2]):.2e}")
    for k, p in enumerate(positions):
        got = {key: float(surface[key][k]) for key in KEYS}
        assert abs(got["train_loss"] - r64[k, 0]) <= tol * abs(r64[k, 0]), (p, "train_loss", got, r64[k])
        assert abs(got["full_loss"] - r64[k, 2]) <= tol * abs(r64[k, 2]), (p, "full_loss", got, r64[k])
        assert got["train_acc"] * sc["n"] == int(data[f"{name}/correct"][k]), (p, "correct images", got, int(data[f"{name}/correct"][k]))
    assert sc["weight_decay"] > 0 and all(float(surface["full_loss"][k]) > float(surface["train_loss"][k]) for k in range(len(positions)))


@pytest.mark.parametrize("name", SCENARIOS)
def test_landscape_leaves_arena_container_and_statistics_alone(runs, name):
    run = runs(name)
    spy, model, checkpoint = run["spy"], run["model"], run["checkpoint"]
    assert len(spy.engines) == 1 and len(spy.before) == len(spy.after) == 1
    before, after = spy.before[0], spy.after[0]
    for key in ("theta", "running_mean", "running_var"):
        assert torch.equal(before[key].view(torch.int32), after[key].view(torch.int32)), key
    assert before["tracked"] == after["tracked"] == int(checkpoint[1]["stem.1.num_batches_tracked"]) > 0
    state = model.state_dict()
    assert list(state) == list(checkpoint[1])
    for key, value in checkpoint[1].items():
        assert torch.equal(state[key].cpu(), value.cpu()), f"the container's {key} is not the checkpoint's"
    assert all(p.grad is None for p in model.parameters())
    # one recorded list: every position after the first is a replay (the weight copies of landscape_end are a list of their own)
    assert spy.replays[0] >= len(run["positions"]) - 1, spy.replays


@pytest.mark.parametrize("name", SCENARIOS)
def test_origin_equals_the_engines_own_evaluation(runs, name):
    """(0, 0) is the checkpoint: its train_loss has the bits of ``Engine.evaluate_batch`` on the same engine, block by block."""
    from fullbatchtraining_amd.engine import stem_patches
    run = runs(name)
    eng, (x, y), positions = run["spy"].engines[0], run["data"], run["positions"]
    k = positions.index([0.0, 0.0])
    block = run["cfg"].data.batch_size
    step_loss, correct = np.float32(0), 0.0
    for i in range(0, x.shape[0], block):
        loss, c = eng.evaluate_batch(stem_patches(x[i:i + block].cuda(), eng.plan.stem, eng.dt), y[i:i + block].cuda())
        step_loss, correct = np.float32(step_loss + np.float32(loss)), correct + c
    want = float(step_loss) / (x.shape[0] // block)
    print(f"{name}: (0, 0) train_loss {float(run['store'].get([0.0, 0.0])['train_loss'])!r}, evaluate_batch {want!r}")
    assert run["store"].get([0.0, 0.0])["train_loss"] == want
    assert run["store"].get([0.0, 0.0])["train_acc"] == correct / x.shape[0]
    assert float(run["surface"]["train_loss"][k]) == np.float32(want)


@pytest.mark.parametrize("name", SCENARIOS)
def test_finished_and_half_filled_stores(runs, name):
    from fullbatchtraining_amd.visualization import LossStore, load_surface
    run = runs(name)
    sc, tmp, positions = run["sc"], run["tmp"], run["positions"]
    # a finished store: nothing is evaluated, nothing is drawn, the results stay
    _, _, store, spy = _crunch(sc, tmp, name, seed=12345)
    assert spy.points == [] and store.path == run["store"].path and len(store) == len(positions)
    # a half-filled one (the same immutable part, the first results only): the missing positions alone, then the bits of the uninterrupted run
    half = run["store"].path.replace(f"{name}_", f"{name}half_")
    shutil.copytree(run["store"].path, half)
    keep = len(positions) // 2
    with open(os.path.join(half, "results.json")) as handle:
        rows = json.load(handle)["results"]
    with open(os.path.join(half, "results.json"), "w") as handle:
        json.dump({"results": rows[:keep]}, handle)
    assert len(LossStore(half)) == keep
    _, _, resumed, spy = _crunch(sc, tmp, name, extra=[f"viz.database_name={name}half.pth"], seed=12345)
    assert resumed.path == half and spy.points == [tuple(p) for p in positions[keep:]]
    a, b = load_surface(half, positions), run["surface"]
    for key in KEYS:
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key


@pytest.mark.parametrize("name", SCENARIOS)
def test_landscape_bf16_has_the_same_argmin(runs, name):
    from fullbatchtraining_amd.visualization import load_surface
    run = runs(name)
    sc, tmp, positions = run["sc"], run["tmp"], run["positions"]
    _, _, store, spy = _crunch(sc, tmp, name, extra=["impl.mixed_precision=True", f"viz.database_name={name}bf16.pth"])
    assert spy.engines[0].dt == torch.bfloat16 and len(spy.points) == len(positions)
    surface = load_surface(store.path, positions)
    print(f"{name} bf16 train_loss {surface['train_loss'].tolist()} fp32 {run['surface']['train_loss'].tolist()}")
    for key in KEYS:
        assert bool(torch.isfinite(surface[key]).all()), key
    assert int(surface["train_loss"].argmin()) == int(run["surface"]["train_loss"].argmin())
    assert torch.equal(spy.before[0]["theta"].view(torch.int32), spy.after[0]["theta"].view(torch.int32))
