"""Host side of the loss-landscape cruncher (fullbatchtraining_amd/visualization.py, cfg.viz) against the vectors the reference's own
``crunch`` / ``compute_randomized_directions`` produced (tests/golden/make_golden_landscape.py): the float32 restatement of a grid point, the
directions, the ``viz`` presets and positions, the store, every refusal, and the two rows of the library's entry-point table.  No GPU."""
import json
import logging
import os
import types

import numpy as np
import pytest
import torch

from fullbatchtraining_amd import visualization as viz
from fullbatchtraining_amd.cfg import compose
from tests import landscape_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(HERE, "golden", "landscape.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(HERE, "golden", "meta_landscape.json")) as handle:
        return json.load(handle)


class Bag(torch.nn.Module):
    """The container of the generator's direction cases: parameters of the given shapes drawn from ``seed`` (* 0.3), in order."""

    def __init__(self, shapes, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.tensors = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(tuple(s), generator=gen) * 0.3) for s in shapes])


# ---------------------------------------------------------------------------------------------------------------------- offset, directions
def test_offset_restatement_equals_the_reference_bit_for_bit(vectors, meta):
    assert str(vectors["offset_form"]) == meta["offset_form"] == landscape_ref.FORM
    positions = vectors["offset/positions"]
    assert [0.0, 0.0] in positions.tolist() and len(positions) == 9
    assert any(abs(x * 2 ** 20 - round(x * 2 ** 20)) > 0 for x, _ in positions), "no non-dyadic coordinate"
    n = len(meta["offset_shapes"])
    assert [list(vectors[f"offset/base/{i}"].shape) for i in range(n)] == meta["offset_shapes"] and [259] in meta["offset_shapes"]
    moved, fused_all = 0, True
    for k, (x, y) in enumerate(positions):
        for i in range(n):
            base, dx, dy, want = (vectors[f"offset/{key}/{i}"] for key in ("base", "dx", "dy", f"theta/{k}"))
            got = landscape_ref.offset(base, dx, dy, x, y)
            assert landscape_ref.same_bits(got, want), (k, i)
            if (x, y) == (0.0, 0.0):
                assert landscape_ref.same_bits(got, base)
            else:
                moved += int((got != base).sum())
            # the forms the generator told apart: one fused product, one rounding of the exact value
            fused = base + ((dx * np.float32(x)).astype(np.float64) + dy.astype(np.float64) * np.float64(np.float32(y))).astype(np.float32)
            fused_all &= landscape_ref.same_bits(fused, want)
    assert moved > 0 and not fused_all, "the vectors no longer tell the fused form apart"


def test_directions_equal_the_reference_bit_for_bit(vectors, meta):
    shapes = [s for _, s in meta["direction_tensors"]]
    assert sorted(map(tuple, meta["direction_cases"])) == sorted((n, i) for n in viz.NORMS for i in ("biasbn", "none"))
    threads = torch.get_num_threads()
    torch.set_num_threads(meta["threads"])
    try:
        for norm, ignore in meta["direction_cases"]:
            bag = Bag(shapes, meta["weight_seed"])
            before = [p.detach().clone() for p in bag.parameters()]
            torch.manual_seed(meta["direction_seed"])
            dx, dy = viz.compute_randomized_directions(bag, types.SimpleNamespace(norm=norm, ignore_layers=ignore))
            for axis, got in (("x", dx), ("y", dy)):
                assert len(got) == len(shapes)
                for i, d in enumerate(got):
                    assert landscape_ref.same_bits(d.numpy(), vectors[f"dir/{norm}/{ignore}/{axis}/{i}"]), (norm, ignore, axis, i)
            for i, (p, w) in enumerate(zip(bag.parameters(), before)):
                assert torch.equal(p, w), "the weights are read only"
                if p.dim() <= 1:
                    assert torch.equal(dx[i], torch.zeros_like(p) if ignore == "biasbn" else w)
            assert not any(torch.equal(a, b) for a, b in zip(dx, dy) if a.dim() > 1), "the second direction is a new draw"
    finally:
        torch.set_num_threads(threads)


def test_direction_norms():
    bag = Bag([(5, 3, 3, 3), (4, 6)], 1)
    w = [p.detach() for p in bag.parameters()]
    for norm in viz.NORMS:
        torch.manual_seed(3)
        dx, _ = viz.compute_randomized_directions(bag, types.SimpleNamespace(norm=norm, ignore_layers="biasbn"))
        for d, p in zip(dx, w):
            per_filter, whole = d.flatten(1).norm(dim=1), d.norm()
            if norm == "filter":
                assert torch.allclose(per_filter, p.flatten(1).norm(dim=1), rtol=1e-5)
            elif norm == "layer":
                assert torch.allclose(whole, p.norm(), rtol=1e-5)
            elif norm == "dfilter":
                assert torch.allclose(per_filter, torch.ones_like(per_filter), rtol=1e-5)
            elif norm == "dlayer":
                assert torch.allclose(whole, torch.tensor(1.0), rtol=1e-5)
    with pytest.raises(ValueError, match="viz.norm"):
        viz.normalize_direction(torch.ones(2, 2), torch.ones(2, 2), "rows")


# ---------------------------------------------------------------------------------------------------------------------- presets, positions
REFERENCE_1D = dict(type="1d", database_name=None, rebuild_existing_database=False, compute_full_loss=True, ignore_layers="biasbn", norm="filter",
                    coordinates=dict(x=dict(min=-1, max=1, num=51), y=dict(min=0, max=0, num=1)), model_eval=True, max_readers=128,
                    readahead=True, meminit=False, max_spare_txns=128, map_size=1e9)


def test_viz_presets_compose():
    assert dict(compose([]).viz) == REFERENCE_1D == dict(compose(["viz=1d"]).viz)
    want = dict(REFERENCE_1D, type="2d", meminit=True, coordinates=dict(x=dict(min=-1, max=1, num=51), y=dict(min=-1, max=1, num=51)))
    assert dict(compose(["viz=2d"]).viz) == want
    assert dict(compose(["viz=none"]).viz) == dict(type="none")
    cfg = compose(["viz=2d", "viz.norm=layer", "viz.coordinates.x.num=3", "hyp=fb1"])
    assert cfg.viz.norm == "layer" and cfg.viz.coordinates.x.num == 3 and cfg.hyp.template_name == "fb1"
    assert len(viz.grid_positions(compose(["viz=2d"]).viz)) == 2601 and len(viz.grid_positions(compose([]).viz)) == 51
    with pytest.raises(ValueError, match="Unknown choice"):
        compose(["viz=3d"])


def test_positions_equal_the_recorded_ones(vectors, meta):
    for name, scen in meta["scenarios"].items():
        cfg = compose(scen["overrides"])
        got = viz.grid_positions(cfg.viz)
        assert got == [row["position"] for row in scen["positions"]] == vectors[f"{name}/positions"].tolist(), name
        assert [0.0, 0.0] in got
    two = viz.grid_positions(compose(["viz=2d", "viz.coordinates.x.num=2", "viz.coordinates.y.num=3"]).viz)
    assert two == [[-1.0, -1.0], [-1.0, 0.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 0.0], [1.0, 1.0]], "x outer, y inner"
    tenth = viz.grid_positions(compose(["viz.coordinates.x.num=21"]).viz)[1][0]
    assert tenth == float(torch.linspace(-1, 1, 21)[1]) and tenth != -0.9, "float32 linspace, not a float64 one"


def test_status_message_is_the_references_line():
    line = viz.status_message(2.31461501121521, 0.0859375, 4.445993423461914, 1.2345, [-0.5, 0.25])
    assert line == "Pos: [-0.50, 0.25] | Time: 1.23s |TRAIN loss  2.3146 | TRAIN Acc:   8.59% |Full loss  4.4460 |"


# ---------------------------------------------------------------------------------------------------------------------- store
def _store_cfg(tmp_path, *over):
    return compose(["hyp=fb1", "impl.checkpoint.name=run7.pth", *over], original_cwd=str(tmp_path))


SETUP = dict(device=torch.device("cpu"), dtype=torch.float)


def test_store_create_reuse_mismatch_rebuild(tmp_path, caplog):
    caplog.set_level(logging.INFO)
    cfg = _store_cfg(tmp_path, "viz.norm=layer")
    model = Bag([(5, 3, 3, 3), (7,)], 5)
    torch.manual_seed(0)
    store, dx, dy = viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    path = os.path.join(str(tmp_path), "checkpoints", "run7_biasbn_layer_losses.fbdb")
    assert store.path == path == viz.store_path(cfg.impl, cfg.viz, cfg.original_cwd) and os.path.isdir(path) and len(store) == 0
    assert "Creating new database" in caplog.text and "Database written successfully" in caplog.text
    assert [tuple(d.shape) for d in dx] == [(5, 3, 3, 3), (7,)] and torch.equal(dx[1], torch.zeros(7)) and not torch.equal(dx[0], dy[0])
    store.put([0.5, -0.25], train_loss=1.5, train_acc=0.25, full_loss=float(np.float32(2.1)))
    # reuse: the same directions, the stored result; nothing is drawn
    state = torch.get_rng_state()
    again, dx2, dy2 = viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    assert torch.equal(torch.get_rng_state(), state) and "Reusing cached database" in caplog.text
    assert all(torch.equal(a, b) for a, b in zip(dx + dy, dx2 + dy2))
    assert again.get([0.5, -0.25]) == dict(train_loss=1.5, train_acc=0.25, full_loss=float(np.float32(2.1))) and again.get([0.5, 0.25]) is None
    # another model: refused, as the reference's assert does
    other = Bag([(5, 3, 3, 3), (7,)], 6)
    with pytest.raises(AssertionError, match="another model"):
        viz.load_loss_database(other, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    # rebuild: new directions, no results
    cfg.viz.rebuild_existing_database = True
    rebuilt, dx3, _ = viz.load_loss_database(other, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    assert len(rebuilt) == 0 and not torch.equal(dx3[0], dx[0])


def test_store_names_follow_the_references_rule(tmp_path):
    cfg = _store_cfg(tmp_path)
    assert os.path.basename(viz.store_path(cfg.impl, cfg.viz, "/x")) == "run7_biasbn_filter_losses.fbdb"
    cfg.viz.database_name = "other.name.db"
    assert viz.store_path(cfg.impl, cfg.viz, "/x") == "/x/checkpoints/other.name_biasbn_filter_losses.fbdb"
    cfg.viz.database_name, cfg.impl.checkpoint.name = None, None
    assert os.path.basename(viz.store_path(cfg.impl, cfg.viz, "/x")) == "debug_db__biasbn_filter_losses.fbdb"


def test_store_resume_missing_positions_and_stale_temp_file(tmp_path):
    cfg = _store_cfg(tmp_path)
    model = Bag([(3, 4)], 5)
    store, _, _ = viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    positions = [[-1.0, 0.0], [0.0, 0.0], [1.0, 0.0]]
    third = float(np.float32(1) / np.float32(3))
    store.put(positions[0], train_loss=third, train_acc=0.5, full_loss=2.0)
    store.put(positions[2], train_loss=float("inf"), train_acc=0.0, full_loss=float("nan"))
    assert not [f for f in os.listdir(store.path) if ".tmp" in f], "a finished rewrite leaves no temporary file"
    # an interrupted rewrite: its temporary file is never read
    with open(os.path.join(store.path, "results.json.tmp.99999"), "w") as handle:
        handle.write('{"results": [[0.0, 0.0, 9.0, 9.0')
    surface = viz.load_surface(store.path, positions)
    assert set(surface) == {"train_loss", "train_acc", "full_loss"} and all(v.dtype == torch.float32 and v.shape == (3,) for v in surface.values())
    assert float(surface["train_loss"][0]) == third and torch.isnan(surface["train_loss"][1]) and torch.isinf(surface["train_loss"][2])
    assert torch.isnan(surface["full_loss"][1]) and torch.isnan(surface["full_loss"][2]) and float(surface["train_acc"][0]) == 0.5
    resumed, _, _ = viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    assert len(resumed) == 2 and resumed.get(positions[1]) is None and resumed.get(positions[0])["train_loss"] == third
    assert viz.load_surface_from_lmdb is viz.load_surface


def test_unfinished_store_raises_the_references_error(tmp_path):
    cfg = _store_cfg(tmp_path)
    model = Bag([(3, 4)], 5)
    path = viz.store_path(cfg.impl, cfg.viz, cfg.original_cwd)
    os.makedirs(path)                                    # the creation stopped before the immutable part was in place
    with open(os.path.join(path, "immutable.pt.tmp.99999"), "wb") as handle:
        handle.write(b"half")
    with pytest.raises(ValueError, match="is unfinished or damaged"):
        viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    with open(os.path.join(path, "immutable.pt"), "wb") as handle:
        handle.write(b"not a checkpoint")
    with pytest.raises(ValueError, match="is unfinished or damaged"):
        viz.load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, SETUP)


def test_lmdb_tuning_keys_are_accepted_and_ignored(tmp_path):
    cfg = _store_cfg(tmp_path, "viz.max_readers=1", "viz.readahead=False", "viz.meminit=True", "viz.max_spare_txns=1", "viz.map_size=10")
    store, _, _ = viz.load_loss_database(Bag([(3, 4)], 5), cfg.impl, cfg.viz, cfg.original_cwd, SETUP)
    store.put([0.0, 0.0], train_loss=1.0, train_acc=1.0, full_loss=1.0)
    assert len(viz.LossStore(store.path)) == 1


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_say_why(monkeypatch):
    viz.check_scope(compose(["hyp=fb1"]))
    viz.check_scope(compose(["hyp=fb1", "hyp.grad_reg.block_strength=0.5", "viz.compute_full_loss=False"]))
    with pytest.raises(NotImplementedError, match="eval mode"):
        viz.check_scope(compose(["hyp=gradreg"]))
    with pytest.raises(ValueError, match="Loss landscape does not contain acc_strength!"):
        viz.check_scope(compose(["hyp=fb1", "hyp.grad_reg.acc_strength=0.1"]))
    with pytest.raises(NotImplementedError, match="augmenting train loader"):
        viz.check_scope(compose(["hyp=fb1", "impl.engine.device_augment=True"]))
    with pytest.raises(ValueError, match="viz.norm"):
        viz.check_scope(compose(["hyp=fb1", "viz.norm=rows"]))
    with pytest.raises(NotImplementedError, match="plotting is not part of the engine"):
        viz.plot_1d_loss_err_row("dir", ["a"], ["A"], [0.0], [[0.0, 0.0]])
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="more than one rank.*zeros_like"):
        viz.check_scope(compose(["hyp=fb1"]))
    with pytest.raises(NotImplementedError, match="more than one rank"):
        viz.crunch(None, None, None, dict(device="cpu"), compose(["hyp=fb1"]))


# ---------------------------------------------------------------------------------------------------------------------- pieces of a position
def test_pieces_and_block_statistics():
    from fullbatchtraining_amd.engine import Engine
    eng = types.SimpleNamespace(G=1, chunk=256)
    pieces = Engine.landscape_pieces(eng, 64 * 9 + 10, 64)
    assert pieces == [(0, 256, 4), (256, 256, 4), (512, 64, 1), (576, 10, 1)], "whole blocks per pass, the ragged block on its own"
    assert Engine.landscape_pieces(eng, 128, 64) == [(0, 128, 2)]
    n_out = sum(g for _, _, g in pieces)
    host = np.concatenate([np.arange(n_out, dtype=np.float32) + 0.5, np.arange(n_out, dtype=np.float32) * 2, [7.0, 7.0]]).astype(np.float32)
    stats = viz.block_statistics(host, pieces, 64, 64 * 9 + 10)
    assert stats == [(np.float32(k + 0.5), 2.0 * k) for k in range(10)] and all(isinstance(l, np.float32) for l, _ in stats)
    # a block larger than a pass arrives in pieces: the image-weighted mean, the counts added
    small = types.SimpleNamespace(G=1, chunk=96)
    pieces = Engine.landscape_pieces(small, 300, 128)
    assert pieces == [(0, 96, 1), (96, 32, 1), (128, 96, 1), (224, 32, 1), (256, 44, 1)]
    host = np.array([1.0, 3.0, 2.0, 6.0, 5.0, 10, 20, 30, 40, 50, 0, 0], dtype=np.float32)
    stats = viz.block_statistics(host, pieces, 128, 300)
    assert stats == [(np.float32((1.0 * 96 + 3.0 * 32) / 128), 30.0), (np.float32((2.0 * 96 + 6.0 * 32) / 128), 70.0), (np.float32(5.0), 50.0)]


# ---------------------------------------------------------------------------------------------------------------------- the library's table
def test_abi_rows_of_the_point_kernel():
    from fullbatchtraining_amd import lib
    handle = lib.load()
    assert handle.fb_abi_version() == lib.EXPECTED_ABI == 17, "the point kernel is additive"
    rows = {handle.fb_entry_name(i).decode(): (handle.fb_entry_kind(i), handle.fb_entry_sig(i).decode()) for i in range(handle.fb_entry_count())}
    assert rows["fb_mt_landscape_point"] == (2, "i:pppplppipip"), "recordable; 10 arguments and the stream"
    assert rows["fb_mt_landscape_point_supported"] == (0, "i:ii"), "a host query"
    fn = handle.fb_cmd_fn_id(b"fb_mt_landscape_point")
    assert fn >= 0 and handle.fb_cmd_fn_nargs(fn) == 11 and handle.fb_cmd_fn_id(b"fb_mt_landscape_point_supported") == -1
    assert "fb_mt_landscape_point" in lib._SIGS and "fb_mt_landscape_point_supported" not in lib._SIGS
    assert handle.fb_mt_landscape_point_supported(lib.FB_F32, 0) == 1 and handle.fb_mt_landscape_point_supported(lib.FB_BF16, 0) == 1
    assert handle.fb_mt_landscape_point_supported(lib.FB_F32, 1) == 0 and handle.fb_mt_landscape_point_supported(7, 0) == 0
    header = open(os.path.join(os.path.dirname(HERE), "include", "fb_engine.h")).read()
    assert "int fb_mt_landscape_point(" in header and "int32_t fb_mt_landscape_point_supported(" in header
