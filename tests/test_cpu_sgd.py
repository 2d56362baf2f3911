"""Mini-batch SGD mode (``hyp.train_stochastic``), host side: the float64 restatement of the reference's stochastic branch
(tests/sgd_ref.py) against the reference's own float64 runs (tests/golden/scenarios_sgd.npz, written by tests/golden/make_golden_sgd.py),
the scope check of the trainer, and the entry points the mode adds to the library's table."""
import json
import os
import re

import numpy as np
import pytest
import torch

from fullbatchtraining_amd.cfg import compose
from fullbatchtraining_amd.models import construct_model
from oracle import fb_oracle as orc
from tests import sgd_ref
from tests.helpers import hyp_from_cfg, loader_pass_indices, make_data, rel_err, shuffling_loaders, summarise

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64
FB_ERR_ARG = -1          # include/fb_engine.h, fb_status
SCENARIOS = ["sgd_shuffle_reg", "sgd_plain", "sgd_ragged", "sgd_smooth"]


@pytest.fixture(scope="module")
def golden_sgd():
    data = np.load(os.path.join(HERE, "golden", "scenarios_sgd.npz"))
    with open(os.path.join(HERE, "golden", "meta_sgd.json")) as handle:
        meta = json.load(handle)
    return data, meta


def test_golden_scenarios_are_admissible(golden_sgd):
    """The reference's fp32 and float64 runs agree within 1e-3 on train_loss, full_loss and param_norm at every recorded step -- otherwise
    the bound max(tol |r64|, 5 |r32 - r64|) of the engine tests hides errors (mini-batch trajectories on random images are chaotic)."""
    data, meta = golden_sgd
    assert set(meta["scenarios"]) == set(SCENARIOS) and meta["spread_limit"] == 1e-3
    for name in SCENARIOS:
        assert all(o.startswith(("hyp=base_sgd", "model=resnet20")) for o in meta["scenarios"][name]["overrides"][:2])
        for stat in ("train_loss", "full_loss", "param_norm"):
            r32, r64 = data[f"{name}/stat/{stat}"], data[f"{name}@f64/stat/{stat}"]
            spread = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
            assert spread < 1e-3 and abs(spread - meta["spread"][name][stat]) <= 1e-12, (name, stat, spread)
        assert "preclip_gradnorm" not in list(data[f"{name}/stat_keys"]) and "clipped_step" not in list(data[f"{name}/stat_keys"])
    # the scenarios chosen here (all but the given sgd_shuffle_reg): a second, engine-free fp32 evaluation -- the restatement with torch's CPU
    # kernels -- lands within half the tolerance the engine tests judge the scenario at (tests/golden/make_golden_sgd.py)
    assert meta["judged_at"] == {"sgd_shuffle_reg": 3e-3, "sgd_plain": 2e-4, "sgd_ragged": 2e-4, "sgd_smooth": 2e-4}
    for name in ("sgd_plain", "sgd_ragged", "sgd_smooth"):
        assert all(meta["spread_restatement_fp32"][name][k] < meta["judged_at"][name] / 2 for k in ("train_loss", "full_loss", "param_norm")), name
        assert meta["spread_restatement_fp32"][name]["grad_norm_train_max"] < max(meta["judged_at"][name], 1e-3) / 2, name


@pytest.mark.parametrize("name", SCENARIOS)
def test_restatement_reproduces_the_reference_in_float64(golden_sgd, name):
    data, meta = golden_sgd
    sc = meta["scenarios"][name]
    cfg = compose(sc["overrides"] + [f"data.pixels={sc['pixels']}"])
    assert cfg.hyp.train_stochastic is True
    torch.manual_seed(sc["model_seed"])
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(sc["n"], sc["pixels"])
    x = x.to(F64)
    state = {k: (v.clone().to(F64) if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    net = sgd_ref.Net(cfg.model, model)
    order_fn = before_eval = None
    if "shuffle" in name:
        tl, vl = shuffling_loaders(x, y, cfg.data.batch_size)
        order_fn = lambda step: loader_pass_indices(tl)                                           # noqa: E731
        before_eval = lambda: torch.empty((), dtype=torch.int64).random_(generator=vl.generator)  # noqa: E731
    block = min(cfg.data.batch_size, sc["n"])
    stats = sgd_ref.train_sgd(net, state, x, y, hyp_from_cfg(cfg), cfg.hyp.steps, block, cfg.hyp.scheduler, cfg.hyp.warmup, Xv=x, Yv=y,
                              validate_every=1000, order_fn=order_fn, before_eval=before_eval)
    key = f"{name}@f64"
    keys = [k for k in data[f"{key}/stat_keys"]]
    assert sorted(k for k in stats if k not in ("lr", "_momentum")) == sorted(keys)       # the same statistics, no preclip_gradnorm / clipped_step
    for stat in keys:
        assert np.allclose(stats[stat], data[f"{key}/stat/{stat}"], rtol=1e-7, atol=1e-12), (stat, stats[stat], data[f"{key}/stat/{stat}"])
    assert len([k for k in keys if k.startswith("grad_norm_train_")]) == sc["n"] // block
    _, samp = summarise([state[k].to(F64) for k in model.state_dict().keys()])
    assert rel_err(samp, data[f"{key}/final_sample"]) < 1e-7
    assert rel_err(state["fc.bias"].numpy(), data[f"{key}/final_fc_bias"]) < 1e-7
    assert rel_err(state["stem.1.running_mean"].numpy(), data[f"{key}/final_stem_running_mean"]) < 1e-9
    assert int(state["stem.1.num_batches_tracked"]) == int(data[f"{key}/final_num_batches_tracked"][0])


def test_torch_clip_coef_is_the_form_of_clip_grad_norm():
    gen = torch.Generator().manual_seed(3)
    grads = [torch.randn(5, 7, generator=gen, dtype=F64), torch.randn(11, generator=gen, dtype=F64)]
    norm = float(torch.cat([g.reshape(-1) for g in grads]).norm())
    for clip in (0.5 * norm, norm * (1 + 1e-9), norm * (1 - 1e-9), 3 * norm):
        params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, clip, norm_type=2.0)
        coef = float(sgd_ref.torch_clip_coef(grads, clip))
        assert coef == min(1.0, clip / (norm + 1e-6)) or abs(coef - min(1.0, clip / (norm + 1e-6))) < 1e-15
        for p, g in zip(params, grads):
            assert torch.allclose(p.grad, g * coef, rtol=1e-14, atol=0)
    assert float(sgd_ref.torch_clip_coef(grads, norm)) < 1.0          # norm == clip: the torch form scales, `if norm > clip` does not


# ---------------------------------------------------------------------------------------------------------------------- scope --
def test_check_scope_accepts_the_default_configuration():
    from fullbatchtraining_amd.training import _check_scope
    cfg = compose([])
    assert cfg.hyp.train_stochastic is True and cfg.hyp.template_name == "baseline"
    _check_scope(cfg, branch="stochastic")
    _check_scope(compose(["hyp.grad_clip=0.5", "hyp.grad_reg.block_strength=0.5", "hyp.label_smoothing=0.1", "impl.mixed_precision=True"]), branch="stochastic")
    _check_scope(compose(["hyp=fb1"]))
    with pytest.raises(NotImplementedError, match="does not select"):      # (asked about the full-batch branch, its default, as before)
        _check_scope(cfg)
    with pytest.raises(NotImplementedError, match="does not select"):
        _check_scope(compose(["hyp=fb1"]), branch="stochastic")


@pytest.mark.parametrize("over,needle", [
    (["hyp/optim_modification=SAM"], "optim_modification"),
    (["hyp/optim_modification=LARS"], "optim_modification"),
    (["hyp.grad_reg.acc_strength=0.25"], "pre_grads=None"),
    (["hyp.batch_clip=1.0"], "_record_stats"),
    (["hyp.train_semi_stochastic=True"], "LMDB"),
    (["hyp.train_switch_stochastic=0"], "never resets"),
    (["hyp.only_linear_layers_weight_decay=True"], "one weight decay"),
])
def test_check_scope_names_what_is_out_of_scope(over, needle):
    from fullbatchtraining_amd.training import _check_scope
    with pytest.raises(NotImplementedError, match=re.escape(needle)):
        _check_scope(compose(over), branch="stochastic")
    if "train_switch_stochastic" in over[0]:                               # ... whichever branch is asked about
        with pytest.raises(NotImplementedError, match="inverts hyp.train_stochastic for the whole run"):
            _check_scope(compose(["hyp=fb1"] + over))


def test_check_scope_refuses_more_than_one_rank(monkeypatch):
    from fullbatchtraining_amd.training import _check_scope
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _check_scope(compose([]), branch="stochastic")


# ---------------------------------------------------------------------------------------------------------------- entry table --
def test_entry_table_lists_the_sgd_entry_points():
    """``fb_mt_sgd_prep`` / ``fb_mt_sgd_torch`` with the signatures the compiler derived from the header's prototypes, recordable; the
    ``_supported`` query is a host function; the library and the binding are at ABI 17."""
    from fullbatchtraining_amd import lib
    h = lib.load()
    assert lib.EXPECTED_ABI == 17 == h.fb_abi_version()
    table = {h.fb_entry_name(i).decode(): (h.fb_entry_sig(i).decode(), h.fb_entry_kind(i)) for i in range(h.fb_entry_count())}
    #          theta grad mom n gnorm2 clip lr wd mu damp nesterov first | tab n_layers w_fwd w_dgrad dtype | stream
    assert table["fb_mt_sgd_prep"] == ("i:ppplpfffffii" + "pippi" + "p", 2)
    assert table["fb_mt_sgd_torch"] == ("i:ppplpfffffii" + "p", 2) and table["fb_mt_sgd_torch"][0] == table["fb_mt_clip_sgd"][0]
    assert table["fb_mt_sgd_prep_supported"] == ("i:ii", 0)
    for name in ("fb_mt_sgd_prep", "fb_mt_sgd_torch"):
        fn = h.fb_cmd_fn_id(name.encode())
        assert fn >= 0 and h.fb_cmd_fn_nargs(fn) == len(table[name][0]) - 2 == len(lib._SIGS[name])
    assert h.fb_cmd_fn_id(b"fb_mt_sgd_prep_supported") == -1
    assert h.fb_mt_sgd_prep_supported(lib.FB_F32, 0) == 1 and h.fb_mt_sgd_prep_supported(lib.FB_BF16, 0) == 1
    assert h.fb_mt_sgd_prep_supported(lib.FB_F32, 1) == 0 and h.fb_mt_sgd_prep_supported(7, 0) == 0
    header = open(os.path.join(os.path.dirname(HERE), "include", "fb_engine.h")).read()
    assert re.search(r"int fb_mt_sgd_prep\(float\* theta, const float\* grad, float\* mom, int64_t n, const float\* gnorm2, float grad_clip", header)


def test_sgd_prep_refuses_bad_arguments_without_a_device():
    """Null pointers and an unsupported dtype are refused before anything touches the device (no GPU needed)."""
    from fullbatchtraining_amd import lib
    h = lib.load()
    common = (1024, None, -1.0, 0.1, 0.0, 0.9, 0.0, 1, 0)
    assert h.fb_mt_sgd_prep(None, 16, 16, *common, None, 0, None, None, lib.FB_F32, None) == FB_ERR_ARG
    assert h.fb_mt_sgd_prep(16, None, 16, *common, None, 0, None, None, lib.FB_F32, None) == FB_ERR_ARG
    assert h.fb_mt_sgd_prep(16, 16, None, *common, None, 0, None, None, lib.FB_F32, None) == FB_ERR_ARG            # momentum 0.9 without a buffer
    assert h.fb_mt_sgd_prep(16, 16, 16, 1024, None, 0.5, 0.1, 0.0, 0.9, 0.0, 1, 0, None, 0, None, None, lib.FB_F32, None) == FB_ERR_ARG   # clip without the norm
    assert h.fb_mt_sgd_prep(16, 16, 16, *common, None, 1, 16, 16, lib.FB_F32, None) == FB_ERR_ARG                  # a layer row without a table
    assert h.fb_mt_sgd_prep(16, 16, 16, *common, 16, 1, None, 16, lib.FB_F32, None) == FB_ERR_ARG                  # ... without the forward copy
    assert h.fb_mt_sgd_prep(16, 16, 16, *common, None, 0, None, None, 7, None) == FB_ERR_ARG
    assert h.fb_mt_sgd_prep(16, 20, 16, *common, None, 0, None, None, lib.FB_F32, None) == FB_ERR_ARG              # 16-byte alignment
    assert h.fb_mt_sgd_prep(16, 16, 16, *common, None, 513, 16, 16, lib.FB_F32, None) == FB_ERR_ARG
    assert b"fb_mt_sgd_prep" in h.fb_last_error_string()
    assert h.fb_mt_sgd_torch(None, 16, 16, *common, None) == FB_ERR_ARG
