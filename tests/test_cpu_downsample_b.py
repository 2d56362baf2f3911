"""Host side of the strided 1x1 shortcut (``model.downsample=B``, reference resnets.py:142-146): the parameter container against the
reference's recorded state_dict layout and seeded initial values (tests/golden/make_golden_dsb.py), the two new entry points of the C ABI,
the plan the engine derives from the container, and the container's plain-torch ``forward``."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import summarise

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dsb():
    with open(os.path.join(HERE, "meta_dsb.json")) as handle:
        meta = json.load(handle)
    return dict(np.load(os.path.join(HERE, "scenarios_dsb.npz"))), meta


def _construct(overrides, seed=0):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model

    cfg = compose(overrides)
    torch.manual_seed(seed)
    return cfg, construct_model(cfg.model, 3, 10)


@pytest.mark.parametrize("tag", ["resnet20b", "resnet50b"])
def test_state_dict_layout_and_seeded_init_equal_the_reference(dsb, tag):
    data, meta = dsb
    cfg, model = _construct(meta[f"{tag}_overrides"])
    assert cfg.model.downsample == "B"
    state = model.state_dict()
    assert {k: [list(v.shape), str(v.dtype)] for k, v in state.items()} == meta[f"{tag}_keys"]
    assert list(state) == list(meta[f"{tag}_keys"])                       # ... in the reference's order
    assert any(k.endswith("downsample.0.weight") for k in state) and not any(".downsample.2." in k for k in state)
    got = summarise(list(state.values()))[1]
    assert got.shape == data[f"{tag}/init_sample"].shape and np.array_equal(got, data[f"{tag}/init_sample"])     # 0 ulp


def test_resnet20_preset_carries_the_reference_keys():
    from fullbatchtraining_amd.cfg import compose

    m = compose(["model=resnet20"]).model
    assert dict(m) == dict(name="ResNet20", depth=20, width=16, stem="CIFAR", convolution="Standard", nonlin_fn="ReLU",
                           normalization="BatchNorm2d", downsample="B", initialization="skip-residual")
    _, model = _construct(["model=resnet20"])
    assert [model.layers[s][0].conv1.out_channels for s in range(3)] == [64, 128, 256]           # the width key is not read
    assert model.layers[0][0].downsample is None and len(model.layers[1][0].downsample) == 2


def test_other_shortcut_forms_still_raise():
    for form in ("A", "preact-B", "preact-C"):
        with pytest.raises(NotImplementedError, match="'B'.*'C'"):
            _construct(["model=resnet18", f"model.downsample={form}"])


def test_downsample_c_is_unchanged_by_the_b_form():
    """Same seed: the 'C' container keeps its keys (downsample.1 / .2) and the two forms draw the same initial values (the shortcut's
    convolution has the same shape and the same place in the RNG order)."""
    _, c = _construct(["model=resnet18"])
    _, b = _construct(["model=resnet18", "model.downsample=B"])
    sc, sb = c.state_dict(), b.state_dict()
    assert "layers.1.0.downsample.1.weight" in sc and "layers.1.0.downsample.2.running_var" in sc
    assert [k.replace("downsample.1.", "downsample.0.").replace("downsample.2.", "downsample.1.") for k in sc] == list(sb)
    assert all(torch.equal(u, v) for u, v in zip(sc.values(), sb.values()))


def test_library_exports_the_subsample_calls():
    import __graft_entry__ as entry
    from fullbatchtraining_amd import lib

    entry.build()
    handle = lib.load()
    assert lib.EXPECTED_ABI >= 14 and handle.fb_abi_version() == lib.EXPECTED_ABI        # (the two calls came with v14)
    for name in ("fb_subsample2_fwd", "fb_subsample2_bwd_add"):
        assert name in lib.EXPORTS and hasattr(handle, name)
        fn = handle.fb_cmd_fn_id(name.encode())                            # replayable by the native command-list executor
        assert fn >= 0 and handle.fb_cmd_fn_nargs(fn) == len(lib._SIGS[name]) == 8
    header = open(os.path.join(os.path.dirname(HERE), os.pardir, "include", "fb_engine.h")).read()
    assert "fb_subsample2_bwd_add(void* dx, const void* dy" in header and "resnets.py:142-146" in header


def test_subsample_calls_refuse_bad_arguments_without_a_launch():
    """Argument checks come before the launch, so they answer on a host without a GPU too: a channel count that does not form 16-byte
    vectors, null and misaligned pointers, an empty tensor -> the invalid-argument status."""
    import __graft_entry__ as entry
    from fullbatchtraining_amd import lib

    entry.build()
    h = lib.load()
    FB_ERR_ARG = -1
    for fn in (h.fb_subsample2_fwd, h.fb_subsample2_bwd_add):
        assert fn(4096, 8192, 2, 8, 8, 66, lib.FB_F32, None) == FB_ERR_ARG
        assert b"16-byte vectors" in h.fb_last_error_string()
        assert fn(4096, 8192, 2, 8, 8, 68, lib.FB_BF16, None) == FB_ERR_ARG      # 68 = 17 x 4: fp32 vectors, not bf16 ones
        assert fn(None, 8192, 2, 8, 8, 64, lib.FB_BF16, None) == FB_ERR_ARG
        assert fn(4096, 8200, 2, 8, 8, 64, lib.FB_BF16, None) == FB_ERR_ARG
        assert fn(4096, 8192, 0, 8, 8, 64, lib.FB_BF16, None) == FB_ERR_ARG
        assert fn(4096, 8192, 2, 8, 8, 64, 7, None) == FB_ERR_ARG


@pytest.mark.parametrize("over,pixels,want", [
    (["model=resnet20"], 16, {"layers.1.0": ("B", 2, 16, 8), "layers.2.0": ("B", 2, 8, 4)}),
    (["model=resnet50", "model.stem=standard", "model.downsample=B"], 64,
     {"layers.0.0": ("B", 1, 16, 16), "layers.1.0": ("B", 2, 16, 8), "layers.2.0": ("B", 2, 8, 4), "layers.3.0": ("B", 2, 4, 2)}),
    (["model=resnet18"], 16, {"layers.1.0": ("C", 2, 16, 8), "layers.2.0": ("C", 2, 8, 4), "layers.3.0": ("C", 2, 4, 2)}),
])
def test_plan_takes_shortcut_names_kind_and_size_from_the_model(over, pixels, want):
    from fullbatchtraining_amd.engine import Plan

    _, model = _construct(over)
    plan = Plan(model, pixels)
    got = {}
    for b in plan.blocks:
        if b.shortcut is None:
            assert b.kind is None
            continue
        S = b.shortcut
        prefix = S.conv_name.rsplit(".downsample.", 1)[0]
        ci, ni = (0, 1) if b.kind == "B" else (1, 2)
        assert (S.conv_name, S.bn_name) == (f"{prefix}.downsample.{ci}", f"{prefix}.downsample.{ni}")
        assert (S.R, S.stride, S.pad) == (1, 1, 0) and S.hout == S.hin == b.convs[-1].hout      # executed as a 1x1 stride-1 convolution
        got[prefix] = (b.kind, b.stride, b.hin, S.hin)
    assert got == want
    # the 'B' size rule on an odd map: a strided 1x1 convolution samples ceil(h / 2) positions, AvgPool2d floors
    odd = Plan(_construct(["model=resnet50", "model.stem=standard", "model.downsample=B"])[1], 100)
    sizes = [(b.hin, b.shortcut.hin) for b in odd.blocks if b.shortcut is not None and b.stride == 2]
    assert sizes == [(25, 13), (13, 7), (7, 4)]


def test_host_forward_of_a_b_block_is_the_strided_convolution():
    """``forward`` of the container (plain torch, the float64 yardstick of the GPU tests) on the first downsampling block of ResNet-20/B
    against the block written out by hand with ``conv2d(stride=2)`` as its shortcut -- float64, train-mode BatchNorm."""
    import torch.nn.functional as F

    _, model = _construct(["model=resnet20"])
    blk = copy.deepcopy(model.layers[1][0]).double().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):                        # (gamma = 1, beta = 0 would hide a swapped affine pair)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    p = {k: v.detach() for k, v in blk.state_dict().items()}
    assert p["downsample.0.weight"].shape == (128, 64, 1, 1)
    x = torch.randn(6, 64, 9, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(3))      # odd map: 9 -> 5

    def bn(t, name):
        mean, var = t.mean((0, 2, 3), keepdim=True), t.var((0, 2, 3), unbiased=False, keepdim=True)
        return (t - mean) / torch.sqrt(var + 1e-5) * p[f"{name}.weight"].view(1, -1, 1, 1) + p[f"{name}.bias"].view(1, -1, 1, 1)

    out = torch.relu(bn(F.conv2d(x, p["conv1.weight"], None, 2, 1), "bn1"))
    out = bn(F.conv2d(out, p["conv2.weight"], None, 1, 1), "bn2")
    short = bn(F.conv2d(x, p["downsample.0.weight"], None, 2, 0), "downsample.1")
    want = torch.relu(out + short)
    # the same shortcut as "subsample, then 1x1 stride-1 convolution" -- what the engine runs
    assert torch.allclose(F.conv2d(x, p["downsample.0.weight"], None, 2, 0), F.conv2d(x[:, :, ::2, ::2], p["downsample.0.weight"]), rtol=0, atol=1e-13)
    got = blk(x)
    assert got.shape == (6, 128, 5, 5) and torch.allclose(got, want, rtol=0, atol=1e-12)
    # running statistics moved for the shortcut's BatchNorm too
    assert int(blk.downsample[1].num_batches_tracked) == 1 and float(blk.downsample[1].running_mean.abs().max()) > 0
