"""Golden vectors for the strided 1x1 shortcut (``model.downsample=B``, reference ``resnets.py:142-146``), produced by running the REAL
reference on the CPU with the harness of ``make_golden.py`` (which stays as it is: its helpers are imported).

Outputs (committed, data only):
  tests/golden/scenarios_dsb.npz   ``dsb_plain`` / ``dsb_gradreg`` (+ their ``@f64`` twins) in the key scheme of scenarios.npz, plus
                                   ``<scenario>/valid64`` = [loss, accuracy] of the final model on the first 64 images, and the strided
                                   samples ``resnet20b/init_sample`` / ``resnet50b/init_sample`` of the seeded initial state
  tests/golden/meta_dsb.json       scenario table, state_dict key / shape / dtype lists of ResNet-20/B and ResNet-50/B

Usage:  python tests/golden/make_golden_dsb.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

SCENARIOS_DSB = {
    # ResNet-20 with the reference's own resnet20.yaml (downsample B), 16 px, chunks of 32; otherwise fb_plain / fb_gradreg
    "dsb_plain": (128, 16, ["hyp=fb1", "model=resnet20", "hyp.steps=3", "hyp.warmup=0", "hyp.optim.lr=0.1", "data.batch_size=32"], 0),
    "dsb_gradreg": (64, 16, ["hyp=fb1", "model=resnet20", "hyp.steps=2", "hyp.warmup=0", "hyp.grad_reg.block_strength=0.5", "data.batch_size=32"], 0),
}
MODELS = {"resnet20b": ["model=resnet20"], "resnet50b": ["model=resnet50", "model.downsample=B"]}


def valid64(model, n, pixels, dtype):
    """Loss and accuracy of the final model in eval mode on the first 64 images (plain cross entropy, reference training.py:343-388)."""
    x, y = mg.make_data(n, pixels)
    x, y = x[:64].to(dtype), y[:64]
    model.eval()
    with torch.no_grad():
        out = model(x)
        loss = torch.nn.functional.cross_entropy(out, y)
        acc = (out.argmax(dim=-1) == y).double().mean()
    return np.array([float(loss), float(acc)])


def main():
    torch.set_num_threads(8)
    fullbatch = mg.import_reference()
    from fullbatchtraining_amd.cfg import compose

    mg.ALL_SCENARIOS.update(SCENARIOS_DSB)
    out = {}
    for name, (n, pixels, _, _) in SCENARIOS_DSB.items():
        for dtype in (torch.float, torch.double):
            _, model = mg.run_scenario(fullbatch, compose, name, out, dtype=dtype)
            out[f"{name if dtype == torch.float else name + '@f64'}/valid64"] = valid64(model, n, pixels, dtype)
    # (the per-chunk probe samples of run_scenario are not used by the tests of these scenarios: their scalars and per-tensor summaries stay)
    out = {k: v for k, v in out.items() if not (k.endswith(("_raw_sample", "_reg_sample", "probe_state_sample")))}
    meta = dict(sample_stride=mg.SAMPLE_STRIDE,
                scenarios={k: dict(n=v[0], pixels=v[1], overrides=v[2], model_seed=v[3]) for k, v in SCENARIOS_DSB.items()})
    for tag, overrides in MODELS.items():
        cfg = compose(overrides)
        torch.manual_seed(0)
        model = fullbatch.models.construct_model(cfg.model, 3, 10)
        state = model.state_dict()
        meta[f"{tag}_keys"] = {k: [list(v.shape), str(v.dtype)] for k, v in state.items()}
        meta[f"{tag}_overrides"] = overrides
        out[f"{tag}/init_sample"] = mg.summarise(list(state.values()))[1]
    np.savez_compressed(os.path.join(HERE, "scenarios_dsb.npz"), **out)
    with open(os.path.join(HERE, "meta_dsb.json"), "w") as handle:
        json.dump(meta, handle, indent=1)
    print("wrote", os.path.join(HERE, "scenarios_dsb.npz"), os.path.join(HERE, "meta_dsb.json"))


if __name__ == "__main__":
    main()
