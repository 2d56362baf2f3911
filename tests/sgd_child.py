"""Child process of tests/test_gpu_sgd_training.py: one ``train()`` run in mini-batch SGD mode in a FRESH process (the update path is chosen
from the environment when the trainer is built), results into an .npz file.

    python -m tests.sgd_child OUT.npz OVERRIDE [OVERRIDE ...]
"""
import sys

import numpy as np
import torch


def main(out, overrides):
    from fullbatchtraining_amd.cfg import compose
    from fullbatchtraining_amd.models import construct_model
    from fullbatchtraining_amd.training import FullBatchTrainer
    from tests.helpers import make_data

    cfg = compose(list(overrides) + ["impl.validate_every_nth_step=1000"])
    torch.manual_seed(5)
    model = construct_model(cfg.model, 3, 10)
    x, y = make_data(4 * cfg.data.batch_size, cfg.data.pixels)
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    trainer = FullBatchTrainer(model, (x, y), (x[:64], y[:64]), setup, cfg)
    for _ in range(cfg.hyp.steps):
        trainer.step()
    trainer.evaluate()
    eng, stats = trainer.engine, trainer.stats
    res = dict(theta=eng.theta.cpu().numpy(), mom=eng.mom.cpu().numpy(), running_mean=eng.running_mean.cpu().numpy(),
               running_var=eng.running_var.cpu().numpy(), num_batches_tracked=np.array([eng.num_batches_tracked]),
               fused=np.array([int(trainer.sgd_fused)]), cmdlists=np.array([len(eng.cmdlists)]), replays=np.array([eng.replays]))
    for key in list(stats.keys()):
        if key != "train_time":
            res[f"stat/{key}"] = np.array(stats[key], dtype=np.float64)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
