"""Counterpart of the reference's crunch_loss_landscape.py: the full-batch training loss on a 1-D or 2-D grid around a checkpoint (or the
initialisation) along normalised random directions, filed in a store under ./checkpoints (fullbatchtraining_amd/visualization.py).

    python crunch_loss_landscape.py [cfg overrides, e.g. viz=2d viz.coordinates.x.num=11 impl.mixed_precision=True impl.checkpoint.name=fb.pth data.size=5120]

Synthetic CIFAR-shaped data (this environment has no dataset access); `data.size` images (default 5120).  Prints one line per position and,
at the end, the position of the smallest training loss.  Read a finished store with `visualization.load_surface(path, positions)`."""
import logging
import sys

import torch

from fullbatchtraining_amd.cfg import compose
from fullbatchtraining_amd.models import construct_model
from fullbatchtraining_amd.visualization import crunch, grid_positions, load_surface


def main():
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    over = [a for a in sys.argv[1:] if not a.startswith("data.size=")]
    size = next((int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("data.size=")), 5120)
    if not any(a.startswith("hyp=") for a in over):
        over = ["hyp=fb1"] + over                      # full-batch GD (the reference's train_stochastic=False branch)
    cfg = compose(over, name="landscape")
    torch.manual_seed(cfg.seed if getattr(cfg, "seed", None) is not None else 0)
    model = construct_model(cfg.model, 3, 10)
    gen = torch.Generator().manual_seed(1234)
    x, y = torch.randn(size, 3, 32, 32, generator=gen), torch.randint(0, 10, (size,), generator=gen)
    setup = dict(device=torch.device("cuda:0"), dtype=torch.float, memory_format=torch.contiguous_format)
    store = crunch(model, (x, y), None, setup, cfg)
    positions = grid_positions(cfg.viz)
    surface = load_surface(store.path, positions)
    best = int(torch.nan_to_num(surface["train_loss"], nan=float("inf")).argmin())
    print(f"{len(store)} of {len(positions)} positions in {store.path}; smallest TRAIN loss {float(surface['train_loss'][best]):.4f} at {positions[best]}")


if __name__ == "__main__":
    main()
