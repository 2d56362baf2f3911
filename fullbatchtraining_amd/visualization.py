"""Loss-landscape cruncher (``cfg.viz``): the surface of the reference's ``fullbatch/visualization`` package on the engine.

``crunch(model, trainloader, validloader, setup, cfg)`` evaluates the full-batch training loss, in ``model.eval()`` arithmetic, at every point
``theta* + x dx + y dy`` of the 1-D or 2-D grid of ``cfg.viz.coordinates`` along two normalised random directions and files the results in a
store under ``<cfg.original_cwd>/checkpoints``.  A point costs one replay of one recorded launch list (``Engine.landscape_point``: the fused
point kernel ``fb_mt_landscape_point``, the BatchNorm coefficients, every forward pass) and one read-back.

What differs from the reference, on purpose:
  * the store is a directory ``<base>_<ignore_layers>_<norm>_losses.fbdb`` instead of an LMDB file (same naming rule for ``<base>``): an immutable
    part written once (``immutable.pt``: the state dict and both directions, in the reference's layouts) and ``results.json``, rewritten through a
    temporary file and ``os.replace`` after every read-back.  The LMDB tuning keys of ``cfg.viz`` are accepted and ignored;
  * the reference sleeps for a random time of up to ten seconds before its first position so that several processes that share an LMDB do not
    start on the same key.  One process owns a store here: the sleep is dropped;
  * afterwards the arena holds the checkpoint again, bit for bit; the container and the running statistics are never written (the reference
    leaves the model at the last grid point);
  * more than one rank, ``viz.compute_full_loss`` with ``grad_reg.block_strength != 0`` and an augmenting train loader are refused (see ``crunch``);
    nothing here plots (``plot_1d_loss_err_row``).
"""
import json
import logging
import os
import shutil
import time

import numpy as np
import torch

from .training import _device_augmentation, _stage, optim_interface

log = logging.getLogger(__name__)

NORMS = ("filter", "layer", "weight", "dfilter", "dlayer")
STORE_SUFFIX = ".fbdb"
_IMMUTABLE, _RESULTS = "immutable.pt", "results.json"
_KEYS = ("train_loss", "train_acc", "full_loss")


# ----------------------------------------------------------------------------------------------------------------------
# directions
# ----------------------------------------------------------------------------------------------------------------------
def normalize_direction(direction, weights, norm="filter", eps=1e-10):
    """Rescale ``direction`` in place against ``weights`` (one parameter tensor each, more than one dimension):
    ``filter``: every slice along dimension 0 gets the norm of the same slice of the weights, |w_f| / (|d_f| + eps);
    ``layer``: the tensor gets the norm of the weights; ``weight``: every entry is multiplied by its weight;
    ``dfilter``: every slice along dimension 0 gets unit norm, 1 / (|d_f| + eps); ``dlayer``: the tensor gets unit norm."""
    if norm not in NORMS:
        raise ValueError(f"viz.norm {norm!r}: one of {NORMS}")
    with torch.no_grad():
        if norm == "filter":
            for f in range(direction.shape[0]):
                direction[f].mul_(weights[f].norm() / (direction[f].norm() + eps))
        elif norm == "dfilter":
            for f in range(direction.shape[0]):
                direction[f].div_(direction[f].norm() + eps)
        elif norm == "layer":
            direction.mul_(weights.norm() / direction.norm())
        elif norm == "dlayer":
            direction.div_(direction.norm())
        else:
            direction.mul_(weights)
    return direction


def compute_randomized_directions(model, cfg_viz):
    """Two random directions in the layout of ``model.parameters()``.  Each: one ``randn_like`` per parameter, in order, THEN the tensors with more
    than one dimension are normalised (``cfg_viz.norm``) and the others are zeroed (``ignore_layers == 'biasbn'``) or become a copy of the weights."""
    def one():
        params = list(model.parameters())
        with torch.no_grad():
            drawn = [torch.randn_like(p) for p in params]
            for d, w in zip(drawn, params):
                if d.dim() > 1:
                    normalize_direction(d, w.detach(), cfg_viz.norm)
                elif cfg_viz.ignore_layers == "biasbn":
                    d.zero_()
                else:
                    d.copy_(w)
        return drawn

    x_direction = one()
    return x_direction, one()


# ----------------------------------------------------------------------------------------------------------------------
# store
# ----------------------------------------------------------------------------------------------------------------------
def store_path(cfg_impl, cfg_viz, original_cwd):
    """The reference's naming rule with the store's own suffix."""
    base_name = cfg_impl.checkpoint.name if cfg_viz.database_name is None else cfg_viz.database_name
    if base_name is None:
        base_name = "debug_db_"
    full_name = os.path.splitext(base_name)[0] + f"_{cfg_viz.ignore_layers}_{cfg_viz.norm}_losses{STORE_SUFFIX}"
    return os.path.join(original_cwd, "checkpoints", full_name)


def _replace_into(path, write):
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as handle:
        write(handle)
        handle.flush()
        os.fsync(handle.fileno())
    os.replace(tmp, path)


class LossStore:
    """The results of one store: {(x, y): {train_loss, train_acc, full_loss}}.  ``put`` rewrites ``results.json`` atomically; leftovers of an
    interrupted rewrite (``results.json.tmp.*``) are never read."""

    def __init__(self, path):
        self.path, self.results = path, {}
        file = os.path.join(path, _RESULTS)
        if os.path.isfile(file):
            with open(file) as handle:
                for x, y, *values in json.load(handle)["results"]:
                    self.results[(float(x), float(y))] = dict(zip(_KEYS, (float(v) for v in values)))

    @staticmethod
    def key(position):
        return float(position[0]), float(position[1])

    def get(self, position):
        return self.results.get(self.key(position))

    def put(self, position, **values):
        self.results[self.key(position)] = {k: float(values[k]) for k in _KEYS}
        rows = [[x, y, *(v[k] for k in _KEYS)] for (x, y), v in self.results.items()]
        _replace_into(os.path.join(self.path, _RESULTS), lambda handle: handle.write(json.dumps({"results": rows}).encode()))

    def __len__(self):
        return len(self.results)


def load_loss_database(model, cfg_impl, cfg_viz, original_cwd, setup, log=log):
    """Create the store (new directions) or reuse it -> (store, x_direction, y_direction), the directions on ``setup['device']``.  A reused store
    must hold the state dict of ``model``, tensor for tensor.  ``viz.rebuild_existing_database`` removes an existing store first."""
    db_path = store_path(cfg_impl, cfg_viz, original_cwd)
    if cfg_viz.rebuild_existing_database and os.path.isdir(db_path):
        shutil.rmtree(db_path)
    file = os.path.join(db_path, _IMMUTABLE)
    if not os.path.isdir(db_path):
        log.info(f"Creating new database at {db_path}.")
        os.makedirs(db_path)
        x_direction, y_direction = compute_randomized_directions(model, cfg_viz)
        payload = dict(model_state_dict={k: v.detach().cpu() for k, v in model.state_dict().items()},
                       x_direction=[d.cpu() for d in x_direction], y_direction=[d.cpu() for d in y_direction])
        _replace_into(file, lambda handle: torch.save(payload, handle))
        log.info(f"Database written successfully at {db_path}.")
    else:
        log.info(f"Reusing cached database at {db_path}.")
    try:
        payload = torch.load(file, map_location=setup["device"], weights_only=False)
        stored, x_direction, y_direction = payload["model_state_dict"], payload["x_direction"], payload["y_direction"]
    except Exception as exc:                       # no immutable part, or one that does not load: the creation never finished
        raise ValueError(f"The provided LMDB dataset at {db_path} is unfinished or damaged.") from exc
    own = model.state_dict()
    if list(own) != list(stored):
        raise AssertionError(f"the store at {db_path} holds another model: its state dict has other keys")
    for key in own:
        if not torch.equal(own[key].detach().cpu(), stored[key].detach().cpu()):
            raise AssertionError(f"the store at {db_path} holds another model: {key} differs")
    return LossStore(db_path), x_direction, y_direction


def load_surface(db_path, positions):
    """-> dict(train_loss, train_acc, full_loss) of float32 tensors [len(positions)], NaN where the store has no result for a position."""
    landscape = {k: torch.full((len(positions),), float("nan")) for k in _KEYS}
    store = LossStore(db_path)
    for idx, position in enumerate(positions):
        value = store.get(position)
        if value is not None:
            for key in _KEYS:
                landscape[key][idx] = value.get(key, float("nan"))
    return landscape


load_surface_from_lmdb = load_surface            # (the reference's name for it)


def plot_1d_loss_err_row(*args, **kwargs):
    raise NotImplementedError("plotting is not part of the engine: read the surface with load_surface(db_path, positions) and plot it with any tool "
                              "(the reference's plot_1d_loss_err_row needs matplotlib, which this package does not depend on)")


# ----------------------------------------------------------------------------------------------------------------------
# the cruncher
# ----------------------------------------------------------------------------------------------------------------------
def grid_positions(cfg_viz):
    """[[x, y], ...] in the reference's order (x outer, y inner): ``torch.linspace`` in float32, read as Python floats."""
    c = cfg_viz.coordinates
    xcoords = torch.linspace(c.x.min, c.x.max, c.x.num)
    ycoords = torch.linspace(c.y.min, c.y.max, c.y.num)
    return [[x.item(), y.item()] for x in xcoords for y in ycoords]


def status_message(train_loss, train_acc, full_loss, time_stamp, current_position):
    return (f"Pos: [{float(current_position[0]):4.2f}, {float(current_position[1]):4.2f}] | Time: {time_stamp:4.2f}s |"
            f"TRAIN loss {train_loss:7.4f} | TRAIN Acc: {train_acc:7.2%} |"
            f"Full loss {full_loss:7.4f} |")


def check_scope(cfg, trainloader=None):
    """What the cruncher refuses, each with its reason."""
    if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise NotImplementedError("loss landscape on more than one rank: the reference's own distributed path dies on zeros_like(model.parameters()) "
                                  "(crunch.py:51), so there is nothing to reproduce; run one process per store")
    if cfg.hyp.grad_reg.acc_strength != 0:
        raise ValueError("Loss landscape does not contain acc_strength!")
    if cfg.viz.compute_full_loss and cfg.hyp.grad_reg.block_strength != 0:
        raise NotImplementedError("viz.compute_full_loss with grad_reg.block_strength != 0: the regulariser's term of the full loss needs the gradient "
                                  "norm of every block in eval mode, and the engine's backward pass exists in training mode only; set "
                                  "viz.compute_full_loss=False or hyp.grad_reg.block_strength=0")
    if cfg.viz.norm not in NORMS:
        raise ValueError(f"viz.norm {cfg.viz.norm!r}: one of {NORMS}")
    if _device_augmentation(cfg, trainloader) is not None:
        raise NotImplementedError("an augmenting train loader (impl.engine.device_augment): every position would see other images; the landscape is "
                                  "evaluated on the images as staged once")


def block_statistics(host, pieces, block, datapoints):
    """Per block of the loader, in order: [(mean loss as numpy.float32, correct images)] from a position's read-back ``host`` (the layout of
    ``Engine.landscape_point``) and the ``pieces`` it was cut into.  A block larger than one forward pass arrives in pieces: its mean is the
    image-weighted mean of theirs, formed in double and rounded once."""
    n_out = sum(groups for _, _, groups in pieces)
    losses, corrects, slot, out = host[:n_out], host[n_out:2 * n_out], 0, []
    part_loss, part_correct, part_n = 0.0, 0.0, 0
    for i0, n, groups in pieces:
        size = min(block, datapoints - i0 // block * block)          # images of the block this piece starts in
        if groups > 1 or n == size:
            out += [(np.float32(losses[slot + g]), float(corrects[slot + g])) for g in range(groups)]
        else:
            part_loss, part_correct, part_n = part_loss + float(losses[slot]) * n, part_correct + float(corrects[slot]), part_n + n
            if part_n == size:
                out.append((np.float32(part_loss / size), part_correct))
                part_loss, part_correct, part_n = 0.0, 0.0, 0
        slot += groups
    return out


def crunch(model, trainloader, validloader, setup, cfg):
    """The reference's ``crunch`` (crunch.py:18-172) in one process on one GPU; see the module docstring for what differs (no start-up sleep,
    a directory store, the arena restored).  Returns the store."""
    check_scope(cfg, trainloader)
    device = setup["device"] if isinstance(setup["device"], torch.device) else torch.device(setup["device"])
    model.eval()
    optimizer, _ = optim_interface(model, cfg.hyp)

    if cfg.impl.checkpoint.name is not None:
        file = os.path.join(cfg.original_cwd, "checkpoints", cfg.impl.checkpoint.name)
        optim_state, model_state, _, _, step = torch.load(file, map_location="cpu", weights_only=False)
        model.load_state_dict(model_state)
        optimizer.load_state_dict(optim_state)
        log.info(f"Loaded model checkpoint from step {step} successfully.")
    else:
        step = 0
        cfg.impl.checkpoint.name = cfg.name
        log.info("No checkpoint supplied! Loss landscape will be computed for the model initialization without training.")
    weight_decay = float(getattr(cfg.hyp.optim, "weight_decay", 0.0))

    # the images in loader order, staged once (a tensor pair drops its ragged tail like the trainer; a loader yields what it yields)
    X, Y = _stage(trainloader, None)
    block = min(int(cfg.data.batch_size), X.shape[0])
    if isinstance(trainloader, (tuple, list)):
        X, Y = X[:X.shape[0] // block * block], Y[:X.shape[0] // block * block]
    elif getattr(trainloader, "batch_size", None):
        block = min(int(trainloader.batch_size), X.shape[0])
    datapoints = X.shape[0]
    num_blocks = -(-datapoints // block)

    store, x_direction, y_direction = load_loss_database(model, cfg.impl, cfg.viz, cfg.original_cwd, dict(setup, device="cpu"), log)

    positions = grid_positions(cfg.viz)
    if all(store.get(position) is not None for position in positions):     # a finished store: no engine, no staging
        for position in positions:
            log.info(f"Skipping loss at position {position}")
        return store

    dtype = torch.bfloat16 if cfg.impl.mixed_precision else torch.float32
    eng, patches, labels = staged_engine(model, X, Y, block, dtype, device, int(cfg.impl.get("engine", {}).get("chunk_group", 98)))
    pieces = eng.landscape_pieces(datapoints, block)
    n_out = sum(g for _, _, g in pieces)

    eng.landscape_begin(x_direction, y_direction)
    try:
        for position in positions:
            if store.get(position) is not None:
                log.info(f"Skipping loss at position {position}")
                continue
            train_time = time.time()
            host = eng.landscape_point(position[0], position[1], patches, labels, block).cpu().numpy()      # the position's one host wait
            stats = block_statistics(host, pieces, block, datapoints)
            assert len(stats) == num_blocks, (len(stats), num_blocks)
            step_loss, step_preds = np.float32(0), 0.0
            for loss, correct in stats:            # float32, in loader order: the reference's `step_loss += block_loss`
                step_loss = np.float32(step_loss + loss)
                step_preds += correct
            param_norm = np.float32(host[2 * n_out])
            full_loss = float(np.float32(step_loss / np.float32(num_blocks)) + np.float32(np.float32(0.5 * weight_decay) * param_norm))
            train_loss, train_acc = float(step_loss) / num_blocks, step_preds / datapoints
            time_stamp = time.time() - train_time
            log.info(status_message(train_loss, train_acc, full_loss, time_stamp, position))
            store.put(position, train_loss=train_loss, train_acc=train_acc, full_loss=full_loss)
    finally:
        eng.landscape_end()
    return store


def staged_engine(model, X, Y, block, dtype, device, chunk_group=98):
    """An engine sized for eval-mode passes over the images ``X`` (in blocks of ``block``), their stem patches and labels on the device."""
    from .engine import Engine, Plan, max_group, padded_chunk, stem_patches

    datapoints = X.shape[0]
    plan = Plan(model, X.shape[-1])
    # images per forward pass: whole blocks, as many as impl.engine.chunk_group asks for and the device holds beside the staged patches; of a
    # block larger than that, pieces (eval mode has no per-block statistics: a pass is cut wherever it suits the memory)
    unit = padded_chunk(plan, 1)
    block_pad = padded_chunk(plan, block)
    own = datapoints * plan.stem.hout * plan.stem.wout * plan.stem.cin_pad * torch.empty((), dtype=dtype).element_size()
    cap_images = max_group(plan, unit, dtype, device, reserve_bytes=own) * unit
    if block_pad <= cap_images:
        blocks_per_pass = max(1, min(int(chunk_group), cap_images // block_pad, datapoints // block))
        pass_images = blocks_per_pass * block_pad
    else:
        pass_images = cap_images
    eng = Engine(model, X.shape[-1], pass_images, 1, compute_dtype=dtype, device=device)
    patches = stem_patches(X.to(device), eng.plan.stem, dtype)
    labels = Y.to(device).contiguous()
    return eng, patches, labels
