"""Drop-in counterpart of the reference's full-batch branch of ``fullbatch.training.train``.

Mirrors, for ``hyp.train_stochastic=False``:
  train                      reference fullbatch/training/training.py:50-75, 217-239, 288-340
  gradient_evaluation        :226-234   (closure: accumulate, stats, clip)          -> Engine.full_gradient / sgd_step
  _accumulate_full_gradient  :121-185
  _record_stats              :85-119    (same keys, same formulas)
  _modify_gradient_params    :187-215   (norm bias, global L2 / L-infinity clip, gradient noise)
  evaluate                   :343-388
  get_loss_fn                :391-413   (cross entropy, label smoothing, incorrect-xent: fused into the head kernel)
  optim_interface            fullbatch/training/optimizers.py:10-93 (what it can select: the table in optimizers.py; cosine-*, warm-up)
  _save_to_checkpoint / _load_from_checkpoint   fullbatch/training/utils.py:43-70 (same 5-list layout)

All arithmetic of a step runs in ``libfbengine.so`` on the GPU; torch optimizers/schedulers are instantiated only as
*state containers* so that ``optimizer.state_dict()`` / ``scheduler.state_dict()`` in checkpoints have the reference's
exact layout and the LR sequence is produced by the same torch code the reference calls.
"""
import logging
import os
import time
from collections import defaultdict

import numpy as np
import torch

from . import lib, optimizers
from .engine import Engine, stem_patches
from .optimizers import (FISTA, LARS, SAM, SGD_AGC, WOLFE_DEFAULTS, GradualWarmupScheduler, WolfeGradientDescent, WolfeSearch, _OptimizerWrapper,  # noqa: F401
                         _scheduler_for, wolfe_constants)     # (the first seven: importers find them here)

log = logging.getLogger("fullbatchtraining_amd")


def optim_interface(model, cfg_hyp):
    """(optimizer, scheduler) as state containers, after the scope check; the descriptor rides along, the scheduler drives the wrapped SGD."""
    optim = optimizers.select(cfg_hyp)
    mod = cfg_hyp.optim_modification.name
    if not optim.search and mod not in ("none", "SAM", "LARS", "LARC"):      # (the search refuses every modification by name)
        raise ValueError(f"Invalid optim_modification {mod} provided.")
    optim.check(cfg_hyp)
    optimizer = optim.container(model, cfg_hyp)
    optimizer.descriptor = optim
    return optimizer, _scheduler_for(optimizer.optim if isinstance(optimizer, _OptimizerWrapper) else optimizer, cfg_hyp)


# ----------------------------------------------------------------------------------------------------------------------
# checkpoints (reference training/utils.py:43-70)
# ----------------------------------------------------------------------------------------------------------------------
def _sync_optimizer_state(engine, model, optimizer):
    """Expose the engine's state as ``optimizer.state`` in the reference layout (a container ``optim_interface`` did not build: SGD's momentum)."""
    getattr(optimizer, "descriptor", optimizers.TABLE["Gradient Descent", "none"]).sync(engine, model, optimizer)


def _save_to_checkpoint(model, optimizer, scheduler, scaler, counter, file="checkpoints/fb.pth", engine=None):
    if engine is not None:
        engine.store_to_model(model)
        _sync_optimizer_state(engine, model, optimizer)
    optim_state, model_state, scheduler_state = optimizer.state_dict(), model.state_dict(), scheduler.state_dict()
    scaler_state = scaler.state_dict() if scaler is not None else None
    torch.save([optim_state, model_state, scheduler_state, scaler_state, counter.step], file)


def _load_from_checkpoint(model, optimizer, scheduler, scaler, counter, max_steps, device=None, file="checkpoints/fb.pth", engine=None):
    try:
        optim_state, model_state, scheduler_state, scaler_state, step = torch.load(file, map_location=device, weights_only=False)
    except FileNotFoundError:
        print("No existing checkpoint found. Starting to train from step 0.")
        return
    model.load_state_dict(model_state)
    optimizer.load_state_dict(optim_state)
    scheduler.load_state_dict(scheduler_state)
    counter.step = step
    if engine is not None:
        engine.load_from_model(model)
        getattr(optimizer, "descriptor", optimizers.TABLE["Gradient Descent", "none"]).load(engine, model, optimizer)
    if step >= max_steps:
        raise ValueError("Maximum step size reached. Terminating computations.")
    print(f"Existing checkpoint loaded successfully. Continuing to train from step {step}.")


# ----------------------------------------------------------------------------------------------------------------------
class _HeadLoss(torch.nn.Module):
    """The loss functions of the reference's ``get_loss_fn`` that the head kernel implements: mean cross entropy with label smoothing
    ``s`` (LabelSmoothCrossEntropyLoss, reference modules.py:86-101) and optionally only on misclassified samples
    (IncorrectCrossEntropyLoss, modules.py:104-119).  Callable like the reference's modules (host-side, for callers that hold a
    loss_fn); the engine reads ``smoothing`` / ``only_incorrect`` and runs the fused kernel."""

    def __init__(self, smoothing=0.0, only_incorrect=False):
        super().__init__()
        self.smoothing, self.only_incorrect = float(smoothing), bool(only_incorrect)

    def forward(self, input, target):
        log_prob = torch.nn.functional.log_softmax(input, dim=-1)
        weight = torch.ones_like(input) * self.smoothing / (input.shape[-1] - 1.0)
        weight.scatter_(-1, target.unsqueeze(-1), (1.0 - self.smoothing))
        loss_per_sample = (-weight * log_prob).sum(dim=-1)
        if self.only_incorrect:
            loss_per_sample = loss_per_sample * (1 - (input.argmax(dim=1) == target).float())
        return loss_per_sample.mean()


def get_loss_fn(cfg_hyp, batch_size):
    """Reference training.py:391-413.  The maxup losses need the augmented-trials layout of the stochastic pipeline (off this path)."""
    smoothing = cfg_hyp.label_smoothing if cfg_hyp.label_smoothing not in [None, ""] else 0.0
    if cfg_hyp.loss_modification is None:
        return torch.nn.CrossEntropyLoss() if smoothing == 0 else _HeadLoss(smoothing)
    if cfg_hyp.loss_modification == "incorrect-xent":
        return _HeadLoss(smoothing, only_incorrect=True)
    if "maxup" in str(cfg_hyp.loss_modification):
        raise NotImplementedError("maxup losses are off the full-batch hot path")
    raise ValueError(f"Invalid loss modification {cfg_hyp.loss_modification}.")


def _is_shuffling(loader):
    """A DataLoader whose sampler is not sequential (the reference's loaders for hyp.shuffle=True): every pass has a new order."""
    return isinstance(loader, torch.utils.data.DataLoader) and not isinstance(loader.sampler, torch.utils.data.SequentialSampler)


def _stage_dataset(loader, device):
    """The DATASET behind a loader, in dataset order, on the device -- read through a private sequential loader so that the
    generator of the caller's loader is not advanced."""
    probe = torch.utils.data.DataLoader(loader.dataset, batch_size=1024, shuffle=False, drop_last=False, generator=torch.Generator())
    xs, ys = zip(*[(x, y) for x, y in probe])
    return torch.cat(xs).to(device), torch.cat(ys).to(device=device, dtype=torch.long)


def _pass_indices(loader):
    """Sample indices of one pass over ``loader`` in its order; advances its generator (or the default one) exactly like the
    reference's ``for ... in trainloader`` does: the DataLoader iterator draws a base seed, then the sampler its permutation."""
    torch.empty((), dtype=torch.int64).random_(generator=loader.generator)
    return torch.tensor([i for batch in loader.batch_sampler for i in batch], dtype=torch.long)


def _stage(loader, device):
    """Materialise a (static, unaugmented) loader as tensors in loader order (drop_last honoured), on ``device`` -- or, with
    ``device=None``, wherever they are (the trainer then moves only its own rank's slice into HBM)."""
    if isinstance(loader, (tuple, list)) and torch.is_tensor(loader[0]):
        X, Y = loader[0], loader[1]
    else:
        xs, ys = [], []
        for x, y in loader:
            xs.append(x)
            ys.append(y)
        X, Y = torch.cat(xs), torch.cat(ys)
    if device is None:
        return X, Y.to(dtype=torch.long)
    return X.to(device), Y.to(device=device, dtype=torch.long)


def _check_scope(cfg, branch="full-batch"):
    """Raises NotImplementedError unless ``cfg`` is in scope of ``branch`` of the reference's ``train()``: "full-batch" (training.py:224-239) or
    "stochastic" (:241-286, the mini-batch SGD mode).  The trainer passes the branch ``hyp.train_stochastic`` selects; a caller that asks for the
    full-batch branch -- the default, what this function has always meant -- with a configuration that selects the other one is refused."""
    hyp = cfg.hyp
    if branch not in ("full-batch", "stochastic"):
        raise ValueError(f"branch {branch!r}: 'full-batch' or 'stochastic'")
    if hyp.train_switch_stochastic is not None:
        raise NotImplementedError("hyp.train_switch_stochastic: the reference never resets the flag it flips (training.py:222-223), so any value >= 0 "
                                  "inverts hyp.train_stochastic for the whole run -- set hyp.train_stochastic itself")
    if bool(hyp.train_stochastic) != (branch == "stochastic"):
        raise NotImplementedError(f"hyp.train_stochastic={bool(hyp.train_stochastic)} does not select the {branch} branch this check was asked about "
                                  "(FullBatchTrainer runs both: it checks the branch the configuration selects)")
    optim = optimizers.select(hyp, refuse=False)    # (what the table does not have is optim_interface's to refuse, after everything here)
    if optim is not None:
        optim.check(hyp)
    if hyp.train_stochastic:         # mini-batch SGD mode (reference training.py:241-286)
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("hyp.train_stochastic on more than one rank (the reference all-reduces every mini-batch gradient; the engine's "
                                      "mini-batch mode runs in one process)")
        if hyp.optim_modification.name != "none":
            raise NotImplementedError(f"hyp.train_stochastic with optim_modification {hyp.optim_modification.name!r} (the mini-batch update is plain "
                                      "clip + SGD in one launch)")
        if hyp.grad_reg.acc_strength != 0:
            raise NotImplementedError("hyp.train_stochastic with grad_reg.acc_strength != 0 (the reference passes pre_grads=None to the regulariser, "
                                      "training.py:265)")
        if hyp.batch_clip is not None:
            raise NotImplementedError("hyp.train_stochastic with hyp.batch_clip (the reference dies in _record_stats, training.py:117-118)")
        if hyp.train_semi_stochastic:
            raise NotImplementedError("hyp.train_semi_stochastic (needs the LMDB rounds of construct_subset_dataloader)")
        if hyp.only_linear_layers_weight_decay:
            raise NotImplementedError("hyp.train_stochastic with only_linear_layers_weight_decay (the mini-batch update takes one weight decay)")
        return
    if hyp.grad_reg.acc_strength != 0 and max(cfg.data.batch_size // hyp.sub_batch, 1) != 1 \
            and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise NotImplementedError("grad_reg.acc_strength with sub_batch < batch_size on several ranks (the pre-pass runs whole blocks; "
                                  "chunk ranges of the ranks would have to be cut at block boundaries)")
    if hyp.batch_clip is not None and float(hyp.grad_clip_norm) != 2.0:
        raise NotImplementedError("hyp.batch_clip with grad_clip_norm != 2 (the per-chunk clip kernel implements the L2 norm)")
    if hyp.grad_clip is not None and not float(hyp.grad_clip_norm) >= 1.0:
        raise NotImplementedError("grad_clip_norm must be a p-norm with p >= 1 (or inf)")


def _device_augmentation(cfg, trainloader):
    """On-device RandomCrop / RandomHorizontalFlip (reference config/data/CIFAR10.yaml:11-13).  Opt-in with
    `impl.engine.device_augment=True`: the caller vouches that the feed (tensor pair or loader) yields UN-augmented, normalised
    images; they stay resident and every step sees a freshly cropped / flipped copy.  Without it a feed is staged once as it comes
    (static dataset), which is also what the reference runs with `data.augmentations_train=` do.
    Returns None or dict(crop_pad, flip_p, pad_value)."""
    aug = cfg.data.get("augmentations_train")
    if not aug:
        return None
    if not bool(cfg.impl.get("engine", {}).get("device_augment", False)):
        log.warning("data.augmentations_train is set: the device-resident feed stages the loader ONCE (static dataset); "
                    "impl.engine.device_augment=True augments un-augmented inputs on the device every step.")
        return None
    out = dict(crop_pad=0, flip_p=0.0, pad_value=None)
    for key in aug.keys():
        if key == "RandomCrop":
            size, pad = (list(aug[key]) + [0])[:2] if not isinstance(aug[key], int) else (aug[key], 0)
            if int(size) != int(cfg.data.pixels):
                raise NotImplementedError(f"RandomCrop to {size} != data.pixels {cfg.data.pixels}")
            out["crop_pad"] = int(pad)
        elif key == "RandomHorizontalFlip":
            out["flip_p"] = float(aug[key])
        else:
            raise NotImplementedError(f"data.augmentations_train.{key}: only RandomCrop and RandomHorizontalFlip run on the device")
    if cfg.data.get("normalize", False):       # RandomCrop pads the raw image with black; the tensors here are normalised
        out["pad_value"] = [-float(m) / float(sd) for m, sd in zip(cfg.data.mean, cfg.data.std)]
    return out


def _evaluate_batch(eng, xb, yb, test_time_flips):
    """Loss sum and #correct of one validation batch (reference training.py:365-380).  ``test_time_flips``: the reference feeds the SUM
    of the softmax outputs of the image and of its horizontal mirror to the loss function and the argmax (training.py:370-373); the
    two forward passes run through the engine (the mirror is taken by the patch-gather kernel), the epilogue is ``fb_head_tta``."""
    if not test_time_flips:
        l, c = eng.evaluate_batch(stem_patches(xb, eng.plan.stem, eng.dt), yb)
        return l * yb.shape[0], c
    n = xb.shape[0]
    eng.evaluate_batch(stem_patches(xb, eng.plan.stem, eng.dt), yb)
    left = eng.logits[:n].clone()
    mirror = torch.ones(n, dtype=torch.int8, device=xb.device)
    eng.evaluate_batch(stem_patches(xb.float().contiguous(), eng.plan.stem, eng.dt, aug=(None, None, mirror, 0, None)), yb)
    ws = torch.empty(2 * n + 2, device=xb.device, dtype=torch.float32)
    lib.call("fb_head_tta", left.data_ptr(), eng.logits.data_ptr(), yb.data_ptr(), n, eng.plan.classes, ws.data_ptr(), ws.data_ptr() + 8 * n,
             ws.data_ptr() + 8 * n + 4)
    loss_sum, correct = ws[2 * n:].tolist()
    return loss_sum, correct


class _Stats(defaultdict):
    """The ``stats`` dict of a run (reference: ``defaultdict(list)``).  The per-step statistics are produced on the GPU and read back
    asynchronously; any READ of the dict first completes the read-backs that are still pending, so a reader always sees every step that
    ``FullBatchTrainer.step`` has returned from -- the reference's semantics (its `_record_stats` syncs) -- while a loop that does not
    look at the statistics between steps (bench.py) keeps the host one step ahead of the GPU instead of idling it for the 2-3 ms of
    host-side bookkeeping per step (7-9 % of a step at 8 GPUs)."""

    def __init__(self, flush):
        super().__init__(list)
        self._flush = flush

    def raw(self, key):
        return defaultdict.__getitem__(self, key)

    def __getitem__(self, key):
        self._flush()
        return defaultdict.__getitem__(self, key)

    def __contains__(self, key):
        self._flush()
        return defaultdict.__contains__(self, key)

    def __iter__(self):
        self._flush()
        return defaultdict.__iter__(self)

    def __len__(self):
        self._flush()
        return defaultdict.__len__(self)

    def keys(self):
        self._flush()
        return defaultdict.keys(self)

    def items(self):
        self._flush()
        return defaultdict.items(self)

    def values(self):
        self._flush()
        return defaultdict.values(self)

    def get(self, key, default=None):
        self._flush()
        return defaultdict.get(self, key, default)

    def __reduce__(self):                      # pickles / copies as a plain dict of lists
        self._flush()
        return (dict, (dict(defaultdict.items(self)),))


class FullBatchTrainer:
    """Owns the engine, the resident dataset and the optimizer/scheduler state containers for one training run."""

    def __init__(self, model, trainloader, validloader, setup, cfg):
        _check_scope(cfg, branch="stochastic" if cfg.hyp.train_stochastic else "full-batch")
        self.cfg, self.model = cfg, model
        self.device = torch.device(setup["device"]) if not isinstance(setup["device"], torch.device) else setup["device"]
        self.optimizer, self.scheduler = optim_interface(model, cfg.hyp)
        self.optim = self.optimizer.descriptor   # (its update runs on the engine's arena; the torch optimizer is the state container the checkpoint layout wants)
        self.loss_fn = get_loss_fn(cfg.hyp, cfg.data.batch_size)
        self.world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
        self.rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        # the multi-process code path (collectives, sharded update); FB_FORCE_DIST=1 takes it with an initialised process group of ONE
        # rank as well, which runs the real RCCL reduce-scatter / all-gather calls on a 1-GPU box (tests/test_gpu_sharded.py)
        self.multi = self.world > 1 or (torch.distributed.is_initialized() and os.environ.get("FB_FORCE_DIST") == "1")
        self.optim.check(cfg.hyp, multi=self.multi)
        # a shuffling train loader: the dataset stays resident in dataset order and every step regathers it in the order of a new
        # pass over the loader's batch sampler (reference: `for block, (inputs, labels) in enumerate(trainloader)` every step)
        self.shuffler = trainloader if _is_shuffling(trainloader) else None
        if self.shuffler is not None:
            Xall, Yall = _stage_dataset(trainloader, self.device)
            per_pass = len(trainloader.batch_sampler) * (trainloader.batch_size or 1) if trainloader.drop_last else len(trainloader.sampler)
            X, Y = Xall[:per_pass], Yall[:per_pass]                   # shapes only; the first step gathers the first permutation
        else:
            X, Y = _stage(trainloader, None)                         # only this rank's chunk range is copied to the device below
        block = min(cfg.data.batch_size, X.shape[0])
        # mini-batch SGD mode: every block of the loader is ONE BatchNorm batch and one update (the stochastic branch has no sub_batch chunking)
        self.stochastic = bool(cfg.hyp.train_stochastic)
        chunks_in_block = 1 if self.stochastic else max(block // cfg.hyp.sub_batch, 1)
        if block % chunks_in_block != 0:
            raise NotImplementedError("data.batch_size must be divisible into equal sub_batch chunks")
        self.chunk, self.block = block // chunks_in_block, block
        self.num_blocks = X.shape[0] // block               # drop_last=True
        self.n_chunks = self.num_blocks * chunks_in_block
        self.datapoints = self.n_chunks * self.chunk
        s = cfg.hyp.grad_reg.block_strength
        impl = cfg.hyp.grad_reg.implementation
        fd = s != 0 or cfg.hyp.grad_reg.acc_strength != 0
        fd_sets = 0 if not fd else (2 if impl == "central-differences" else 1)
        self.dtype = torch.bfloat16 if (cfg.impl.mixed_precision and not fd) else torch.float32
        if cfg.impl.mixed_precision and fd:
            log.warning("grad_reg finite differences need matching fp32 passes (perturbation ~1e-6 per weight): running fp32.")
        from .parallel import ShardPlan, group_size
        self.shard = ShardPlan(self.n_chunks, self.world, self.rank)
        from .engine import Plan, max_group, padded_chunk
        plan = Plan(model, X.shape[-1])
        # chunk sizes that do not fill whole 128-pixel statistics blocks (data.batch_size=125: all 50 000 images in 400 chunks,
        # reference data_preparation.py:64-72) are stored padded with zero images (label -1)
        self.chunk_pad = padded_chunk(plan, self.chunk)
        # what this trainer keeps on the device beside the engine: the stem's patches of the rank's whole shard (and the base images where they are re-augmented)
        es = torch.empty((), dtype=self.dtype).element_size()
        own = self.shard.count * self.chunk_pad * plan.stem.hout * plan.stem.wout * plan.stem.cin_pad * es + self.shard.count * self.chunk * X[0].numel() * 4
        want, cap = int(cfg.impl.get("engine", {}).get("chunk_group", 98)), max_group(plan, self.chunk_pad, self.dtype, self.device, reserve_bytes=own, fd_sets=fd_sets)
        # K-slice counts of the weight gradients are sized for the group of the WHOLE problem on one GPU -- the same number on every rank and in every run, so
        # that a chunk's summation order (hence its gradient, bit for bit) does not depend on the number of GPUs, on what else runs on the device or on the
        # allocator's state: the nominal cap comes from the device's TOTAL memory less what the 1-process run would keep resident (not from free memory, not from
        # this rank's share), and a job of several ranks takes the smallest of its ranks' values
        own_whole = self.n_chunks * self.chunk_pad * plan.stem.hout * plan.stem.wout * plan.stem.cin_pad * es + self.n_chunks * self.chunk * X[0].numel() * 4
        cap_nominal = max_group(plan, self.chunk_pad, self.dtype, self.device, reserve_bytes=own_whole, use_free=False, fd_sets=fd_sets)
        if self.world > 1:
            t = torch.tensor([cap_nominal], dtype=torch.int64, device=self.device if torch.distributed.get_backend() == "nccl" else "cpu")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN)
            cap_nominal = int(t.item())
        nominal = group_size(self.n_chunks, want, cap=cap_nominal)
        # this rank's own group: what is free NOW is a safety clamp on top (a rank's share is never cut larger than the nominal cap allows a whole problem's)
        if cap < min(cap_nominal, max(self.shard.count, 1)):
            log.warning(f"chunk group capped at {cap} chunks by the device's free memory (the nominal cap from its total memory is {cap_nominal}); "
                        "results are unchanged, launches are smaller")
        G = group_size(self.shard.count, want, cap=min(cap, cap_nominal))
        if self.stochastic:                      # one block per gradient: the weights change before the next one
            G = nominal = 1
        log.info(f"chunk groups: {G} chunks per launch on this rank ({self.shard.count} chunks), K-slice counts sized for a nominal group of {nominal}")
        self.engine = Engine(model, X.shape[-1], self.chunk_pad, G, compute_dtype=self.dtype, device=self.device, fd_sets=fd_sets,
                             arena_align=64 * self.world, chunk_valid=self.chunk, nominal_group=nominal,
                             f32_split=str(cfg.impl.get("engine", {}).get("fd_arithmetic", "bf16x6")) if fd else None)
        self.engine.label_smoothing = getattr(self.loss_fn, "smoothing", 0.0)
        self.engine.only_incorrect = getattr(self.loss_fn, "only_incorrect", False)
        stem = self.engine.plan.stem
        lo, hi = self.shard.first * self.chunk, (self.shard.first + self.shard.count) * self.chunk
        self.patches = torch.zeros(self.shard.count * self.chunk_pad, stem.hout, stem.wout, stem.cin_pad, device=self.device,
                                   dtype=self.dtype) if hi > lo else None
        self.augment = _device_augmentation(cfg, trainloader)
        if self.shuffler is not None:
            if self.augment is not None:
                raise NotImplementedError("a shuffling train loader together with impl.engine.device_augment")
            self._all_images, self._all_labels = Xall.float().contiguous(), Yall
        mine = X[lo:hi].to(self.device) if (hi > lo and self.shuffler is None) else None
        self.images = mine.float().contiguous() if (self.augment is not None and mine is not None) else None   # base images stay resident
        self._aug_step, self._n_total, self._lo = 0, X.shape[0], lo
        if mine is not None and self.augment is None:
            self._gather_patches(mine)
        del mine
        self.labels = self._pad_labels(Y[lo:hi].to(self.device)).clone()      # (a buffer of its own: a shuffling feed rewrites it every step)
        if self.stochastic:
            # ONE fixed staging buffer for the block in flight: the recorded launches of a chunk group are keyed by -- and hold -- the address of
            # its patches, so one recorded list (two with the regulariser) serves every block of every epoch
            self.stage_patches = torch.zeros(self.chunk_pad, *self.patches.shape[1:], device=self.device, dtype=self.dtype)
            self.stage_labels = torch.full((self.chunk_pad,), -1, dtype=torch.long, device=self.device)
            self.sgd_fused = self.engine.sgd_prep_fused()
        # a validation DataLoader is read once through a private loader (its generator untouched); every validation pass then advances
        # that generator by the one base-seed draw the reference's pass over it makes (keeps shared generators aligned)
        self._valid_loader = validloader if isinstance(validloader, torch.utils.data.DataLoader) else None
        if self._valid_loader is not None and isinstance(validloader.sampler, torch.utils.data.SequentialSampler):
            self.valid = _stage_dataset(validloader, self.device)
        else:
            self.valid = _stage(validloader, self.device) if validloader is not None else None
        self._pending, self._pinned, self._flushing = [], [], False
        self.stats = _Stats(self.flush_stats)
        self.enqueue_times = []

    # ------------------------------------------------------------------------------------------------------------------
    def step(self):
        """One optimizer step = the reference's ``optimizer.step(gradient_evaluation)`` (training.py:226-237)."""
        cfg, eng, hyp = self.cfg, self.engine, self.cfg.hyp
        train_time = time.time()
        # reference `train_time` = wall time of the gradient evaluation (training.py:112,122), which ends in a device sync there.  Here the host
        # runs a step ahead of the GPU and a step's statistics are read back while the next one is queued, so the step's duration is taken
        # on the DEVICE: from this event (it follows the previous step's last kernel in stream order) to the read-back of the statistics
        self._step_begin = torch.cuda.Event(enable_timing=True)
        self._step_begin.record()
        if self.augment is not None and self.images is not None:
            self._regather_augmented()
        if self.shuffler is not None:
            self._regather_shuffled()
        lr = self.optimizer.param_groups[0]["lr"]
        gr = hyp.grad_reg
        if self.stochastic:
            return self._sgd_epoch(lr, train_time)
        if self.multi:
            self._running0 = torch.stack([eng.running_mean, eng.running_var]).clone()
        mod = hyp.optim_modification.name

        # more than one rank, plain step: the gradient exchange leaves in two buckets, the late one (last stage + classifier) as soon as
        # the last backward pass has left the last stage (parallel.BucketExchange, Engine.full_gradient(late_bucket=...))
        noisy = hyp.grad_noise["additive"] is not None or hyp.grad_noise["multiplicative"] is not None
        replicated = self.multi and (mod == "SAM" or hyp.norm_bias.strength > 0 or hyp.only_linear_layers_weight_decay or noisy
                                     or (hyp.grad_clip is not None and float(hyp.grad_clip_norm) != 2.0))
        exchange = late = None
        if self.multi and not replicated:
            from .parallel import BucketExchange, exchange_bounds, shard_ops
            exchange = BucketExchange(eng.avg, eng.theta, self.shard, shard_ops(self, lr, 0.0 if mod in ("LARS", "LARC") else None),
                                      exchange_bounds(self))
            self._last_exchange = exchange
            if self.shard.count > 0 and os.environ.get("FB_EXCHANGE_OVERLAP", "1") != "0":
                late = (exchange.bounds[1], lambda: exchange.start(1))

        def closure():
            """``gradient_evaluation`` (reference training.py:217-225) up to the clip, which is fused into the consumer of ``eng.avg``."""
            hook = None
            if self.multi and gr.acc_strength != 0:
                from .parallel import reduce_pre_pass
                hook = lambda: reduce_pre_pass(self)          # noqa: E731
            out = eng.full_gradient(self.patches, self.labels, lr, gr.block_strength, gr.eps, gr.implementation, acc_strength=gr.acc_strength,
                                    after_pre_pass=hook, pre_block=self.block // self.chunk * self.chunk_pad, batch_clip=hyp.batch_clip,
                                    late_bucket=late)
            self._pre_sqnorm = None
            if gr.acc_strength != 0:             # |pre_grads|^2 for full_loss (reference training.py:98-101)
                lib.call("fb_mt_norms2", eng.pre.data_ptr(), None, eng.plan.P, eng.norms2.data_ptr(), eng.mt_ws.data_ptr())
                self._pre_sqnorm = eng.norms2[0:1].clone()
            return out

        # more than one rank: the plain step shards the update (reduce-scatter, shard-local clip + SGD, all-gather); the options that
        # need the whole averaged gradient on every rank all-reduce it instead and then run the 1-process code below, replicated
        if replicated:
            from .parallel import replicated_reduce
            local_closure = closure

            def closure():                       # noqa: F811  (the closure of the replicated path includes the exchange)
                self._running0 = torch.stack([eng.running_mean, eng.running_var]).clone()
                return replicated_reduce(self, *local_closure())

        loss_k, correct_k, sq_k = closure()
        if self.multi and not replicated:
            from .parallel import sharded_update
            loss_k, correct_k, sq_k = sharded_update(self, loss_k, correct_k, sq_k, lr,
                                                    weight_decay=0.0 if mod in ("LARS", "LARC") else None, exchange=exchange)
            self._state_is_sharded = True        # momentum / clipped gradient complete only on each rank's shard until gather_state()
        else:
            def modify():
                """``_modify_gradient_params`` up to the clip coefficient (reference training.py:187-204): norm bias on the averaged
                gradient, then the clip norm (L2 or L-infinity) into ``eng.norms2[0]``; ``eng.norms2[1]`` = |theta|^2."""
                eng.grad_and_param_sqnorm()
                if hyp.norm_bias.strength > 0:
                    eng.norm_bias(hyp.norm_bias.strength, hyp.norm_bias.norm_type, hyp.norm_bias.bias)
                    eng.grad_and_param_sqnorm()
                if hyp.grad_clip is not None and float(hyp.grad_clip_norm) == float("inf"):
                    eng.clip_norm_inf()
                elif hyp.grad_clip is not None and float(hyp.grad_clip_norm) != 2.0:
                    eng.clip_norm_p(float(hyp.grad_clip_norm))
                if not noisy:
                    return eng.norms2
                # gradient noise acts on the clipped gradient (reference training.py:205-215): clip in place, then one randn_like per
                # parameter and kind, in the reference's order; the statistics keep the pre-clip norm
                norms = eng.norms2.clone()
                if hyp.grad_clip is not None:
                    eng.apply_clip(hyp.grad_clip)
                for kind in ("additive", "multiplicative"):
                    if hyp.grad_noise[kind] is not None:
                        flat = eng.flatten([torch.randn_like(p) for p in self.model.parameters()])
                        if self.multi:       # every rank must add the same noise: rank 0's draw
                            torch.distributed.broadcast(flat, src=0)
                        eng.grad_noise(flat, hyp.grad_noise[kind], kind == "multiplicative")
                return norms

            clip = None if noisy else hyp.grad_clip          # (already applied in place where noise follows it)
            if self.optim.search:
                self._wolfe_step(closure, modify, clip, lr, train_time, (loss_k, correct_k, sq_k))
                self.scheduler.step()
                return
            norms = modify()
            if mod == "SAM":                     # sam.py:84-92: closure, first_step, closure, second_step; stats are recorded twice
                self._record_stats(loss_k, correct_k, sq_k, norms, lr, train_time)
                if noisy:
                    eng.grad_and_param_sqnorm()  # the ascent step is normalised by the norm of the final (clipped, noisy) gradient
                eng.sam_ascent(self.optimizer.rho, clip)
                loss_k, correct_k, sq_k = closure()
                norms = modify()                 # param_norm of the second record is taken at theta + e_w, like the reference's
                self._record_stats(loss_k, correct_k, sq_k, norms, lr, train_time)
                eng.sam_restore()
                self.optim.update(eng, hyp, lr, clip, optimizer=self.optimizer)
                self.scheduler.step()
                return
            # LARS / LARC: the wrapper zeroes the weight decay around SGD.step(closure) and nothing else survives the closure (see LARS)
            self.optim.update(eng, hyp, lr, clip, zero_wd=mod in ("LARS", "LARC"), optimizer=self.optimizer)
            self._record_stats(loss_k, correct_k, sq_k, norms, lr, train_time)
            self.scheduler.step()
            return
        self._record_stats(loss_k, correct_k, sq_k, eng.norms2, lr, train_time)
        self.scheduler.step()

    def _wolfe_step(self, closure, modify, clip, lr, train_time, first):
        """``WolfeGradientDescent.step(closure)`` (sgd_linesearch.py:285-345).  ``first``: the closure's result at theta0, already evaluated.
        Every evaluation is closure + ``_modify_gradient_params`` with the clip applied IN PLACE (the direction and every phi' use the clipped
        gradient), one statistics record, and ONE read-back that carries the record, phi'(0) and phi'(alpha) together: the search cannot go on
        without the loss and phi', so that wait per evaluation is inherent.  The loss the search compares is the record's ``train_loss``.  No final
        step: the parameters stay at the last evaluated trial point."""
        eng, o = self.engine, self.cfg.hyp.optim

        def finish(result, slot):
            norms = modify()
            if clip is not None:
                eng.apply_clip(clip)
            if slot == 0:
                eng.wolfe_direction(o.weight_decay, o.momentum, o.dampening, o.nesterov)
            else:
                eng.wolfe_phi_grad(o.weight_decay)
            self._record_stats(*result, norms, lr, train_time, extra=eng.wolfe_out)
            self.flush_stats()
            return self.stats.raw("train_loss")[-1], self._extra[slot]

        def evaluate(alpha):
            eng.wolfe_trial(lr, alpha)
            return finish(closure(), 1)

        loss0, phi_grad0 = finish(first, 0)
        self.wolfe = WolfeSearch(*wolfe_constants(o))
        self.optimizer.state["alpha"] = self.wolfe.search(loss0, phi_grad0, evaluate)

    def _sgd_epoch(self, lr, train_time):
        """One "step" of the stochastic branch = one epoch (reference training.py:241-286): per block of the loader the block gradient as one
        BatchNorm batch (|g|^2 of the raw gradient, then the regulariser with the epoch's lr), ``clip_grad_norm_`` (always L2, the torch form),
        the SGD update; ``_modify_gradient_params`` is commented out there, so there is no norm bias, no gradient noise and no
        preclip_gradnorm / clipped_step.  Nothing here waits for the device: losses, hits and norms of the blocks land in device arrays that
        ``_record_stats`` reads back once."""
        eng, hyp, gr = self.engine, self.cfg.hyp, self.cfg.hyp.grad_reg
        nb, cp = self.num_blocks, self.chunk_pad
        f32 = dict(device=self.device, dtype=torch.float32)
        loss_all, correct_all, sq_all = torch.empty(nb, **f32), torch.empty(nb, **f32), torch.empty(nb, **f32)
        # tools/sgd_mode_bench.py: a list here collects one (begin, end) device-event pair per block around the update section
        sections = getattr(self, "sgd_section_events", None)
        for b in range(nb):
            self.stage_patches.copy_(self.patches[b * cp:(b + 1) * cp])
            self.stage_labels.copy_(self.labels[b * cp:(b + 1) * cp])
            # (the first block of an epoch prepares the copies itself: evaluation, an EMA swap or a checkpoint load may have come between)
            loss_k, correct_k, sq_k = eng.full_gradient(self.stage_patches, self.stage_labels, lr, gr.block_strength, gr.eps, gr.implementation,
                                                        weights_prepared=b > 0)
            loss_all[b:b + 1].copy_(loss_k)
            correct_all[b:b + 1].copy_(correct_k)
            sq_all[b:b + 1].copy_(sq_k)
            if sections is not None:
                begin = torch.cuda.Event(enable_timing=True)
                begin.record()
            # ---- the update section: norm, update, compute-dtype copies of the new parameters
            if hyp.grad_clip is not None:        # |avg|^2 of the (regularised) block gradient for the clip
                lib.call("fb_mt_norms2", eng.avg.data_ptr(), None, eng.plan.P, eng.norms2.data_ptr(), eng.mt_ws.data_ptr())
            fused = self.sgd_fused and self.optim.launch is None   # (only plain SGD's update can write the weight copies in the same launch)
            self.optim.update(eng, hyp, lr, hyp.grad_clip, torch_clip=True, fused=fused)
            if not fused:                        # the composition: fb_weight_prep per layer (a recorded list)
                eng.prep_weights(eng.theta, 1)
            if sections is not None:
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                sections.append((begin, end))
        self._pre_sqnorm = None
        norms = eng.grad_and_param_sqnorm()      # param_norm: the parameters after the last update (reference training.py:92)
        self._record_stats(loss_all, correct_all, sq_all, norms, lr, train_time)
        self.scheduler.step()

    def _gather_patches(self, images, aug=None):
        """Stem patches of this rank's images (chunk order) into ``self.patches``; with a padded chunk size every chunk's images go to
        the head of its ``chunk_pad`` rows and the padding rows are (re)zeroed."""
        stem = self.engine.plan.stem
        if self.chunk_pad == self.chunk:
            stem_patches(images, stem, self.dtype, aug=aug, out=self.patches)
            return
        dense = stem_patches(images, stem, self.dtype, aug=aug)
        rows = self.patches.view(self.shard.count, self.chunk_pad, *self.patches.shape[1:])
        rows[:, :self.chunk].copy_(dense.view(self.shard.count, self.chunk, *dense.shape[1:]))
        rows[:, self.chunk:].zero_()

    def _pad_labels(self, labels):
        if self.chunk_pad == self.chunk:
            return labels.contiguous()
        out = torch.full((self.shard.count, self.chunk_pad), -1, dtype=torch.long, device=labels.device)
        out[:, :self.chunk] = labels.view(self.shard.count, self.chunk)
        return out.reshape(-1)

    def gather_state(self):
        """Make the momentum and the averaged-gradient arenas whole on every rank again after sharded updates (a collective; no-op
        for one process or after a replicated update)."""
        if getattr(self, "_state_is_sharded", False):
            from .parallel import gather_sharded_state
            gather_sharded_state(self)
            self._state_is_sharded = False

    def _regather_shuffled(self):
        """A new pass over the shuffling train loader: its batch sampler gives this step's sample order (rank 0's draw on several
        ranks); this rank's slice of it is gathered from the resident dataset and turned into stem patches again."""
        idx = _pass_indices(self.shuffler).to(self.device)
        if self.multi:
            torch.distributed.broadcast(idx, src=0)
        lo, hi = self._lo, self._lo + self.shard.count * self.chunk
        mine = idx[lo:hi]
        if hi > lo:
            self._gather_patches(self._all_images.index_select(0, mine))
            # (into the resident buffer: the recorded launches of a chunk group are keyed by -- and hold -- its address)
            self.labels.copy_(self._pad_labels(self._all_labels.index_select(0, mine)))

    def _regather_augmented(self):
        """A fresh RandomCrop offset / flip per image and step (the reference draws them in its DataLoader workers once per epoch =
        step); drawn for the WHOLE dataset from one seeded CPU generator so that a rank's images get the same augmentation however
        the chunks are sharded, then the stem patches of this rank's images are gathered again on the device."""
        a = self.augment
        seed = self.cfg.seed if getattr(self.cfg, "seed", None) is not None else 0
        gen = torch.Generator().manual_seed(1_000_003 * int(seed) + self._aug_step)
        self._aug_step += 1
        n, lo = self.images.shape[0], self._lo
        oy = ox = fl = None
        if a["crop_pad"] > 0:
            off = torch.randint(0, 2 * a["crop_pad"] + 1, (2, self._n_total), generator=gen, dtype=torch.int8)
            oy, ox = (off[i, lo:lo + n].to(self.device) for i in range(2))
        if a["flip_p"] > 0:
            fl = (torch.rand(self._n_total, generator=gen) < a["flip_p"]).to(torch.int8)[lo:lo + n].to(self.device)
        self._gather_patches(self.images, aug=(oy, ox, fl, a["crop_pad"], a["pad_value"]))

    def _record_stats(self, loss_k, correct_k, sq_k, norms2, lr, train_time, extra=None):
        """Queue the read-back of one closure's statistics (per-chunk losses / hits / squared gradient norms, the two global norms, the
        pre-pass norm, the per-chunk clip count) and finish the records of earlier closures, whose kernels are long done.  ``extra``: device
        scalars that ride along in the same read-back (the line search's phi'); ``self._extra`` holds them once the record is finished."""
        hyp = self.cfg.hyp
        self.enqueue_times.append(time.time() - train_time)         # everything of the step is queued
        pre2 = self._pre_sqnorm if getattr(self, "_pre_sqnorm", None) is not None else torch.zeros(1, device=norms2.device)
        clipped = torch.zeros(1, device=norms2.device)
        if hyp.batch_clip is not None:           # the count the reference means to log (its own line, training.py:118, dies with a NameError)
            clipped = self.engine.clipped_all.sum().reshape(1)
            if self.multi:
                torch.distributed.all_reduce(clipped)
        dev = torch.cat([loss_k, correct_k, sq_k, norms2, pre2, clipped] + ([] if extra is None else [extra]))
        host = self._pinned.pop() if self._pinned and self._pinned[-1].numel() == dev.numel() else torch.empty(dev.numel(), dtype=torch.float32, pin_memory=True)
        host.copy_(dev, non_blocking=True)
        done = torch.cuda.Event(enable_timing=True)
        done.record()
        self._pending.append((host, done, lr, (self._step_begin, done)))
        self.flush_stats(keep=1)

    def flush_stats(self, keep=0):
        """Finish the pending statistics records (all but the ``keep`` newest): wait for their read-back, then the host-side formulas."""
        if self._flushing:
            return
        self._flushing = True
        try:
            while len(self._pending) > keep:
                host, done, lr, train_time = self._pending.pop(0)
                done.synchronize()
                self._finish_record(host, lr, train_time)
                self._pinned.append(host)
        finally:
            self._flushing = False

    def _finish_record(self, host, lr, train_time):
        """Same keys/formulas as reference training.py:85-119 and :205-211."""
        hyp, stats = self.cfg.hyp, self.stats
        K = self.n_chunks
        loss_k, correct_k, sq_k, (gn2, pn2), pre2, clipped = (host[:K], host[K:2 * K], host[2 * K:3 * K], host[3 * K:3 * K + 2], host[3 * K + 2],
                                                              host[3 * K + 3])
        self._extra = host[3 * K + 4:].tolist()
        for idx, entry in enumerate(sq_k.sqrt().tolist()):
            stats.raw(f"grad_norm_train_{idx}").append(entry)
        # sequential fp32 sum, like the reference's `step_loss += chunk_loss` (np.cumsum accumulates strictly left to right)
        step_loss = torch.tensor(float(np.cumsum(loss_k.numpy(), dtype=np.float32)[-1])) if K > 0 else torch.zeros(())
        full_grad_norm = sq_k.mean()
        param_norm = pn2
        train_loss = step_loss / K
        full_loss = train_loss + 0.5 * getattr(hyp.optim, "weight_decay", 0.0) * param_norm
        if hyp.grad_reg.block_strength != 0:
            full_loss = full_loss + lr / 4 * hyp.grad_reg.block_strength * full_grad_norm
        if hyp.grad_reg.acc_strength != 0:
            full_loss = full_loss + lr / 4 * hyp.grad_reg.acc_strength * pre2
        stats.raw("train_loss").append(train_loss.item())
        stats.raw("train_acc").append(correct_k.sum().item() / self.datapoints)
        stats.raw("train_time").append(train_time[0].elapsed_time(train_time[1]) * 1e-3)
        stats.raw("param_norm").append(param_norm.item())
        stats.raw("grad_norm").append(full_grad_norm.sqrt().item())
        stats.raw("full_loss").append(full_loss.item())
        if hyp.batch_clip is not None:
            stats.raw("clipped_batches").append(int(clipped.item()))
        if hyp.grad_clip is not None and not self.stochastic:      # (recorded by _modify_gradient_params, which the stochastic branch does not call)
            grad_norm = gn2.sqrt().item()
            stats.raw("preclip_gradnorm").append(grad_norm)
            stats.raw("clipped_step").append(1 if grad_norm > hyp.grad_clip else 0)

    def evaluate(self, stats=None):
        """Reference training.py:343-388: BN in eval mode, mean CE and accuracy over the validation set (optionally with mirrored inputs)."""
        stats = self.stats if stats is None else stats
        if self.valid is None:
            return stats
        X, Y = self.valid
        if getattr(self, "_valid_loader", None) is not None:     # the reference's pass over the validation loader draws one base seed
            torch.empty((), dtype=torch.int64).random_(generator=self._valid_loader.generator)
        eng = self.engine
        cap = eng.G * eng.chunk
        loss_sum, correct, n = 0.0, 0.0, 0
        ema = bool(self.cfg.hyp.evaluate_ema) and getattr(eng, "theta_ema", None) is not None
        if ema:                                  # eval_model = ema_model (reference training.py:290-292)
            eng.swap_ema()
        try:
            for i in range(0, X.shape[0], cap):
                xb, yb = X[i:i + cap], Y[i:i + cap]
                l, c = _evaluate_batch(eng, xb, yb, bool(self.cfg.hyp.test_time_flips))
                loss_sum += l
                correct += c
                n += yb.shape[0]
                if self.cfg.dryrun:
                    break
        finally:
            if ema:
                eng.swap_ema()
        stats["valid_loss"] += [loss_sum / n]
        stats["valid_acc"] += [correct / n]
        return stats


def evaluate(model, dataloader, stats, setup, impl, hyp, dryrun=False):
    """Validation loss / accuracy of a model (signature of reference training.py:343): BN in eval mode (running statistics),
    mean CE, fraction correct.  Used by verify_model_checkpoint.py; `train` evaluates through its own engine instead."""
    if stats is None:
        stats = defaultdict(list)
    device = setup["device"] if torch.device(setup["device"]).type == "cuda" else torch.device("cuda")
    X, Y = _stage(dataloader, device)
    dtype = torch.bfloat16 if impl.mixed_precision else torch.float32
    batch = min(1024, X.shape[0])
    eng = Engine(model, X.shape[-1], batch, 1, compute_dtype=dtype, device=device)
    loss_sum, correct, n = 0.0, 0.0, 0
    for i in range(0, X.shape[0], batch):
        xb, yb = X[i:i + batch], Y[i:i + batch]
        l, c = _evaluate_batch(eng, xb, yb, bool(getattr(hyp, "test_time_flips", False)))
        loss_sum, correct, n = loss_sum + l, correct + c, n + yb.shape[0]
        if dryrun:
            break
    stats["valid_loss"] += [loss_sum / n]
    stats["valid_acc"] += [correct / n]
    return stats


def status_message(optimizer, stats, step):
    def last(key):
        return stats[key][-1] if len(stats[key]) > 0 else float("NaN")

    return (f'Step: {step:<4}| lr: {optimizer.param_groups[0]["lr"]:.4f} | Time: {stats["train_time"][-1]:4.2f}s |'
            f'TRAIN loss {stats["train_loss"][-1]:7.4f} | TRAIN Acc: {stats["train_acc"][-1]:7.2%} |'
            f'VAL loss {last("valid_loss"):7.4f} | VAL Acc: {last("valid_acc"):7.2%} |')


def _measure_implementation_noise(model, trainloader, validloader, setup, cfg):
    """Floating-point difference between two successive evaluations of the (regularised, clipped) full-batch gradient from the
    same checkpoint -- the protocol of reference training.py:429-600 / measure_floating_point_accuracy.py, same printed lines.
    Every reduction of the engine has a fixed order (no atomics), so the two gradients are bit-identical and the errors are 0.0;
    that is the acceptance test for the deterministic split-K / statistics reductions.  Returns the numbers as a dict."""
    trainer = FullBatchTrainer(model, trainloader, validloader, setup, cfg)
    if trainer.world > 1:
        raise NotImplementedError("_measure_implementation_noise: single-process protocol")
    eng, hyp, optimizer, scheduler = trainer.engine, cfg.hyp, trainer.optimizer, trainer.scheduler

    class Counter:
        step: int = 0

    if cfg.impl.checkpoint.name is None:
        print("Could not load checkpoint. Using newly initalized model.")
        cfg.impl.checkpoint.name = cfg.name
        file = os.path.join(cfg.original_cwd, "checkpoints", cfg.impl.checkpoint.name)
        os.makedirs(os.path.dirname(file), exist_ok=True)
        _save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=file, engine=eng)
    file = os.path.join(cfg.original_cwd, "checkpoints", cfg.impl.checkpoint.name)

    def gradient_evaluation():
        _, model_state, _, _, step = torch.load(file, map_location="cpu", weights_only=False)
        model.load_state_dict(model_state)
        eng.load_from_model(model)                       # parameters and BN buffers as in the checkpoint
        log.info(f"Loaded model checkpoint from step {step} successfully.")
        lr, gr = optimizer.param_groups[0]["lr"], hyp.grad_reg
        loss_k, _, _ = eng.full_gradient(trainer.patches, trainer.labels, lr, gr.block_strength, gr.eps, gr.implementation,
                                         acc_strength=gr.acc_strength)
        if hyp.grad_clip is not None:                    # _modify_gradient_params, clip part (reference :198-211)
            grad_norm = float(eng.grad_and_param_sqnorm()[0].sqrt())
            if grad_norm > hyp.grad_clip:
                lib.call("fb_mt_scale", eng.avg.data_ptr(), eng.plan.P, hyp.grad_clip / (grad_norm + 1e-6))
        return loss_k.mean(), eng.avg.clone()

    loss1, g1 = gradient_evaluation()
    print(f"Completed first pass with loss {loss1.item()}.")
    loss2, g2 = gradient_evaluation()
    print(f"Completed first pass with loss {loss2.item()}.")
    out = dict(loss=[loss1.item(), loss2.item()],
               norm_linf=g1.max().item(), norm_l2=g1.double().pow(2).sum().sqrt().item(), norm_l1=g1.double().abs().sum().item(),
               error_linf=(g1 - g2).max().item(), error_l2=(g1 - g2).double().pow(2).sum().sqrt().item(),
               error_l1=(g1 - g2).double().abs().sum().item())
    print(f"Gradient Norms | L^Inf: {out['norm_linf']} | L2: {out['norm_l2']} | L1: {out['norm_l1']}.")
    print(f"Error in L^inf Norm: Total: {out['error_linf']} | Relative: {out['error_linf'] / out['norm_linf']}.")
    print(f"Error in L^2 Norm: Total: {out['error_l2']} | Relative: {out['error_l2'] / out['norm_l2']}.")
    print(f"Error in L^1 Norm: Total: {out['error_l1']} | Relative: {out['error_l1'] / out['norm_l1']}.")
    return out


def train(model, trainloader, validloader, setup, cfg):
    """Train given model based on implementation details and hyperparameters (signature of reference training.py:50)."""
    trainer = FullBatchTrainer(model, trainloader, validloader, setup, cfg)
    stats, optimizer, scheduler, eng = trainer.stats, trainer.optimizer, trainer.scheduler, trainer.engine

    class Counter:
        step: int = 0

    if cfg.impl.checkpoint.name is not None:
        file = os.path.join(cfg.original_cwd, "checkpoints", cfg.impl.checkpoint.name)
        _load_from_checkpoint(model, optimizer, scheduler, None, Counter, cfg.hyp.steps, device="cpu", file=file, engine=eng)

    if cfg.hyp.evaluate_ema:                     # the reference's deepcopy of the (possibly just loaded) model, training.py:72-73
        eng.ema_init()
    while Counter.step < cfg.hyp.steps:
        trainer.step()
        Counter.step += 1
        if cfg.hyp.evaluate_ema:                 # training.py:289-294: update after every step, evaluate the EMA model
            eng.ema_update(cfg.hyp.eval_ema_momentum)
        if (Counter.step - 1) % cfg.impl.validate_every_nth_step == 0 or Counter.step >= cfg.hyp.steps or cfg.dryrun:
            trainer.evaluate()
        if trainer.rank == 0:
            log.info(status_message(optimizer, stats, Counter.step))
        if not torch.as_tensor(stats["train_loss"][-1]).isfinite():
            log.info("Terminating iterations due to divergence of loss...")
            break
        if cfg.hyp.stop_at_full_training_accuracy > 0:
            if min(stats["train_acc"][-cfg.hyp.stop_at_full_training_accuracy:]) == 1:
                log.info("Terminating training after fitting all datapoints.")
                trainer.evaluate()
                break
        if cfg.impl.checkpoint.name is not None:
            if (Counter.step - 1) % cfg.impl.checkpoint.save_every_nth_step == 0 or Counter.step >= cfg.hyp.steps:
                trainer.gather_state()           # every rank: the saved momentum buffers must be whole (sharded update)
                if trainer.rank == 0:
                    file = os.path.join(cfg.original_cwd, "checkpoints", cfg.impl.checkpoint.name)
                    os.makedirs(os.path.dirname(file), exist_ok=True)
                    _save_to_checkpoint(model, optimizer, scheduler, None, Counter, file=file, engine=eng)
        if cfg.dryrun:
            break
    trainer.gather_state()
    eng.store_to_model(model, with_grad=not trainer.stochastic)    # closure contract: p.grad holds the last (clipped) full gradient
    if trainer.stochastic:                       # ... while the stochastic branch ends every update with optimizer.zero_grad() (training.py:282)
        import inspect
        to_none = inspect.signature(torch.optim.Optimizer.zero_grad).parameters["set_to_none"].default
        for p in model.parameters():
            p.grad = None if to_none else torch.zeros_like(p)
    _sync_optimizer_state(eng, model, optimizer)
    return stats
