"""The stochastic branch of the reference's ``train()`` (``hyp.train_stochastic=True``, reference training.py:241-286) restated in plain
torch on top of ``oracle.fb_oracle`` as it stands: ``chunk_gradient``, ``gradreg``, ``sgd_step``, ``LRSchedule``, ``evaluate``.  Pinned to the
reference's own float64 runs by tests/test_cpu_sgd.py (tests/golden/scenarios_sgd.npz); the yardstick of the GPU tests of the mode.

Per "step" (= one epoch): every block of the loader is ONE BatchNorm batch and one ``optimizer.step(closure)``; the closure records |g|^2 of
the raw block gradient, applies the regulariser with ``pre_grads=None`` and the epoch's lr, then ``torch.nn.utils.clip_grad_norm_`` (always
L2; ``coef = min(1, clip / (norm + 1e-6))`` -- NOT the ``if norm > clip`` form of ``_modify_gradient_params``, which the branch does not
call: no norm bias, no gradient noise, no ``preclip_gradnorm`` / ``clipped_step``).  ``_record_stats`` runs once, after the last update.

The oracle's own network (``orc.forward`` / ``orc.backward``) knows the 'C' shortcut only; the reference's ResNet-20 has the strided 1x1
shortcut ('B').  ``Net`` hides the difference: for 'C' it is ``orc.chunk_gradient`` / ``orc.evaluate`` themselves, for 'B' the same two
quantities from autograd through the parameter container's own plain-torch ``forward`` (the yardstick of tests/test_gpu_downsample_b.py),
with the oracle's loss function; ``orc.gradreg`` takes either through its ``chunk_gradient`` argument.
"""
import copy
from collections import defaultdict

import torch
from torch.func import functional_call

from oracle import fb_oracle as orc


class Net:
    """``chunk_gradient`` and ``evaluate`` with the oracle's signatures for a parameter container ``model`` (any shortcut form)."""

    def __init__(self, cfg_model, model):
        self.native = cfg_model.downsample == "C"
        self.spec = orc.Spec(cfg_model.depth, stem=cfg_model.stem) if self.native else _LossSpec()
        self.model = None if self.native else copy.deepcopy(model)

    def _module(self, like):
        if self.model.stem[0].weight.dtype != like.dtype or self.model.stem[0].weight.device != like.device:
            self.model = self.model.to(device=like.device, dtype=like.dtype)
        return self.model

    def chunk_gradient(self, spec, params, buffers, x, y, q=orc.identity, update_bn=True):
        if self.native:
            return orc.chunk_gradient(spec, params, buffers, x, y, q, update_bn)
        assert q is orc.identity and update_bn
        m = self._module(x).train()
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        logits = functional_call(m, {**leaves, **buffers}, (x,))      # (train mode: the running statistics in ``buffers`` take their update in place)
        loss, correct, _ = orc.cross_entropy_fwd_bwd(logits, y, getattr(spec, "label_smoothing", 0.0), getattr(spec, "only_incorrect", False))
        grads = torch.autograd.grad(loss, list(leaves.values()))
        return [g.detach().clone() for g in grads], loss.detach(), correct

    def evaluate(self, spec, params, buffers, X, Y, batch=128, q=orc.identity, test_time_flips=False):
        if self.native:
            return orc.evaluate(spec, params, buffers, X, Y, batch, q, test_time_flips)
        m = self._module(X).eval()
        step_loss, step_preds, datapoints = 0.0, 0.0, 0
        with torch.no_grad():
            for i in range(0, X.shape[0], batch):
                xb, yb = X[i:i + batch], Y[i:i + batch]
                logits = functional_call(m, {**params, **buffers}, (xb,))
                if test_time_flips:
                    logits = logits.softmax(dim=1) + functional_call(m, {**params, **buffers}, (torch.flip(xb, [3]),)).softmax(dim=1)
                loss, correct, _ = orc.cross_entropy_fwd_bwd(logits, yb)
                step_loss += float(loss) * yb.shape[0]
                step_preds += float(correct)
                datapoints += yb.shape[0]
        return step_loss / datapoints, step_preds / datapoints


class _LossSpec:
    """What the loss function reads from a spec (``train_sgd`` sets it)."""
    label_smoothing, only_incorrect = 0.0, False


def torch_clip_coef(grads, max_norm):
    """``clip_grad_norm_(parameters, max_norm, norm_type=2.0)``: the factor every gradient is multiplied with (a 0-d tensor)."""
    total = torch.norm(torch.stack([torch.norm(g, 2.0) for g in grads]), 2.0)
    return torch.clamp(max_norm / (total + 1e-6), max=1.0)


def sgd_epoch(spec, params, buffers, momentum, X, Y, hyp, lr, stats, block, q=orc.identity, chunk_gradient=orc.chunk_gradient):
    """One pass over ``X`` / ``Y`` (already in loader order) in blocks of ``block`` images, ``drop_last``; mutates ``params`` / ``buffers`` /
    ``momentum`` and appends the reference's statistics to ``stats``."""
    n_blocks = X.shape[0] // block
    first = next(iter(params.values()))
    grad_norms = torch.zeros(n_blocks, dtype=first.dtype, device=first.device)
    step_loss, step_preds, datapoints = 0.0, 0.0, 0
    for b in range(n_blocks):
        xb, yb = X[b * block:(b + 1) * block], Y[b * block:(b + 1) * block]
        datapoints += block
        grads, loss, correct = chunk_gradient(spec, params, buffers, xb, yb, q)                          # training.py:263
        grad_norms[b] = orc.sqnorm(grads)                                                                 # :264
        grads = orc.gradreg(spec, params, buffers, grads, xb, yb, lr, hyp["block_strength"], hyp["eps"], hyp["implementation"], q,
                            chunk_gradient=chunk_gradient)                                                # :265
        if hyp.get("grad_clip") is not None:                                                              # :274-275
            coef = torch_clip_coef(grads, hyp["grad_clip"])
            for g in grads:
                g.mul_(coef)
        step_loss = step_loss + loss                                                                      # :277
        step_preds = step_preds + correct
        orc.sgd_step(params, grads, momentum, lr, hyp)                                                    # :281
    # _record_stats(stats, None, step_loss, ...), training.py:85-119, with the parameters after the last update
    for idx, entry in enumerate(grad_norms.sqrt().tolist()):
        stats[f"grad_norm_train_{idx}"].append(entry)
    param_norm = sum(p.pow(2).sum() for p in params.values())
    full_grad_norm = grad_norms.mean()
    full_loss = step_loss / n_blocks + 0.5 * hyp["weight_decay"] * param_norm
    if hyp["block_strength"] != 0:
        full_loss = full_loss + lr / 4 * hyp["block_strength"] * full_grad_norm
    stats["train_loss"].append(float(step_loss) / n_blocks)
    stats["train_acc"].append(float(step_preds) / datapoints)
    stats["param_norm"].append(float(param_norm))
    stats["grad_norm"].append(float(full_grad_norm.sqrt()))
    stats["full_loss"].append(float(full_loss))


def train_sgd(net, state, X, Y, hyp, steps, block, scheduler="cosine-decay", warmup=0, q=orc.identity, Xv=None, Yv=None, validate_every=100,
              order_fn=None, before_eval=None, momentum=None, first_step=0):
    """The driver of ``oracle.fb_oracle.train`` around ``sgd_epoch``: schedule, EMA, validation; mutates ``state``; returns the stats
    (``stats["_momentum"]``: the momentum buffers).  ``net``: a ``Net``.  ``momentum`` / ``first_step``: continue a run (buffers, epochs
    already taken)."""
    spec = net.spec
    params, buffers = orc.split_state(state)
    momentum = [None] * len(params) if momentum is None else momentum
    spec.label_smoothing = float(hyp.get("label_smoothing") or 0.0)
    spec.only_incorrect = hyp.get("loss_modification") == "incorrect-xent"
    sched = orc.LRSchedule(hyp["lr"], scheduler, steps, warmup)
    for _ in range(first_step):
        sched.step()
    stats = defaultdict(list)
    ema = hyp.get("evaluate_ema", False)
    if ema:
        ema_params = {k: v.clone() for k, v in params.items()}
        ema_buffers = {k: v.clone() for k, v in buffers.items()}
    for step in range(first_step, steps):
        Xs, Ys = X, Y
        if order_fn is not None:
            idx = order_fn(step)
            Xs, Ys = X[idx], Y[idx]
        sgd_epoch(spec, params, buffers, momentum, Xs, Ys, hyp, sched.lr, stats, block, q, chunk_gradient=net.chunk_gradient)
        stats["lr"].append(sched.lr)
        sched.step()
        eval_params, eval_buffers = params, buffers
        if ema:
            m = hyp["eval_ema_momentum"]
            for src, dst in ((params, ema_params), (buffers, ema_buffers)):
                for k in src:
                    dst[k].copy_(m * dst[k] + (1 - m) * src[k])
            eval_params, eval_buffers = ema_params, ema_buffers
        if Xv is not None and (step % validate_every == 0 or step + 1 >= steps):
            if before_eval is not None:
                before_eval()
            vl, va = net.evaluate(spec, eval_params, eval_buffers, Xv, Yv, q=q, test_time_flips=hyp.get("test_time_flips", False))
            stats["valid_loss"].append(vl)
            stats["valid_acc"].append(va)
    stats["_momentum"] = momentum
    return stats
