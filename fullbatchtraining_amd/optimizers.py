"""What ``hyp.optim`` can select (reference fullbatch/training/optimizers.py:10-93): ``TABLE`` holds one descriptor per optimizer -- what its
fused update does not cover (``check``), the torch object that carries its state in the reference's checkpoint layout (``container``), the engine
call of an update (``update``), the state's way between engine and container (``sync`` / ``load``) -- and ``training.py`` asks ``select(cfg_hyp)``."""
import math
import re
from collections import defaultdict

import numpy as np
import torch
from torch.optim.lr_scheduler import _LRScheduler


# ---- LR schedule objects (state containers; reference optimizers.py:69-93, additional_optimizers/scheduler.py:32-111) ----------------
class GradualWarmupScheduler(_LRScheduler):
    """Linear warm-up from 0 (multiplier 1.0) to the base lr over ``total_epoch`` steps, then hands over to
    ``after_scheduler``.  Attribute names and ``state_dict`` layout follow the reference so checkpoints interchange."""

    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError("multiplier should be greater thant or equal to 1.")
        self.multiplier, self.total_epoch, self.after_scheduler, self.finished = multiplier, total_epoch, after_scheduler, False
        super().__init__(optimizer)

    def get_lr(self):
        if self.last_epoch > self.total_epoch:
            if self.after_scheduler:
                if not self.finished:
                    self.after_scheduler.base_lrs = [b * self.multiplier for b in self.base_lrs]
                    self.finished = True
                return self.after_scheduler.get_last_lr()
            return [b * self.multiplier for b in self.base_lrs]
        if self.multiplier == 1.0:
            return [b * (float(self.last_epoch) / self.total_epoch) for b in self.base_lrs]
        return [b * ((self.multiplier - 1.0) * self.last_epoch / self.total_epoch + 1.0) for b in self.base_lrs]

    def step(self, epoch=None):
        if self.finished and self.after_scheduler:
            self.after_scheduler.step(None if epoch is None else epoch - self.total_epoch)
            self._last_lr = self.after_scheduler.get_last_lr()
        else:
            return super().step(epoch)

    def state_dict(self):
        state = {k: v for k, v in self.__dict__.items() if k != "optimizer"}
        state["after_scheduler"] = {k: v for k, v in self.after_scheduler.__dict__.items() if k != "optimizer"}
        return state

    def load_state_dict(self, state_dict):
        after = state_dict.pop("after_scheduler")
        self.after_scheduler.__dict__.update(after)
        self.__dict__.update(state_dict)


def _scheduler_for(optimizer, cfg_hyp):
    """The lr schedule of reference optimizers.py:69-91 around the (unwrapped) optimizer."""
    sched = cfg_hyp.scheduler
    if sched == "cosine-decay-floored":
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, cfg_hyp.steps, eta_min=cfg_hyp.optim.lr / 25)
    elif sched == "cosine-decay":
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, cfg_hyp.steps, eta_min=0.0)
    elif sched == "cosine-4000":
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, 4000, eta_min=0.0)
    elif sched == "linear":
        scheduler = torch.optim.lr_scheduler.MultiStepLR(
            optimizer, milestones=[cfg_hyp.steps // 2.667, cfg_hyp.steps // 1.6, cfg_hyp.steps // 1.142], gamma=0.1)
    elif sched == "exponential":
        scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.99)
    elif sched in ["", " ", None]:
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[], gamma=1)
    else:
        raise ValueError(f"Invalid scheduler {sched} provided.")
    if cfg_hyp.warmup > 0:
        scheduler = GradualWarmupScheduler(optimizer, multiplier=1.0, total_epoch=cfg_hyp.warmup, after_scheduler=scheduler)
    # The torch optimizer is a STATE CONTAINER here (param_groups / state in the checkpoint layout): the update itself is the engine call of
    # its descriptor's ``update`` (TABLE below), so ``optimizer.step()`` is never called -- tell the schedulers that updates do happen, or the
    # first ``scheduler.step()`` warns "lr_scheduler.step() before optimizer.step()" on every run
    optimizer._opt_called = True
    return scheduler


# ---- state containers: they hold no arithmetic, every update runs in the engine ----------------------------------------
FISTA_KEYS = ("name", "lr", "fista_mod", "projection")


def _fista_mod(fista_mod):
    """``fista_mod`` as a tuple of three floats; ValueError for anything but three finite numbers."""
    try:
        mod = tuple(float(v) for v in fista_mod)
    except (TypeError, ValueError):
        mod = ()
    if len(mod) != 3 or not all(math.isfinite(v) for v in mod) or any(isinstance(v, (bool, str)) for v in fista_mod):
        raise ValueError(f"hyp.optim.fista_mod must be three finite numbers (p, q, r), got {fista_mod!r}")
    return mod


class FISTA(torch.optim.Optimizer):
    """State container with the layout of the reference's ``FISTA`` (additional_optimizers/fista.py): one param group with ``lr``,
    ``fista_mod``, ``projection``; ``state[p] = {"x+", "x-", "tk"}``.  It holds no arithmetic: the update is the engine's fb_mt_fista on the
    arena."""

    def __init__(self, params, projection=None, lr=1e-4, fista_mod=(1.0, 1.0, 4.0)):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        super().__init__(params, dict(lr=lr, fista_mod=fista_mod, projection=projection))

    def step(self, closure=None):
        raise RuntimeError("FISTA is a state container: the update runs in the engine (Engine.fista_step)")


WOLFE_DEFAULTS = dict(c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10)      # WolfeGradientDescent.__init__ (the reference's gd.yaml carries none of them)


def wolfe_constants(cfg_optim):
    """(c1, c2, alpha_max, max_iter) of a ``Gradient Descent`` group: the group's own values where it has them (``+hyp.optim.c1=...``), the
    reference constructor's defaults otherwise."""
    return tuple(cfg_optim.get(k, v) for k, v in WOLFE_DEFAULTS.items())


class WolfeGradientDescent(torch.optim.Optimizer):
    """State container with the layout of the reference's ``WolfeGradientDescent`` (additional_optimizers/sgd_linesearch.py:183-203): one param
    group with the SGD keys and ``c1``, ``c2``, ``alpha_max``, ``max_iter``; ``state[p]["momentum_buffer"]`` and the bare key ``state["alpha"]``
    (the step length the last search returned).  It holds no arithmetic: direction, trial points and phi' are the engine's fb_mt_wolfe_* on the
    arena, the search is ``WolfeSearch``."""

    def __init__(self, params, lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False, c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, c1=c1, c2=c2,
                                      alpha_max=alpha_max, max_iter=max_iter))

    def step(self, closure=None):
        raise RuntimeError("WolfeGradientDescent is a state container: the step runs in FullBatchTrainer.step (WolfeSearch on the engine)")


class WolfeSearch:
    """The control flow of ``WolfeGradientDescent.step`` / ``_zoom`` / ``_interpolate`` (sgd_linesearch.py:303-381) on Python floats: the
    reference's expressions in the reference's order, its look-up table (a ``defaultdict(dict)`` keyed by alpha, so an alpha that was seen is not
    evaluated again), its exits -- and its quirks: ``prev_loss`` is never updated, a zoom that runs out of rounds returns an alpha it never
    evaluated, ``math.sqrt`` of a negative discriminant raises ValueError.  It sees the problem only through ``evaluate(alpha) -> (loss,
    phi_grad)``: the parameters are left wherever the last evaluation put them.

    After ``search``: ``evaluated`` (every alpha handed to ``evaluate``, in order), ``trace`` (every inequality decided, as
    ``(name, alpha, left, right)``), ``exit`` (which way the outer loop ended), ``zoom_exit`` (which way the zoom ended, if there was one) and
    ``table_hits`` (how often the table spared an evaluation)."""

    def __init__(self, c1=1e-4, c2=0.9, alpha_max=10.0, max_iter=10):
        self.c1, self.c2, self.alpha_max, self.max_iter = c1, c2, alpha_max, max_iter
        self.evaluated, self.trace, self.exit, self.zoom_exit, self.table_hits = [], [], None, None, 0

    def _evaluate_phi(self, alpha, evaluate, phi):
        if alpha not in phi:
            loss, phi_grad = evaluate(alpha)
            self.evaluated.append(alpha)
            phi[alpha] = dict(val=loss, grad=phi_grad)
        else:
            self.table_hits += 1

    def search(self, loss0, phi_grad0, evaluate):
        """``loss0 = phi(0)``, ``phi_grad0 = phi'(0)`` -> the alpha the reference stores in ``state['alpha']``."""
        self.evaluated, self.trace, self.exit, self.zoom_exit, self.table_hits = [], [], "max_iter", None, 0
        alpha = 1.0
        phi = defaultdict(dict)
        phi[0] = dict(val=loss0, grad=phi_grad0)
        prev_loss = float("inf")
        prev_alpha = 0
        for iteration in range(self.max_iter):
            self._evaluate_phi(alpha, evaluate, phi)
            sufficient_loss = phi[0]["val"] + self.c1 * alpha * phi[0]["grad"]
            self.trace.append(("decrease", alpha, phi[alpha]["val"], sufficient_loss))
            if (phi[alpha]["val"] > sufficient_loss) or (phi[alpha]["val"] > prev_loss):
                alpha = self._zoom(prev_alpha, alpha, evaluate, phi)
                self.exit = "zoom-1"
                break
            self.trace.append(("curvature", alpha, abs(phi[alpha]["grad"]), -self.c2 * phi[0]["grad"]))
            if abs(phi[alpha]["grad"]) <= -self.c2 * phi[0]["grad"]:
                self.exit = "accepted"
                break
            self.trace.append(("sign", alpha, phi[alpha]["grad"], 0.0))
            if phi[alpha]["grad"] >= 0:
                alpha = self._zoom(alpha, prev_alpha, evaluate, phi)
                self.exit = "zoom-2"
                break
            prev_alpha = alpha
            alpha = min(alpha * 2.5, self.alpha_max)
            if alpha == self.alpha_max:
                self.exit = "alpha_max"
                break
        return alpha

    def _zoom(self, alpha_low, alpha_high, evaluate, phi):
        for iteration in range(self.max_iter):
            if abs(alpha_low - alpha_high) < 1e-4:
                self.zoom_exit = "interval"
                return alpha_low
            alpha = self._interpolate(alpha_low, alpha_high, phi)
            self._evaluate_phi(alpha, evaluate, phi)
            sufficient_loss = phi[0]["val"] + self.c1 * alpha * phi[0]["grad"]
            self.trace.append(("zoom-decrease", alpha, phi[alpha]["val"], sufficient_loss))
            self.trace.append(("zoom-low", alpha, phi[alpha]["val"], phi[alpha_low]["val"]))
            if (phi[alpha]["val"] > sufficient_loss) or (phi[alpha]["val"] > phi[alpha_low]["val"]):
                alpha_high = alpha
            else:
                self.trace.append(("zoom-curvature", alpha, phi[alpha]["grad"], -self.c2 * phi[0]["grad"]))
                if (phi[alpha]["grad"]) <= -self.c2 * phi[0]["grad"]:
                    self.zoom_exit = "curvature"
                    return alpha
                self.trace.append(("zoom-sign", alpha, phi[alpha]["grad"] * (alpha_high - alpha_low), 0.0))
                if phi[alpha]["grad"] * (alpha_high - alpha_low) >= 0:
                    alpha_high = alpha_low
                alpha_low = alpha
        self.zoom_exit = "exhausted"
        return self._interpolate(alpha_low, alpha_high, phi)

    @staticmethod
    def _interpolate(alpha1, alpha2, phi):
        """Cubic interpolation as in Nocedal and Wright."""
        if alpha1 == alpha2:
            return alpha1
        quotient = (phi[alpha1]["val"] - phi[alpha2]["val"]) / (alpha1 - alpha2)
        d_1 = phi[alpha1]["grad"] + phi[alpha2]["grad"] - 3 * quotient
        d_2 = math.copysign(1.0, alpha2 - alpha1) * math.sqrt(d_1**2 - phi[alpha1]["grad"] * phi[alpha2]["grad"])
        update_nom = phi[alpha2]["grad"] + d_2 - d_1
        update_denom = phi[alpha2]["grad"] - phi[alpha1]["grad"] + 2 * d_2
        return alpha2 - (alpha2 - alpha1) * update_nom / update_denom


class SGD_AGC(torch.optim.Optimizer):
    """State container with the layout of the reference's ``SGD_AGC`` (additional_optimizers/sgd_agc.py): one param group per named tensor
    carrying ``name``, ``clipping``, ``eps`` and the SGD keys; ``state[p]["momentum_buffer"]``.  It holds no arithmetic: the update is the
    engine's fb_mt_agc_sgd on the arena."""

    def __init__(self, named_params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, clipping=None, eps=1e-3):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"Invalid lr / momentum / weight_decay: {lr} / {momentum} / {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, clipping=clipping, eps=eps)
        super().__init__([{"params": param, "name": name} for name, param in named_params], defaults)

    def step(self, closure=None):
        raise RuntimeError("SGD_AGC is a state container: the update runs in the engine (Engine.agc_sgd_step)")


class _OptimizerWrapper:
    """State container with the reference wrappers' surface (``.optim``, shared ``param_groups``, attribute pass-through, pickling
    via the wrapped optimizer; reference additional_optimizers/sam.py:34-54, lars.py:41-59).  The arithmetic runs in the engine."""

    def __init__(self, optimizer):
        self.optim = optimizer

    @property
    def param_groups(self):
        """Always the wrapped optimizer's CURRENT list: ``Optimizer.load_state_dict`` replaces it, and the scheduler (which drives the
        wrapped SGD) writes the lr there -- a reference held from construction would freeze the lr of a resumed SAM / LARS run."""
        return self.optim.param_groups

    @param_groups.setter
    def param_groups(self, value):
        self.optim.param_groups = value

    def __getstate__(self):
        return self.optim.__getstate__()

    def __setstate__(self, state):
        self.optim.__setstate__(state)

    def __repr__(self):
        return self.optim.__repr__()

    def __getattr__(self, name):
        if name == "optim":
            raise AttributeError(name)
        return getattr(self.optim, name)


class SAM(_OptimizerWrapper):
    """Sharpness-aware minimisation (reference additional_optimizers/sam.py): the step evaluates the full-batch closure twice --
    ``FullBatchTrainer.step`` runs closure -> ``Engine.sam_ascent`` -> closure -> ``Engine.sam_restore`` -> SGD update."""

    def __init__(self, optimizer, rho=0.05):
        assert rho >= 0.0, f"Invalid rho, should be non-negative: {rho}"
        super().__init__(optimizer)
        self.rho = rho


class LARS(_OptimizerWrapper):
    """LARS / LARC wrapper (reference additional_optimizers/lars.py).  Around a closure the reference's wrapper has exactly one
    effect: it rescales ``p.grad`` of the PREVIOUS step, zeroes the group weight decay and then calls ``SGD.step(closure)``, whose
    closure assigns fresh gradients (training.py:183-184) -- the update is plain SGD without weight decay, independent of
    ``trust_coefficient`` / ``clip`` / ``eps`` (pinned against the reference in tests/golden/scenarios_n4.npz)."""

    def __init__(self, optimizer, trust_coefficient=0.02, clip=False, eps=1e-8):
        super().__init__(optimizer)
        self.trust_coefficient, self.clip, self.eps = trust_coefficient, clip, eps


def _arguments(cfg_hyp):
    return {k: v for k, v in cfg_hyp.optim.items() if k not in ("name", "line_search")}


class GradientDescent:
    """``Gradient Descent`` / ``line_search: none`` -> torch.optim.SGD (reference optimizers.py:14-37, 55-67), and the shape of every row.
    ``label`` names the optimizer in the refusals (None: none; SAM / LARS, per-tensor weight decay and the sharded update are built around SGD),
    ``reasons`` says why not for the three shared ones, ``before`` / ``after`` are its own around them.  ``search``: the step is
    ``FullBatchTrainer._wolfe_step``, not an ``update``.  ``kind`` / ``launch``: see ``container`` / ``update``."""
    label = reasons = kind = launch = search = None
    before = after = staticmethod(lambda cfg_hyp: None)

    def check(self, cfg_hyp, multi=False):
        """NotImplementedError for what the update does not cover.  ``multi``: on the multi-process code path (``FB_FORCE_DIST=1``: with one rank)."""
        if self.label is None:
            return
        mod, (why_mod, why_decay, why_sharded) = cfg_hyp.optim_modification.name, self.reasons
        self.before(cfg_hyp)
        if mod != "none":
            raise NotImplementedError(f"{self.label} with optim_modification {mod!r} ({why_mod})")
        if cfg_hyp.only_linear_layers_weight_decay:
            raise NotImplementedError(f"{self.label} with only_linear_layers_weight_decay ({why_decay})")
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError(f"{self.label} on more than one rank ({why_sharded})")
        self.after(cfg_hyp)
        if multi:
            raise NotImplementedError(f"{self.label} on the multi-process code path ({why_sharded})")

    def container(self, model, cfg_hyp):
        """The torch object that carries the state in the reference's checkpoint layout (SAM / LARS: the wrapper around it)."""
        if self.kind is not None:                # ``kind``: a plain constructor over the group's keys
            return self.kind(model.parameters(), **_arguments(cfg_hyp))
        mod = cfg_hyp.optim_modification.name
        if cfg_hyp.only_linear_layers_weight_decay:      # reference optimizers.py:14-21: one param group per tensor, no decay on biases / gains
            parameter_iterable = []
            for key, value in model.named_parameters():
                if len(re.findall("(bias|gain)|skip_gain", key)) > 0:
                    parameter_iterable += [{"params": [value], "weight_decay": 0.0}]
                else:
                    parameter_iterable += [{"params": [value]}]
        else:
            parameter_iterable = model.parameters()
        optimizer = torch.optim.SGD(parameter_iterable, **_arguments(cfg_hyp))
        if mod == "SAM":
            return SAM(optimizer, rho=cfg_hyp.optim_modification.rho)
        if mod in ("LARS", "LARC"):
            return LARS(optimizer, trust_coefficient=cfg_hyp.optim_modification.trust_coefficient, clip=mod == "LARC",
                        eps=cfg_hyp.optim_modification.eps)
        return optimizer

    def update(self, engine, hyp, lr, grad_clip, *, torch_clip=False, zero_wd=False, optimizer=None, fused=False):
        """The ONE engine call of an update, after the clip by the global norm in ``engine.norms2[0]``: the full-batch closure's form (the clipped
        gradient is written back) or, with ``torch_clip``, ``clip_grad_norm_``'s (the mini-batch branch; ``fused``: with the weight copies)."""
        o = hyp.optim
        if self.launch is not None:              # ``launch``: one Engine method that takes these keys of the group, in this order
            getattr(engine, self.launch[0])(lr, *(o[k] for k in self.launch[1:]), grad_clip, torch_clip=torch_clip)
        elif torch_clip:
            engine.sgd_prep_step(lr, o.weight_decay, o.momentum, o.dampening, o.nesterov, grad_clip, fused=fused)
        elif hyp.only_linear_layers_weight_decay and not zero_wd:    # the param groups carry the per-tensor weight decay
            engine.sgd_step_per_tensor(lr, [g["weight_decay"] for g in optimizer.param_groups], o.momentum, o.dampening, o.nesterov, grad_clip)
        else:
            engine.sgd_step(lr, 0.0 if zero_wd else o.weight_decay, o.momentum, o.dampening, o.nesterov, grad_clip)

    def sync(self, engine, model, optimizer):
        """Expose the engine's state as ``optimizer.state`` in the reference layout (here: the momentum buffers and SAM's last ascent step)."""
        if engine.first_step:
            return
        for p, buf in zip(model.parameters(), engine.momentum_state()):
            optimizer.state[p]["momentum_buffer"] = buf.to(p.device, p.dtype)
        if getattr(engine, "e_w", None) is not None:       # SAM keeps its last ascent step in the wrapped optimizer's state (sam.py:66)
            for p, e in zip(model.parameters(), engine.sam_state()):
                optimizer.state[p]["e_w"] = e.to(p.device, p.dtype)

    def load(self, engine, model, optimizer):
        """Hand a loaded ``optimizer.state`` to the engine, if it is complete."""
        bufs = [optimizer.state[p].get("momentum_buffer") for p in model.parameters() if p in optimizer.state]
        if len(bufs) == len(list(model.parameters())) and all(b is not None for b in bufs):
            engine.load_momentum(bufs)


class Wolfe(GradientDescent):
    """``line_search: wolfe`` -> ``WolfeGradientDescent`` (reference optimizers.py:29-30); the state is SGD's momentum and ``state["alpha"]``."""
    label, search, kind = "line_search=wolfe", True, WolfeGradientDescent
    reasons = ("SAM's two closures and the LARS wrapper are built around one SGD update per step, not around a search that evaluates the closure itself",
               "fb_mt_wolfe_direction and fb_mt_wolfe_phi_grad take one weight decay for the whole arena",
               "every evaluation would need the exchanged gradient whole on every rank and one agreed phi'; the sharded update has neither")

    def before(self, cfg_hyp):
        if cfg_hyp.train_stochastic:
            raise NotImplementedError("line_search=wolfe with hyp.train_stochastic (the reference calls optimizer.step() without a closure in the "
                                      "mini-batch branch, training.py:274, and dies in WolfeGradientDescent.step)")


class Adam(GradientDescent):
    """``Adam`` -> torch.optim.AdamW (reference optimizers.py:39-40): one fb_mt_adamw launch."""
    label, launch = "Adam", ("adamw_step", "weight_decay", "betas", "eps")
    reasons = ("SAM's ascent step and the LARS wrapper are built around the SGD update", "the AdamW update takes one weight decay for the whole arena",
               "the sharded update would need exp_avg / exp_avg_sq in gather_sharded_state")

    def before(self, cfg_hyp):
        if cfg_hyp.optim.get("amsgrad", False):
            raise NotImplementedError("hyp.optim.amsgrad=True (fb_mt_adamw keeps no running maximum of exp_avg_sq)")

    def container(self, model, cfg_hyp):
        params = _arguments(cfg_hyp)
        params["betas"] = tuple(params["betas"])
        return torch.optim.AdamW(model.parameters(), **params)

    def sync(self, engine, model, optimizer):
        if getattr(engine, "adam_step", 0) == 0:
            return
        exp_avg, exp_avg_sq, step = engine.adam_state()
        for p, m, v in zip(model.parameters(), exp_avg, exp_avg_sq):     # torch's own state: a float32 scalar step, buffers shaped like p
            optimizer.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m.to(p.device, p.dtype),
                                  "exp_avg_sq": v.to(p.device, p.dtype)}

    def load(self, engine, model, optimizer):
        states = [optimizer.state[p] for p in model.parameters() if p in optimizer.state]
        if len(states) == len(list(model.parameters())) and all("exp_avg" in st for st in states):
            engine.load_adam_state([st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states], int(float(states[0]["step"])))


class AGC(GradientDescent):
    """``GD-AGC`` -> ``SGD_AGC`` (reference optimizers.py:45-52): one fb_mt_agc_sgd launch (engine.avg keeps the global clip only); SGD's momentum."""
    label, launch = "GD-AGC", ("agc_sgd_step", "weight_decay", "momentum", "dampening", "nesterov", "clipping", "eps")
    reasons = ("SAM's ascent step and the LARS wrapper are built around the plain SGD update",
               "the reference selects the tensors by a second regex here; the fb_mt_agc_sgd launch takes one weight decay for the whole arena",
               "the shard boundaries of the sharded update cut through units")

    def container(self, model, cfg_hyp):         # a group per tensor, no unit clip for groups named linear*
        optimizer = SGD_AGC(model.named_parameters(), **_arguments(cfg_hyp))
        for group in optimizer.param_groups:
            if group["name"].startswith("linear"):
                group["clipping"] = None
        return optimizer


class Fista(GradientDescent):
    """``FISTA`` -> ``FISTA`` (reference optimizers.py:43-44): one fb_mt_fista launch."""
    label, kind, launch = "FISTA", FISTA, ("fista_step", "fista_mod")
    reasons = ("SAM's ascent step and the LARS wrapper are built around the SGD update",
               "FISTA has no weight decay; the fb_mt_fista launch takes one group for the whole arena",
               "the sharded update would need x_minus in gather_sharded_state")

    def before(self, cfg_hyp):               # the reference hands every key of the group to FISTA.__init__ and dies with a TypeError on a foreign one
        keys = set(cfg_hyp.optim.keys())
        if keys != set(FISTA_KEYS):
            foreign, missing = sorted(keys - set(FISTA_KEYS)), sorted(set(FISTA_KEYS) - keys)
            raise NotImplementedError(f"optimizer 'FISTA' on a group that is not FISTA's (foreign keys {foreign}, missing keys {missing}): select the "
                                      "optimizer with hyp/optim=fista")
        if cfg_hyp.optim.projection is not None:
            raise NotImplementedError(f"FISTA with projection {cfg_hyp.optim.projection!r} (the reference takes a function handle, which no preset "
                                      "can carry; fb_mt_fista applies none)")

    def after(self, cfg_hyp):
        _fista_mod(cfg_hyp.optim.fista_mod)

    def sync(self, engine, model, optimizer):
        if getattr(engine, "x_minus", None) is None:
            return
        x_minus, tk = engine.fista_state()
        for p, x in zip(model.parameters(), x_minus):   # the reference's own state: after a step x+ holds the values of x-; tk a float32 tensor [1]
            x = x.to(p.device, p.dtype)
            optimizer.state[p] = {"x+": x.clone(), "x-": x, "tk": torch.full((1,), float(tk), dtype=torch.float32, device=p.device)}

    def load(self, engine, model, optimizer):
        states = [optimizer.state[p] for p in model.parameters() if p in optimizer.state]
        if len(states) == len(list(model.parameters())) and all("x-" in st for st in states):
            engine.load_fista_state([st["x-"] for st in states], np.float32(states[0]["tk"].detach().cpu().numpy().reshape(-1)[0]))


TABLE = {("Gradient Descent", "none"): GradientDescent(), ("Gradient Descent", "wolfe"): Wolfe(), ("Adam", "none"): Adam(), ("GD-AGC", "none"): AGC(),
         ("FISTA", "none"): Fista()}


def select(cfg_hyp, refuse=True):
    """The descriptor that ``cfg_hyp.optim`` selects by (name, line_search -- "none" but for gradient descent).  What the table does not have: NotImplementedError, or None with ``refuse=False``."""
    name = cfg_hyp.optim.name
    search = cfg_hyp.optim.get("line_search", "none") if name == "Gradient Descent" else "none"
    if (name, search) in TABLE or not refuse:
        return TABLE.get((name, search))
    if search in ("non-monotone", "restarting"):
        raise NotImplementedError(f"line_search {cfg_hyp.optim.line_search!r}: of the reference's three line searches only the strong-Wolfe search "
                                  "(line_search=wolfe) runs on the engine; the non-monotone and the restarting search are its follow-ups (both "
                                  "repeat torch.optim.SGD.step from a saved state, which needs a momentum snapshot next to theta0)")
    raise NotImplementedError(f"optimizer {name!r}/{cfg_hyp.optim.get('line_search')!r}: only plain gradient "
                              "descent with Nesterov momentum (line_search none or wolfe), AdamW, GD-AGC and FISTA are fused into the engine")
