"""Flat-buffer train-step tail: clip_grad_norm_ + Adam or SGD in two HIP launches (scripts/train.py:265-267).

The reference step is ``clip_grad_norm_(net.parameters(), cfg.clip_grad_norm)`` then
``optimizer.step()`` (train_tools/train.py via scripts/train.py:262-268), the optimizer being
``torch.optim.SGD`` or ``torch.optim.Adam`` by ``cfg.optimizer`` (scripts/train.py:219-224).  With 400+
parameter tensors that is ~20 multi-tensor launches plus per-tensor host work per step.
``FusedAdam`` and ``FusedSGD`` keep parameters, gradients and the optimizer state as single flat fp32
buffers (parameters are re-pointed into the flat storage once, ``param.grad`` are views into the
gradient buffer shared with ``factmx.dp.FlatGradReducer``) and run the whole tail as
``fx_adam_step_checked`` / ``fx_sgd_step``: deterministic g^2 partial sums, then one fused clip +
update.  Semantics are torch.optim.Adam's (amsgrad off, L2 weight decay), torch.optim.SGD's (dampening 0,
nesterov off) and clip_grad_norm_'s (2-norm, coefficient min(max_norm / (norm + 1e-6), 1), clipped
gradient left in ``.grad``).  Both carry ``param_groups`` (one group), read at every step, so the
reference's learning-rate decay loop (scripts/train.py:321-323) runs against them as written;
``build_optimizer(cfg, params)`` is the reference's choice between the two.
"""
import torch

from . import native as nx


def flatten_parameters(params):
    """Re-point every parameter's storage into one contiguous fp32 buffer (same values, same
    Parameter objects, so modules, state_dict and the kernels see no difference)."""
    params = [p for p in params if p.requires_grad]
    dev = params[0].device
    total = sum(p.numel() for p in params)
    flat = torch.empty(total, device=dev, dtype=torch.float32)
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.reshape(-1))
            p.data = flat[off:off + n].view_as(p)
            off += n
    return flat, params


def _hyper(name):
    """A hyper-parameter attribute that lives in ``param_groups[0]``: the attribute and the dict entry
    are one value."""
    return property(lambda self: self.param_groups[0][name],
                    lambda self, value: self.param_groups[0].__setitem__(name, value))


class _FlatOptimizer:
    """What FusedAdam and FusedSGD share: flat parameters, ``.grad`` views into ``grad_flat`` (the flat
    gradient buffer whose views are the parameters' ``.grad`` in the same order, FlatGradReducer.flat;
    without it one is created here), the grad-norm workspace, ``total_norm``, ``step_count`` and one
    ``param_groups`` dict holding the hyper-parameters that ``step()`` reads."""

    lr = _hyper("lr")
    weight_decay = _hyper("weight_decay")
    max_grad_norm = _hyper("max_grad_norm")

    def __init__(self, params, grad_flat, **hyper):
        self.flat, self.params = flatten_parameters(params)
        n = self.flat.numel()
        if grad_flat is None:
            grad_flat = torch.zeros(n, device=self.flat.device)
            off = 0
            for p in self.params:
                p.grad = grad_flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        assert grad_flat.numel() == n and grad_flat.is_contiguous()
        off = 0
        for p in self.params:
            g = p.grad
            if g is None or g.data_ptr() != grad_flat.data_ptr() + 4 * off:
                raise ValueError(f"{type(self).__name__}: parameter .grad must be views into grad_flat in "
                                 "parameter order")
            off += p.numel()
        self.grad_flat = grad_flat
        self.param_groups = [dict(params=self.params, **hyper)]
        self.step_count = 0
        lib = nx.load()
        self._ws = torch.empty(lib.fx_grad_norm_workspace_floats(), device=self.flat.device)
        self.total_norm = torch.zeros(1, device=self.flat.device)

    def _max_norm(self):
        return float(self.max_grad_norm) if self.max_grad_norm else 0.0

    def _status(self):
        # the device status word: a step whose kernels failed (BiGRU timeout in the backward) leaves the
        # parameters and the optimizer state untouched; the failure is raised by the next status read-back
        from .functional import device_status
        return device_status(self.flat.device)

    def zero_grad(self, set_to_none=False):
        self.grad_flat.zero_()


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) with an optional fused
    clip_grad_norm_(max_grad_norm), over flat buffers.  ``grad_flat`` is the flat gradient
    buffer whose views are the parameters' ``.grad`` in the same order (FlatGradReducer.flat);
    without it one is created here."""

    betas = _hyper("betas")
    eps = _hyper("eps")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 grad_flat=None):
        super().__init__(params, grad_flat, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                         max_grad_norm=max_grad_norm)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)

    @torch.no_grad()
    def step(self):
        lib = nx.load()
        self.step_count += 1
        b1, b2 = self.betas
        nx.check(lib.fx_adam_step_checked(nx.ptr(self.flat), nx.ptr(self.grad_flat), nx.ptr(self.exp_avg),
                                          nx.ptr(self.exp_avg_sq), self.flat.numel(), self.step_count,
                                          float(self.lr), float(b1), float(b2), float(self.eps),
                                          float(self.weight_decay), self._max_norm(), nx.ptr(self._ws),
                                          nx.ptr(self.total_norm), nx.ptr(self._status()), nx.stream()),
                 "fx_adam_step_checked")

    def state_dict(self):
        return {"step": self.step_count, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) (dampening 0, nesterov off) with an optional
    fused clip_grad_norm_(max_grad_norm), over flat buffers; ``grad_flat`` as in FusedAdam.
    ``momentum_buffer`` is one flat zeroed buffer, which gives torch's first step (buf = d); it exists
    only once a step has to run with momentum != 0 (None otherwise: momentum-free SGD reads, writes and
    allocates no state)."""

    momentum = _hyper("momentum")

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, max_grad_norm=None, grad_flat=None):
        super().__init__(params, grad_flat, lr=lr, momentum=momentum, weight_decay=weight_decay,
                         max_grad_norm=max_grad_norm)
        self.momentum_buffer = torch.zeros_like(self.flat) if momentum else None

    @torch.no_grad()
    def step(self):
        lib = nx.load()
        self.step_count += 1
        momentum = float(self.momentum)
        if momentum and self.momentum_buffer is None:   # raised from 0 through param_groups
            self.momentum_buffer = torch.zeros_like(self.flat)
        buf = self.momentum_buffer if momentum else None
        nx.check(lib.fx_sgd_step(nx.ptr(self.flat), nx.ptr(self.grad_flat), nx.ptr(buf), self.flat.numel(),
                                 float(self.lr), momentum, float(self.weight_decay), self._max_norm(),
                                 nx.ptr(self._ws), nx.ptr(self.total_norm), nx.ptr(self._status()), nx.stream()),
                 "fx_sgd_step")

    def state_dict(self):
        buf = self.momentum_buffer
        return {"step": self.step_count, "momentum_buffer": None if buf is None else buf.clone(),
                "lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        buf = sd["momentum_buffer"]
        if buf is None:
            self.momentum_buffer = None
        else:
            if self.momentum_buffer is None:
                self.momentum_buffer = torch.empty_like(self.flat)
            self.momentum_buffer.copy_(buf)


def build_optimizer(cfg, params, grad_flat=None):
    """The optimizer ``cfg`` names, as scripts/train.py:219-224 builds it, with the clipping of :266-267
    fused in: ``cfg.optimizer`` "SGD" -> FusedSGD(cfg.lr, cfg.momentum, cfg.weight_decay), "Adam" ->
    FusedAdam(cfg.lr, weight_decay=cfg.weight_decay); max_grad_norm = cfg.clip_grad_norm when > 0."""
    max_norm = cfg.clip_grad_norm if cfg.clip_grad_norm > 0 else None
    if cfg.optimizer == "SGD":
        return FusedSGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay,
                        max_grad_norm=max_norm, grad_flat=grad_flat)
    if cfg.optimizer == "Adam":
        return FusedAdam(params, lr=cfg.lr, weight_decay=cfg.weight_decay, max_grad_norm=max_norm,
                         grad_flat=grad_flat)
    raise ValueError(f"build_optimizer: unknown cfg.optimizer {cfg.optimizer!r} (expected 'SGD' or 'Adam')")


def clip_grad_norm_flat_(grad_flat, max_norm):
    """clip_grad_norm_ over one flat gradient buffer (two launches, no host sync); returns the
    total norm as a 1-element device tensor."""
    lib = nx.load()
    ws = torch.empty(lib.fx_grad_norm_workspace_floats(), device=grad_flat.device)
    norm = torch.empty(1, device=grad_flat.device)
    nx.check(lib.fx_grad_norm(nx.ptr(grad_flat), grad_flat.numel(), nx.ptr(ws), nx.ptr(norm), nx.stream()),
             "fx_grad_norm")
    nx.check(lib.fx_clip_grad_scale(nx.ptr(grad_flat), grad_flat.numel(), nx.ptr(ws), float(max_norm), nx.stream()),
             "fx_clip_grad_scale")
    return norm
