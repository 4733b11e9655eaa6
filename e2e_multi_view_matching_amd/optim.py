"""The optimiser step of the reference's training loop (``train.py:419-426``) as library calls:

* ``Adam`` - ``torch.optim.Adam`` (no weight decay, no amsgrad) whose ``step()`` is ONE ``e2emv_adam_step`` call over every
  parameter of every group (csrc/optim.hip): the finite-gradient gate (``skip_nonfinite=True`` = ``has_finite_gradients`` of
  ``helpers.py:284-288``), ``clip_grad_value_`` (``grad_clip=0.1``) and the update, without a host synchronisation.  The state
  layout is torch's (``step`` a 0-dim float32 tensor, ``exp_avg``, ``exp_avg_sq``), so checkpoints written by either optimiser
  load into the other and ``ExponentialLR`` works unchanged.
* ``has_finite_gradients`` - the reference's function as one ``e2emv_grads_finite`` call and one synchronisation.

No torch op computes anything; no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib

_NEW_KEYS = ("grad_clip", "skip_nonfinite")
_UNIFORM_KEYS = ("betas", "eps", "grad_clip", "skip_nonfinite")  # one value per e2emv_adam_step call


def _torch_defaults():
    """The defaults dict of this torch's ``torch.optim.Adam`` (the keys differ between releases)."""
    return dict(torch.optim.Adam([torch.zeros(1)]).defaults)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _check_options(g):
    """ValueError for what the device step does not implement or cannot mean; `g`: a param group or the defaults."""
    lr = g["lr"]
    if torch.is_tensor(lr):
        raise ValueError("E.Adam: a tensor-valued lr is not supported (the learning rate is a host value per group)")
    if not _is_number(lr) or not lr >= 0.0:
        raise ValueError(f"E.Adam: invalid learning rate {lr!r}")
    betas = g["betas"]
    if len(betas) != 2 or any(torch.is_tensor(b) or not _is_number(b) or not 0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"E.Adam: betas must be two numbers in [0, 1), got {betas!r}")
    if not _is_number(g["eps"]) or not g["eps"] >= 0.0:
        raise ValueError(f"E.Adam: invalid epsilon {g['eps']!r}")
    if g["weight_decay"] != 0:
        raise ValueError("E.Adam: weight_decay is not implemented (must be 0)")
    for k in ("amsgrad", "maximize", "capturable", "differentiable"):
        if g.get(k):
            raise ValueError(f"E.Adam: {k}=True is not implemented")
    clip = g["grad_clip"]
    if clip is not None and not (_is_number(clip) and math.isfinite(clip) and clip > 0):
        raise ValueError(f"E.Adam: grad_clip must be None or a finite positive number, got {clip!r}")


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps)`` on the device, plus ``grad_clip`` (``clip_grad_value_`` inside the step) and
    ``skip_nonfinite`` (a step whose gradients hold a NaN or an infinity anywhere changes nothing and is counted as skipped).
    ``betas``, ``eps`` and the two new options hold for the whole step: they must be equal in every group; ``lr`` is per group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, grad_clip=None,
                 skip_nonfinite=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        defaults = _torch_defaults()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, grad_clip=grad_clip,
                        skip_nonfinite=bool(skip_nonfinite))
        _check_options(defaults)
        self._counters = None  # device int32 [applied, skipped], made by the first step
        super().__init__(params, defaults)

    # ---------------------------------------------------------------- groups and checkpoints
    def _check_uniform(self, groups=None):
        groups = self.param_groups if groups is None else groups
        for k in _UNIFORM_KEYS:
            vals = [tuple(g[k]) if k == "betas" else g[k] for g in groups]
            if any(v != vals[0] for v in vals[1:]):
                raise ValueError(f"E.Adam: {k} must be the same in every param group (one device call per step), got {vals!r}")

    def add_param_group(self, param_group):
        if isinstance(param_group, dict):
            _check_options({**self.defaults, **{k: v for k, v in param_group.items() if k != "params"}})
        super().add_param_group(param_group)
        try:
            self._check_uniform()
        except ValueError:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_counters", None)
        self._fill_groups()

    def _fill_groups(self):
        for g in self.param_groups:  # a checkpoint of torch.optim.Adam has no grad_clip / skip_nonfinite
            for k, v in self.defaults.items():
                g.setdefault(k, v)

    def load_state_dict(self, state_dict):
        merged = [{**self.defaults, **{k: v for k, v in g.items() if k != "params"}} for g in state_dict["param_groups"]]
        for g in merged:
            _check_options(g)
        if merged:
            self._check_uniform(merged)
        super().load_state_dict(state_dict)
        self._fill_groups()
        for p, st in self.state.items():  # torch keeps `step` on the host (or as a number, before 1.12): here it lives beside the parameter
            if "step" in st:
                st["step"] = self._device_step(st["step"], p)

    @staticmethod
    def _device_step(step, p):
        if torch.is_tensor(step):
            return step.detach().to(device=p.device, dtype=torch.float32).reshape(())
        return torch.tensor(float(step), dtype=torch.float32, device=p.device)

    # ---------------------------------------------------------------- the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_uniform()
        todo = []
        for group in self.param_groups:
            _check_options(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("E.Adam does not support sparse gradients")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError(f"E.Adam: parameters must be contiguous float32 tensors, got {p.dtype} with strides {p.stride()}")
                todo.append((p, float(group["lr"])))
        if not todo:
            return loss
        devices = {p.device for p, _ in todo} | {p.grad.device for p, _ in todo}
        if len(devices) > 1:
            raise ValueError(f"E.Adam: the tensors of one step must be on one device, got {sorted(map(str, devices))}")
        dev = devices.pop()
        if dev.type != "cuda":
            raise RuntimeError("E.Adam.step needs its parameters on an MI355X (no CPU fallback)")
        grads, ms, vs, steps = [], [], [], []
        for p, _ in todo:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            s = st["step"]
            if not (torch.is_tensor(s) and s.device == dev and s.dtype == torch.float32 and s.numel() == 1):
                s = st["step"] = self._device_step(s, p)
            for k in ("exp_avg", "exp_avg_sq"):
                t = st[k]
                if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                    raise ValueError(f"E.Adam: state {k} must be a contiguous float32 tensor of the parameter's size on {dev}")
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.to(torch.float32).contiguous()
            grads.append(g)
            ms.append(st["exp_avg"])
            vs.append(st["exp_avg_sq"])
            steps.append(s)
        if self._counters is None or self._counters.device != dev:
            self._counters = torch.zeros(2, dtype=torch.int32, device=dev)
        group = self.param_groups[0]
        params = [p for p, _ in todo]
        n = len(todo)
        arr = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (params, grads, ms, vs, steps)]
        numel = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        lr = (ctypes.c_float * n)(*[v for _, v in todo])
        ctx = _lib.context(dev)
        with torch.cuda.device(dev):
            ctx.call("e2emv_adam_step", n, *arr, numel, lr, float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                     float(group["grad_clip"] or 0.0), 1 if group["skip_nonfinite"] else 0, _lib.ptr(self._counters),
                     _lib.stream_ptr(dev))
        # the kernels wrote through raw pointers: autograd's version counters (and with them the matcher's weight fingerprint,
        # which decides whether the next forward re-commits its weights) have to be told
        torch.autograd.graph.increment_version(params)
        return loss

    def counters(self):
        """(applied, skipped) steps so far as Python ints.  Synchronises - the only method here that does."""
        if self._counters is None:
            return (0, 0)
        a, s = self._counters.tolist()
        return (int(a), int(s))


def has_finite_gradients(net_or_params):
    """``helpers.has_finite_gradients``: False if any gradient of the module's (or the iterable's) parameters holds a NaN or an
    infinity.  One device call over all gradients and one synchronisation (the reference: one per parameter tensor)."""
    params = net_or_params.parameters() if isinstance(net_or_params, torch.nn.Module) else net_or_params
    if torch.is_tensor(params):
        params = [params]
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return True
    for g in grads:
        if g.is_sparse:
            raise ValueError("has_finite_gradients does not support sparse gradients")
        if g.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"has_finite_gradients: float32, float16 or bfloat16 gradients, got {g.dtype}")
    devices = {g.device for g in grads}
    if len(devices) > 1:
        raise ValueError(f"has_finite_gradients: the gradients must be on one device, got {sorted(map(str, devices))}")
    dev = devices.pop()
    if dev.type != "cuda":
        raise RuntimeError("has_finite_gradients needs the gradients on an MI355X (no CPU fallback)")
    grads = [g if g.dtype == torch.float32 and g.is_contiguous() else g.to(torch.float32).contiguous() for g in grads]
    n = len(grads)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    ctx = _lib.context(dev)
    with torch.cuda.device(dev):
        ctx.call("e2emv_grads_finite", n, (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]),
                 (ctypes.c_int64 * n)(*[g.numel() for g in grads]), _lib.ptr(flag), _lib.stream_ptr(dev))
    return int(flag.item()) == 0
