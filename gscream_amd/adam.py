"""The optimiser step on the HIP path: Adam for every tensor of every parameter group in one launch.

`Adam` is `torch.optim.Adam` with another `step()`: the same constructor, the same `param_groups`, the same per-parameter state as
`torch.optim.Adam(..., foreach=False, fused=False, capturable=False)` keeps it (`step` a host-side tensor, `exp_avg` / `exp_avg_sq`
shaped like the parameter, created lazily and only for parameters that have a gradient).  `state_dict()` / `load_state_dict()`
therefore interchange with torch's class, and everything that re-keys the optimiser (GaussianModel.cat_tensors_to_optimizer,
_prune_anchor_optimizer, capture / restore, update_learning_rate; this package's anchor_growing and anchor_adjust) works on it
unchanged.  Integration is two lines after GaussianModel.training_setup:

    gaussians.optimizer = gscream_amd.adam.Adam.from_optimizer(gaussians.optimizer)
    gaussians.optimizer_c = gscream_amd.adam.Adam.from_optimizer(gaussians.optimizer_c)

`step()` increments the host-side `step` tensors, builds a table of (p, g, exp_avg, exp_avg_sq, count, seven fp32 scalars) rows and
calls gsr_adam_step (gscream_amd/csrc/adam.hip) once per 32 tensors on the current stream (earlier when 2^22 elements are queued, so
that the device starts on the large tensors while the host fills in the rest).  Nothing is read back, nothing
synchronises, no `step` lives on the device.  The rule per element, fp32 with one rounding per operation (the expression sequence of
torch 1.12, which GScream's environment pins; the installed torch forms m' with lerp_ and rounds differently in the last bit):

    m' = m*b1 + g*c1                 b1 = (float)beta1, c1 = (float)(1 - beta1)
    v' = v*b2 + (c2*g)*g             b2 = (float)beta2, c2 = (float)(1 - beta2)
    d  = sqrt(v') / s2 + e           s2 = (float)sqrt(1 - beta2^t), e = (float)eps
    p' = p + (a*m') / d              a  = (float)(-(lr / (1 - beta1^t)))

with every scalar computed in double from the group's lr, betas, eps and the parameter's own step t (after its increment) and rounded
once to fp32 (`adam_scalars`), as torch passes Python scalars to its kernels.

The WHOLE call takes torch's own step (`last_path = "torch"`, else "hip") if a participating parameter (one with a gradient) is not
fp32, not contiguous, not on a HIP device, has 2^31 - 256 or more elements or a sparse gradient; if a group sets amsgrad, a non-zero
weight_decay, maximize, capturable, differentiable or fused, or holds lr / betas as tensors; if existing state does not have the
layout above; or if `force_torch` is set.  A missing library raises; nothing falls back quietly."""
import ctypes
import math

import numpy as np
import torch

from . import _native

__all__ = ["Adam", "adam_scalars"]

MAX_ELEMENTS = 0x7FFFFF00  # gsr_adam_step's limit per tensor
# step() launches what it has queued once that many elements wait, without filling the table first: the device then works on the large
# tensors (the reference's groups begin with them) while the host prepares the rest, which a host-paced loop does not feel and a
# single step after an idle device does (profiles/adam_timing.json, event_ms).  Small models still take one launch per 32 tensors.
FLUSH_ELEMENTS = 1 << 22
CHUNK_UNITS = 1024         # units (four floats, or one where a pointer is not 16-byte aligned) per block of the kernel (adam.hip ADAM_CHUNK)


def _scalar_dtype():
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32  # torch.optim's _get_scalar_dtype()


def adam_scalars(lr, betas, eps, t):
    """-> (b1, c1, b2, c2, s2, e, a) of the rule above: computed in double, each rounded once to fp32 (returned as Python floats that
    are exactly those fp32 values).  t is the step count after its increment."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    t = float(t)
    f = np.float32
    return (float(f(beta1)), float(f(1.0 - beta1)), float(f(beta2)), float(f(1.0 - beta2)), float(f(math.sqrt(1.0 - beta2 ** t))),
            float(f(float(eps))), float(f(-(float(lr) / (1.0 - beta1 ** t)))))


_C_FLOAT = {torch.float32: ctypes.c_float, torch.float64: ctypes.c_double}


def _increment(step):
    """step += 1 on the host -> the new value.  The usual 0-dim fp32 / fp64 host tensor is incremented in its own memory (a tensor
    operation costs several microseconds, and there is one of these per parameter per step); anything else the way torch does it."""
    c = _C_FLOAT.get(step.dtype)
    if c is None or step.dim() != 0:
        step += 1
        return float(step)
    cell = c.from_address(step.data_ptr())
    cell.value += 1.0
    return cell.value


def _torch_step(opt, closure=None):
    """torch.optim.Adam.step itself, below the profiling / hook wrapper the base class puts around every `step` (this class's step
    already runs inside its own)."""
    f = torch.optim.Adam.step
    if getattr(f, "hooked", False) and hasattr(f, "__wrapped__"):
        f = f.__wrapped__
    return f(opt, closure)


class Adam(torch.optim.Adam):
    force_torch = False  # True: every step() is torch's
    last_path = None     # "hip" / "torch": the path the last step() took

    @classmethod
    def from_optimizer(cls, opt):
        """Adopt an existing torch.optim.Adam: the returned optimiser SHARES its param_groups, state and hooks (the old object keeps
        working on the same state, so use one of the two)."""
        if not isinstance(opt, torch.optim.Adam):
            raise TypeError(f"from_optimizer needs a torch.optim.Adam, got {type(opt).__name__}")
        new = cls.__new__(cls)
        new.__setstate__(opt.__dict__)  # dict.update: the same list of groups, the same state mapping
        return new

    def _plan(self):
        """-> [(group, p, grad, state)] of the parameters that take part, or None when the call has to take torch's step.  Changes
        nothing."""
        if self.force_torch:
            return None
        rows = []
        f32, Tensor, get_state = torch.float32, torch.Tensor, self.state.get
        for group in self.param_groups:
            betas = group["betas"]
            if (group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"] or group["capturable"] or group["differentiable"]
                    or group.get("fused") or isinstance(group["lr"], Tensor) or isinstance(betas[0], Tensor)
                    or isinstance(betas[1], Tensor) or isinstance(group["eps"], Tensor)):
                return None
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if (p.dtype != f32 or not p.is_cuda or not p.is_contiguous() or p.numel() >= MAX_ELEMENTS or g.is_sparse
                        or g.dtype != f32 or g.device != p.device or g.shape != p.shape):
                    return None
                state = get_state(p)
                if state:
                    step, m, v = state.get("step"), state.get("exp_avg"), state.get("exp_avg_sq")
                    if (not isinstance(step, Tensor) or step.is_cuda or m is None or v is None
                            or m.dtype != f32 or m.device != p.device or m.shape != p.shape or not m.is_contiguous()
                            or v.dtype != f32 or v.device != p.device or v.shape != p.shape or not v.is_contiguous()):
                        return None
                rows.append((group, p, g, state))
        return rows

    @staticmethod
    def _launch(device, entries):
        table = (_native.AdamTensor * len(entries))(*entries)
        _native.run("gsr_adam_step", device, len(entries), table)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows = self._plan()
        if rows is None:
            self.last_path = "torch"
            _torch_step(self, None)
            return loss
        self.last_path = "hip"
        if not rows:
            return loss
        queued, keep, scalars = {}, [], {}
        for group, p, g, state in rows:
            if not state:  # lazily, as torch creates it
                state = self.state[p]
                state["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            t = _increment(state["step"])
            n = p.numel()
            if n == 0:
                continue
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)  # alive until its launch is enqueued
            lr, betas, eps = group["lr"], group["betas"], group["eps"]
            key = (lr, betas[0], betas[1], eps, t)
            k = scalars.get(key)
            if k is None:
                k = scalars[key] = adam_scalars(lr, betas, eps, key[4])
            q = queued.get(p.device)
            if q is None:
                q = queued[p.device] = [[], 0]
            q[0].append((p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), n) + k)
            q[1] += n
            if len(q[0]) == _native.ADAM_MAX_TENSORS or q[1] >= FLUSH_ELEMENTS:  # a full table, or enough work to start the device on
                self._launch(p.device, q[0])
                q[0], q[1] = [], 0
        for device, q in queued.items():
            if q[0]:
                self._launch(device, q[0])
        return loss
