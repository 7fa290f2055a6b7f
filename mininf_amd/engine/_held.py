"""
The step-finishing launch held for the optimizer, and everything that enqueues it.
"""
from __future__ import annotations

import sys
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native as nat
from .. import switches
from .. import engine as _engine   # LAST_FUSIONS is rebound there by every elbo()


# ---- the step-finishing launch held for the optimizer --------------------------------------------
# The ELBO forward that writes the final guide gradients of loss.backward() itself (mi_elbo_forward
# with MI_ELBO_FINAL_GRADS) is the step's last kernel before the optimizer's. The launch is therefore
# held (not enqueued) until its first consumer: when that is the Adam step over its gradients
# (mininf_amd.optim.Adam), the launch runs the update in its last block (mi_elbo_forward_adam) and
# the optimizer has no launch of its own. Any other consumer enqueues it first, as it would have been:
# every native launch (_native.stream_handle), every torch operation on the loss (nn._Loss) or on
# a held gradient (PendingGrad) other than metadata queries, the validation read, graph capture
# boundaries (graph.StepGraph) and the distributed gradient reductions. MININF_AMD_DEFER_STEP=0
# launches at once.

_PENDING: Optional["_PendingStep"] = None

# queries that read no tensor data (they run before the launch without flushing it)
_NO_FLUSH = frozenset({
    torch.Tensor.dim, torch.Tensor.size, torch.Tensor.numel, torch.Tensor.nelement,
    torch.Tensor.is_contiguous, torch.Tensor.stride,
    torch.Tensor.storage_offset, torch.Tensor.element_size, torch.Tensor.is_floating_point,
    torch.Tensor.is_complex, torch.Tensor.get_device, torch.Tensor.ndimension,
    torch.Tensor.requires_grad_})
# tensor-valued properties (everything else read through a property is metadata)
_DATA_PROPERTIES = frozenset({"data", "T", "mT", "H", "mH", "real", "imag", "grad", "_base"})
# properties that hand the device address to another library (CuPy, numba, ...), which then reads
# the data on its own: the launch that writes it must be enqueued first
_RAW_POINTER_PROPERTIES = tuple(p for p in (torch.Tensor.__dict__.get("__cuda_array_interface__"),)
                                if p is not None)


def _called_from_package() -> bool:
    """Whether the Python code asking (the first frame outside this module's flush machinery) is
    mininf_amd's own: the package reads gradient addresses to describe launches that the stream
    orders after the held one, so those reads need no flush."""
    frame = sys._getframe(1)
    while frame is not None and frame.f_globals.get("__name__") == __name__:
        frame = frame.f_back
    name = frame.f_globals.get("__name__", "") if frame is not None else ""
    return name == "mininf_amd" or name.startswith("mininf_amd.")


def _flushes(func) -> bool:
    if func is torch.Tensor.data_ptr:
        # a raw address read by user code (ctypes, a DDP-like hook, another kernel library) is a
        # data use the stream does not see; the package's own descriptor reads are not
        return not _called_from_package()
    if func in _NO_FLUSH:
        return False
    if getattr(func, "__name__", None) == "__get__":
        owner = getattr(func, "__self__", None)
        if any(owner is p for p in _RAW_POINTER_PROPERTIES):
            return True
        return getattr(owner, "__name__", None) in _DATA_PROPERTIES
    return True


def torch_function_flush(func, types, args, kwargs):
    """__torch_function__ of the tensors a held launch writes: flush, then the plain operation."""
    if _PENDING is not None and _flushes(func):
        flush_pending_step()
    return torch._C._disabled_torch_function_impl(func, types, args,
                                                 {} if kwargs is None else kwargs)


class PendingGrad(torch.Tensor):
    """
    A guide gradient (``param.grad``) that the held finishing launch writes: an ordinary tensor
    whose first data use enqueues the launch. Plain ``torch.Tensor`` again once it has run.
    """
    __torch_function__ = classmethod(lambda cls, func, types, args=(), kwargs=None:
                                     torch_function_flush(func, types, args, kwargs))


def grad_meta(g: torch.Tensor):
    """(address, dtype, device, contiguous) of a gradient: a PendingGrad's recorded values (no
    flush hook), any other tensor's own."""
    meta = g.__dict__.get("_mi_meta") if type(g) is PendingGrad else None
    return meta if meta is not None else (g.data_ptr(), g.dtype, g.device, g.is_contiguous())


def _current_stream(device: torch.device) -> int:
    index = getattr(device, "index", None)
    if index is None:
        return torch.cuda.current_stream(device).cuda_stream
    return torch._C._cuda_getCurrentRawStream(index)   # (no torch.cuda.Stream object)


class _PendingStep:
    def __init__(self, launch, what: str, grads: List[torch.Tensor], keep, adapter,
                 stream=None) -> None:
        self._launch = launch        # launch(optimizer argument or None) -> error code
        self.what = what
        # the site launches that finish the ELBO write the step's validation words themselves;
        # the ELBO forward (mi_elbo_forward) only mirrors them
        self.writes_flags = what != "mi_elbo_forward"
        self.grad_ptrs = {g.data_ptr() for g in grads if g is not None}
        self.held: List[Tuple[torch.Tensor, torch.Tensor]] = []   # (param, PendingGrad)
        self._keep = keep            # the launch's buffers, alive until it has run
        self.adapt = adapter         # adapter(mi_adam descriptor) -> launch argument, or None
        # (device, hipStream_t) the launch is enqueued on: the stream current at the forward
        self.stream = stream

    def other_stream(self) -> bool:
        """Whether the stream current now is not the one the launch goes to (a consumer inside
        ``torch.cuda.stream(side)``)."""
        return self.stream is not None and _current_stream(self.stream[0]) != self.stream[1]

    def hold(self, var: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
        """``grad`` as the PendingGrad to assign to ``var.grad``. Its address and layout ride along
        as plain attributes (``_mi_meta``: address, dtype, device, contiguous), so the package's
        own checks (the optimizer's plan, the launch descriptors) read them without a torch call
        -- each torch call on a PendingGrad goes through its flush hook."""
        held = grad.as_subclass(PendingGrad)
        held._mi_meta = (grad.data_ptr(), grad.dtype, grad.device, grad.is_contiguous())
        self.held.append((var, held))
        return held

    def run(self, adam=None) -> None:
        code = self._launch(adam)
        if code == 0 and self.other_stream():
            # the consumer's stream waits for the launch (a wait_stream recorded before this flush
            # could not have seen it)
            device, handle = self.stream
            done = torch.cuda.Event()
            done.record(torch.cuda.ExternalStream(handle, device=device))
            torch.cuda.current_stream(device).wait_event(done)
        self._keep = None
        for var, held in self.held:   # the gradients are ordinary tensors from here on
            if var.grad is held:
                var.grad = held.as_subclass(torch.Tensor)
        self.held = []
        nat.check(code, self.what)


def flush_pending_step() -> None:
    """Enqueue the held finishing launch, if any (without an optimizer step)."""
    global _PENDING
    step = _PENDING
    if step is not None:
        _PENDING = None
        step.run(None)


def discard_pending_step() -> None:
    """Drop the held finishing launch unlaunched (a capture that failed part-way)."""
    global _PENDING
    _PENDING = None


def pending_step() -> Optional[_PendingStep]:
    return _PENDING


def attach_optimizer(adam, grads: Sequence[torch.Tensor]) -> bool:
    """
    Run the held finishing launch with the optimizer step ``adam`` (an ``mi_adam`` descriptor over
    ``grads``) in its last block, when the launch writes at least one of those gradients and the
    step is small enough (<= 16384 elements, csrc/adam_math.hpp kFusedAdamMaxNumel); the other
    gradients are complete already (earlier launches on the stream). False: nothing done.
    """
    global _PENDING
    step = _PENDING
    if step is None or adam.num < 1 or \
            not any(grad_meta(g)[0] in step.grad_ptrs for g in grads):
        return False
    if step.other_stream():
        # an optimizer stepping on another stream than the forward's: the launch runs first (the
        # current stream waits for it), the step on its own
        flush_pending_step()
        return False
    arg = step.adapt(adam)
    if arg is None:
        return False
    _PENDING = None
    step.run(arg)
    _engine.LAST_FUSIONS["optimizer_step"] = 1
    return True


_FUSED_ADAM_MAX_NUMEL = 16384


def _small_adam(adam):
    """The finishing launches take the mi_adam descriptor itself (csrc/adam_math.hpp's limit)."""
    numel = sum(adam.tensors[j].numel for j in range(adam.num))
    return adam if numel <= _FUSED_ADAM_MAX_NUMEL else None


def _defer_step(launch, what: str, grads, keep, adapter=_small_adam, stream=None) -> bool:
    """Hold ``launch`` for the optimizer (True), or False: the caller launches now. ``stream``:
    (device, hipStream_t) the launch goes to, for consumers on other streams."""
    global _PENDING
    if not switches.enabled("DEFER_STEP"):
        return False
    flush_pending_step()
    _PENDING = _PendingStep(launch, what, [g for gs in grads for g in gs if g is not None], keep,
                            adapter, stream)
    return True


nat.set_launch_hook(flush_pending_step)
