"""The contract every operator model's executor keeps (fno_engine.FnoNative, uno_engine.UnoNative, lno_engine.LnoNative,
geofno_engine.Fno1dNative), in one piece: what the operator engine, the solver's eval / predict paths and the HIP-graph capture of
the training step rely on, and do not tell the executors apart by.

    nat = model.native()          one executor per model, shared by training, evaluation and prediction
    y = nat.forward(x)            a buffer owned by the executor; switches to the buffer set of x's shape
    nat.backward(gy)              writes every parameter's `.grad` (views of the model's flat_grad)
    nat.generation                bumped when a buffer set is dropped: part of the engine's graph key
    nat.defer_wgrad_sums = True   backward() leaves the weight gradients' partial rows unsummed
    nat.wgrad_segments            ... for a caller that sums them itself, in one launch with its Adam update,
    nat.flush_wgrads(segs)        ... or hands them back

A subclass supplies `supports` (its module's function), `label`, `_alloc(*key)`, `forward(x)` and `_backward(gy)`; the model class
names it in `_executor` (arch/operator_base.py).  DESIGN.md 4.12."""
from __future__ import annotations

from typing import List, Optional

from . import hotpath as hp


def grads_adjacent(*params) -> bool:
    """Do the gradients of `params` follow each other, in this order, in the flat gradient buffer?  (Then their partial rows
    are ONE segment of the row reduction.)"""
    off = params[0].grad.data_ptr()
    for p in params:
        if p.grad.data_ptr() != off:
            return False
        off += 4 * p.numel()
    return True


class NativeExecutor:
    label = ""        # the model family, as the refusal names it: "native <label> path: <reason>"
    supports = None   # staticmethod(model) -> None when the kernels cover the model, else the reason they do not
    # The attributes of the executor itself.  EVERY other attribute belongs to the current buffer set: it is put away with the
    # set and absent while another shape is current.  A subclass with executor-level state of its own extends the tuple.
    EXECUTOR_ATTRS = ("m", "shape", "_sets", "max_sets", "generation", "defer_wgrad_sums", "_wsegs")

    def __init__(self, model):
        why = type(self).supports(model)
        if why is not None:
            raise NotImplementedError(f"native {self.label} path: {why}")
        self.m = model
        self.shape = None
        # One buffer set per input shape (the key of `_switch`), kept alive: training, evaluation and prediction share this
        # executor, the reference's TFNO config trains at 16 x 16 and evaluates at 32 x 32 with eval_during_train, a ragged
        # last eval batch changes the batch size -- and the operator engine REPLAYS a captured HIP graph of the training step
        # that holds the training buffers' addresses.  Handing those back to the caching allocator when another shape comes by
        # would leave the graph writing through stale pointers.  At most `max_sets` sets are kept (least recently used out);
        # dropping one bumps `generation`, which is part of the engine's graph key, so no captured step outlives its buffers.
        self._sets = {}
        self.max_sets = 8
        self.generation = 0
        self.defer_wgrad_sums = False  # backward() leaves the partials of the weight gradients unsummed (wgrad_segments) when set
        self._wsegs: List[tuple] = []  # (source pointer, destination pointer, rows, cols) of the pass's pending row sums

    # ------------------------------------------------------------------ buffers
    def _switch(self, key: tuple) -> None:
        """Make the buffer set of input shape `key` the current one (`_alloc(*key)` on first use); the previous set stays
        alive under its own key."""
        keep = self.EXECUTOR_ATTRS
        if self.shape is not None:
            self._sets[self.shape] = {k: v for k, v in self.__dict__.items() if k not in keep}
        self.shape = None  # no current set until the new one is complete: a failed allocation leaves the executor usable
        for k in [k for k in self.__dict__ if k not in keep]:
            del self.__dict__[k]
        if key in self._sets:
            self.__dict__.update(self._sets.pop(key))  # (re-inserted when it is switched away from: most recently used last)
            self.shape = key
            return
        while len(self._sets) >= self.max_sets:
            self._sets.pop(next(iter(self._sets)))
            self.generation += 1
        self._alloc(*key)
        self.shape = key

    def _alloc(self, *key) -> None:
        """Allocate the buffer set of input shape `key` as attributes of self (raising leaves the executor without a current set)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ backward
    def backward(self, gy) -> None:
        """gy = dL/dy, shaped like forward()'s result; writes dL/d(parameter) into every parameter's `.grad`."""
        self._wsegs = []
        self._backward(gy)
        if not self.defer_wgrad_sums:
            self.flush_wgrads()  # (deferred: the caller sums them together with its Adam update, operator_engine)

    def _backward(self, gy) -> None:
        """The reverse pass; every weight gradient that ends in a sum over partial rows appends its segment to `_wsegs`."""
        raise NotImplementedError

    @property
    def wgrad_segments(self) -> List[tuple]:
        """The row sums the last backward() left pending (empty once they are flushed)."""
        return list(self._wsegs)

    def flush_wgrads(self, segs: Optional[List[tuple]] = None) -> None:
        """ONE launch sums the per-chunk partials of every weight gradient of the pass (hp.reduce_rows_multi: up to 16 segments
        per launch): eight reductions of ~5 us each were launch latency, not work.  segs: pending sums handed back by a caller
        that took them (`wgrad_segments`) instead of this pass's own."""
        hp.reduce_rows_multi(self._wsegs if segs is None else segs, self.y)
        self._wsegs = []
