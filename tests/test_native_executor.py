"""native_executor.NativeExecutor: the buffer sets a replayed HIP graph holds raw pointers into (one per input shape, least recently
used out, `generation` bumped per eviction), which attributes belong to the executor and which to a set, the refusal of a model
the kernels do not cover -- on a subclass whose `_alloc` makes CPU tensors (no kernel library), and the real executors' declarations."""
import numpy as np
import pytest
import torch

from paddlescience_amd.native_executor import NativeExecutor


class _Model:
    why = None
    bad = ()  # widths whose allocation fails


class _Dummy(NativeExecutor):
    label, supports = "dummy", staticmethod(lambda model: model.why)

    def _alloc(self, B, n):
        self.x = torch.zeros(B, n)
        if n in self.m.bad:
            raise NotImplementedError(f"a row of {n} does not fit")
        self.y = torch.zeros(B, n)
        self.width = n

    def forward(self, x):
        if self.shape != tuple(x.shape):
            self._switch(tuple(x.shape))
        self.x.copy_(x)
        torch.mul(self.x, 2.0, out=self.y)
        return self.y

    def _backward(self, gy):
        pass


def _x(B, n):
    return torch.full((B, n), 1.5)


def test_revisited_shape_gets_its_buffers_back():
    nat = _Dummy(_Model())
    assert nat.shape is None and nat.generation == 0 and nat.max_sets == 8
    ya = nat.forward(_x(2, 3))
    pa = (nat.x.data_ptr(), ya.data_ptr())
    assert nat.shape == (2, 3) and torch.equal(ya, _x(2, 3) * 2)
    yb = nat.forward(_x(4, 3))
    assert nat.shape == (4, 3) and yb.data_ptr() != pa[1] and list(nat._sets) == [(2, 3)]
    ya2 = nat.forward(_x(2, 3))
    assert (nat.x.data_ptr(), ya2.data_ptr()) == pa and nat.shape == (2, 3)
    assert list(nat._sets) == [(4, 3)] and nat.generation == 0


def test_generation_rises_by_one_per_eviction_least_recently_used_first():
    nat = _Dummy(_Model())
    nat.max_sets = 3
    ptr = {}
    for n in (1, 2, 3):  # max_sets shapes in play: nothing is dropped
        ptr[n] = nat.forward(_x(1, n)).data_ptr()
    assert nat.generation == 0 and list(nat._sets) == [(1, 1), (1, 2)]
    nat.forward(_x(1, 1))  # shape 1 becomes the most recently used: 2 is now the oldest
    assert nat.generation == 0 and nat.y.data_ptr() == ptr[1]
    nat.forward(_x(1, 4))  # a fourth shape: exactly one set goes, the least recently used
    assert nat.generation == 1 and sorted(nat._sets) == [(1, 1), (1, 3)]
    nat.forward(_x(1, 5))
    assert nat.generation == 2 and sorted(nat._sets) == [(1, 1), (1, 4)]
    nat.forward(_x(1, 1))  # still there: no allocation, no eviction
    assert nat.generation == 2 and nat.y.data_ptr() == ptr[1]
    nat.forward(_x(1, 3))  # evicted above: allocated again, at the price of another set
    assert nat.generation == 3 and len(nat._sets) == 2


def test_failed_allocation_leaves_the_executor_usable():
    model = _Model()
    model.bad = (7,)
    nat = _Dummy(model)
    ya = nat.forward(_x(2, 3))
    with pytest.raises(NotImplementedError, match="does not fit"):
        nat.forward(_x(2, 7))
    assert nat.shape is None and not hasattr(nat, "y")  # no half-built set is current
    assert list(nat._sets) == [(2, 3)] and nat.generation == 0
    assert torch.equal(nat.forward(_x(2, 5)), _x(2, 5) * 2) and nat.shape == (2, 5)
    assert nat.forward(_x(2, 3)).data_ptr() == ya.data_ptr()  # the set it left behind was kept
    with pytest.raises(NotImplementedError, match="does not fit"):  # and the bad shape fails the same way again
        nat.forward(_x(2, 7))


def test_executor_attributes_survive_a_switch_and_set_attributes_do_not():
    nat = _Dummy(_Model())
    nat.forward(_x(2, 3))
    nat.defer_wgrad_sums = True
    nat._wsegs = [(1, 2, 3, 4)]
    nat.max_sets = 5
    nat.scratch_of_a = torch.ones(3)  # not declared: belongs to the current set
    assert nat.width == 3
    nat.forward(_x(2, 4))
    assert nat.defer_wgrad_sums is True and nat._wsegs == [(1, 2, 3, 4)] and nat.max_sets == 5 and nat.m is not None
    assert nat.wgrad_segments == [(1, 2, 3, 4)]
    assert not hasattr(nat, "scratch_of_a") and nat.width == 4
    assert set(nat.__dict__) - set(nat.EXECUTOR_ATTRS) == {"x", "y", "width"}
    nat.forward(_x(2, 3))
    assert torch.equal(nat.scratch_of_a, torch.ones(3)) and nat.width == 3
    assert nat.defer_wgrad_sums is True and nat._wsegs == [(1, 2, 3, 4)]


def test_backward_frame_resets_then_flushes_unless_deferred(monkeypatch):
    from paddlescience_amd import hotpath as hp

    flushed = []
    monkeypatch.setattr(hp, "reduce_rows_multi", lambda segs, like: flushed.append((list(segs), like)))

    class _Segs(_Dummy):
        def _backward(self, gy):
            assert self._wsegs == []  # the frame cleared the previous pass's
            self._wsegs.append((10, 20, 3, 4))

    nat = _Segs(_Model())
    nat.forward(_x(1, 2))
    nat._wsegs = [(9, 9, 9, 9)]
    nat.backward(None)
    assert len(flushed) == 1 and flushed[0][0] == [(10, 20, 3, 4)] and flushed[0][1] is nat.y and nat.wgrad_segments == []
    nat.defer_wgrad_sums = True
    nat.backward(None)
    assert len(flushed) == 1 and nat.wgrad_segments == [(10, 20, 3, 4)]
    segs = nat.wgrad_segments
    nat.backward(None)  # (a captured step replays no Python: the caller keeps the list it took)
    nat.flush_wgrads(segs)
    assert flushed[1][0] == [(10, 20, 3, 4)] and nat.wgrad_segments == []


def test_unsupported_model_is_refused_with_the_hook_s_reason():
    model = _Model()
    model.why = "too wide"
    with pytest.raises(NotImplementedError, match="^native dummy path: too wide$"):
        _Dummy(model)


@pytest.mark.parametrize("module, cls, label, extra", [
    ("fno_engine", "FnoNative", "FNO", set()), ("uno_engine", "UnoNative", "UNO", set()),
    ("lno_engine", "LnoNative", "LNO", set()), ("geofno_engine", "Fno1dNative", "FNO1d", set())])
def test_real_executors_declare_the_base_s_attributes(module, cls, label, extra):
    import importlib

    mod = importlib.import_module(f"paddlescience_amd.{module}")
    E = getattr(mod, cls)
    assert issubclass(E, NativeExecutor) and E.label == label and E.supports is mod.supports
    assert set(E.EXECUTOR_ATTRS) >= set(NativeExecutor.EXECUTOR_ATTRS)
    assert {"_wsegs", "defer_wgrad_sums"} <= set(E.EXECUTOR_ATTRS)
    assert not {"_wbufs", "_wcall"} & set(E.EXECUTOR_ATTRS)  # device memory of one shape: per set
    assert set(E.EXECUTOR_ATTRS) - set(NativeExecutor.EXECUTOR_ATTRS) == extra
    assert "_switch" not in E.__dict__ and "backward" not in E.__dict__ and "flush_wgrads" not in E.__dict__


def test_deferred_segments_belong_to_the_step_graph_key_that_left_them():
    """OperatorEngine.forward_backward_deferred after a REPLAY (no Python runs, the executor still holds the last eager pass's list):
    the segments of the pass that was run under that key, not of whichever pass ran last."""
    from paddlescience_amd.operator_engine import OperatorEngine

    class _Executor:
        generation, defer_wgrad_sums, wgrad_segments = 0, False, []

    class _Constraint:
        version = 0

        def __init__(self, segs):
            self.segs = segs

        def forward_backward_native(self, native):
            assert native.defer_wgrad_sums is True
            native.wgrad_segments = list(self.segs)

    class _Graphs:
        """A step graph that runs a key's first call and "replays" every later one."""
        max_graphs = 16

        def __init__(self):
            self.seen, self.ran = set(), []

        def run(self, key, eager):
            if key not in self.seen:
                self.seen.add(key)
                eager()
                self.ran.append(key)

        def clear(self):
            self.seen.clear()

    class _Net:
        flat_grad = torch.zeros(1)

        def native(self):
            return _Executor()

    eng = OperatorEngine(_Net())
    eng._step_graph = graphs = _Graphs()
    SA, SB = [(1, 2, 3, 4)], [(5, 6, 7, 8), (9, 10, 11, 12)]
    a, b = _Constraint(SA), _Constraint(SB)
    assert eng.forward_backward_deferred([a]) == SA
    assert eng.forward_backward_deferred([b]) == SB
    assert eng.forward_backward_deferred([a]) == SA and len(graphs.ran) == 2  # (replayed: b's list is what the executor holds)
    assert eng.forward_backward_deferred([b]) == SB and eng.native.defer_wgrad_sums is False
    eng.invalidate_graphs()  # the graphs go, and with them what was recorded for their keys
    a.segs = [(13, 14, 15, 16)]
    assert eng.forward_backward_deferred([a]) == [(13, 14, 15, 16)] and len(graphs.ran) == 3


@pytest.fixture
def emu():
    from paddlescience_amd import _lib, device
    from tests.emu import build_emu

    build_emu.inject()
    device.set_device("cpu")
    yield
    _lib._inject_for_tests(None)
    device.set_device(None)


def test_operator_engine_reports_the_executor_s_own_reason(emu):
    """An LNO whose head does not fit LDS: the engine fails with LnoNative's reason (not with the first executor's "not an FNONet")."""
    import ppsci
    from paddlescience_amd import _lib as L
    from paddlescience_amd.operator_engine import OperatorEngine

    width, hidden = 64, 4096
    assert not L.lib().ppsci_lno_head_supported(width, hidden)
    T, X, Y = (np.linspace(0, 1, n).reshape(1, n) for n in (4, 3, 3))
    model = ppsci.arch.LNO(("input",), ("output",), width, (2, 2, 2), T, (X, Y), 1, hidden)
    with pytest.raises(NotImplementedError, match=f"^native LNO path: width {width} with {hidden} hidden features does not fit the head"):
        OperatorEngine(model)
