"""The guard-band harness (tests/guard_band.py) can fail: shown on the CPU with small fake entries written in numpy.

The fake is a row-wise ``y = 2 x`` over [n, 3] float64, clip by clip after a host table of offsets, which also fills a host
output with the number of rows it handled.  It receives addresses, as a C entry does, and touches memory through them, so a
defective variant really does leave its arrays -- by at most one tile of rows, which stays inside the arena's guard.  One variant
is correct; every other has one defect, and each defect is caught by exactly the check of ``guard_band.check`` named beside it."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import guard_band as gb  # noqa: E402
from tests import stream_order as so  # noqa: E402

N, TILE = 70, 64
OFFS = np.array([0, 33, 34, N], np.int64)
F64 = torch.float64
STRAY = np.frombuffer(b"\x5a" * 8, np.float64)[0]   # what a defective fake writes: no byte of it equals a fill


def _mem(addr, count, dtype=np.float64):
    """`count` elements of memory at an address, as a writable numpy array."""
    nbytes = count * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_ubyte * nbytes).from_address(addr), dtype=dtype)


def _x():
    x = np.random.default_rng(7).normal(size=(N, 3))
    x[0, 0] = x[-1, -1] = 0.0   # where a stray zero is added, or a zero left unwritten, the result is still right: only the
    return x                    # comparison between the fills can tell


class Fake(so.Case):
    entry = "fake_double"

    def __init__(self, defect=None):
        super().__init__()
        self.defect = defect
        x = _x()
        self.dev_in = {"x": (torch.from_numpy(x), torch.from_numpy(x + 1.0))}
        self.host_in = {"offsets": (OFFS, OFFS)}
        self.out_spec = {"y": ((N, 3), F64)}
        self.host_out_spec = {"count": ((1,), np.int64)}

    def invoke(self, b, st, stream):
        d = self.defect
        px, py = b.dev["x"].data_ptr(), b.out["y"].data_ptr()
        offs_addr, count_addr = b.host["offsets"].ctypes.data, b.host_out["count"].ctypes.data
        n_seq = len(OFFS) - 1
        offs = _mem(offs_addr, n_seq + 2, np.int64)        # (the entry behind the table is touched by one defect only)
        x, y = _mem(px - 8, 3 * N + 2)[1:], _mem(py - 8, 3 * (N + TILE) + 1)[1:]
        wrong_path = d == "misaligned path differs" and py % 16 != 0
        for c in range(n_seq):
            lo, hi = 3 * int(offs[c]), 3 * int(offs[c + 1])
            if d == "leaves the last element unwritten" and c == n_seq - 1:
                hi -= 1
            y[lo:hi] = 2.0 * x[lo:hi] if not wrong_path else 2.0 * x[lo:hi] + 1.0
        if d == "modifies an input":
            _mem(px + 8 * 4, 8, np.uint8)[:] ^= 0xFF
        if d == "writes one element behind the output":
            y[3 * N] = STRAY
        if d == "writes one element before the output":
            _mem(py - 8, 1)[0] = STRAY
        if d == "writes a tile behind the output":
            y[3 * N:3 * (N + TILE)] = STRAY
        if d == "reads behind the input":
            y[3 * N - 1] = 2.0 * x[3 * N - 1] + x[3 * N]
        if d == "reads before the input":
            y[0] = 2.0 * x[0] + _mem(px - 8, 1)[0]
        stray = int(offs[n_seq + 1]) if d == "reads past the host table" else 0
        _mem(count_addr, 1, np.uint64)[0] = (int(offs[n_seq]) - int(offs[0]) + stray) & (2 ** 64 - 1)
        if d == "writes one byte behind a host output":
            _mem(count_addr + 8, 1, np.uint8)[0] = 0x5A
        return 0


def _plain():
    y = 2.0 * _x()
    return {"y": y.view(np.uint8).reshape(-1).copy(), "host:count": np.array([N], np.int64).view(np.uint8).copy()}


def _violations(defect, shift=0):
    return {fill: gb.run(Fake(defect), "cpu", fill, shift, shift)[1] for fill in gb.FILLS}


@pytest.mark.parametrize("shift", [0, 1])
def test_the_correct_fake_passes(shift):
    ans = gb.check(Fake(), "cpu", _plain(), shift, shift)
    assert so.same(ans, _plain())


# defect -> the violation every fill must report, exactly
REPORTED = {
    "writes one element behind the output": ("out:y", "after", 0, 8),
    "writes one element before the output": ("out:y", "before", -8, 8),
    "writes a tile behind the output": ("out:y", "after", 0, 8 * 3 * TILE),
    "modifies an input": ("dev:x", "input modified", 8 * 4, 8),
    "writes one byte behind a host output": ("host_out:count", "after", 0, 1),
}


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("defect", sorted(REPORTED))
def test_a_write_outside_or_into_an_input_is_reported(defect, shift):
    name, side, offset, nbytes = REPORTED[defect]
    for fill, viol in _violations(defect, shift).items():
        assert len(viol) == 1, (fill, viol)
        assert viol[0] == (name, side, offset, nbytes), (fill, viol)
    with pytest.raises(AssertionError, match=side):
        gb.check(Fake(defect), "cpu", _plain(), shift, shift)


# defect -> the output in which the three fills' answers differ
DEPENDS = {
    "reads behind the input": "y",
    "reads before the input": "y",
    "reads past the host table": "host:count",
    "leaves the last element unwritten": "y",
}


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("defect", sorted(DEPENDS))
def test_a_result_that_depends_on_outside_bytes_differs_between_the_fills(defect, shift):
    runs = {fill: gb.run(Fake(defect), "cpu", fill, shift, shift) for fill in gb.FILLS}
    assert all(not viol for _, viol in runs.values()), runs     # nothing was written outside: the guards alone see nothing
    zero = runs[0x00][0]
    assert so.same(zero, _plain()), "under the zero fill this defect gives the right answer: equality with the plain answer alone sees nothing"
    for fill in (0xFF, 0x41):
        assert so.differing(zero, runs[fill][0]) == [DEPENDS[defect]]
    with pytest.raises(AssertionError, match="fills .* differ"):
        gb.check(Fake(defect), "cpu", _plain(), shift, shift)


def test_a_wrong_answer_on_the_element_aligned_path_is_seen_by_the_plain_comparison_only():
    """(not a bounds defect: the third assertion's own control.  The fake's path for an output off a 16-byte boundary computes
    something else, inside its arrays and independent of the fill.)"""
    case = Fake("misaligned path differs")
    gb.check(case, "cpu", _plain(), 0, 0)
    runs = {fill: gb.run(case, "cpu", fill, 1, 1) for fill in gb.FILLS}
    assert all(not viol for _, viol in runs.values())
    assert all(so.same(runs[0x00][0], runs[f][0]) for f in gb.FILLS)
    with pytest.raises(AssertionError, match="ordinary allocations"):
        gb.check(case, "cpu", _plain(), 1, 1)


def test_a_declared_written_extent_is_compared_alone_and_the_rest_must_hold_the_fill():
    class Partial(Fake):
        def written(self, b, name):
            return 34 if name == "y" else None

        def invoke(self, b, st, stream):
            y = _mem(b.out["y"].data_ptr(), 3 * N)
            y[:3 * 34] = 2.0 * _mem(b.dev["x"].data_ptr(), 3 * 34)
            if self.defect:
                y[3 * 40] = STRAY
            _mem(b.host_out["count"].ctypes.data, 1, np.int64)[0] = N
            return 0
    plain = _plain()
    plain["y"][8 * 3 * 34:] = so.FILL           # what a run in ordinary allocations leaves there
    ans = gb.check(Partial(), "cpu", plain)
    assert ans["y"].size == 8 * 3 * 34
    with pytest.raises(AssertionError, match="outside the written extent"):
        gb.check(Partial("writes behind its extent"), "cpu", plain)

    class Columns(Fake):                        # the same with a mask: the middle column is left alone
        def written(self, b, name):
            return np.array([True, False, True]) if name == "y" else None

        def invoke(self, b, st, stream):
            y, x = _mem(b.out["y"].data_ptr(), 3 * N).reshape(N, 3), _mem(b.dev["x"].data_ptr(), 3 * N).reshape(N, 3)
            y[:, ::2] = 2.0 * x[:, ::2]
            if self.defect:
                y[5, 1] = STRAY
            _mem(b.host_out["count"].ctypes.data, 1, np.int64)[0] = N
            return 0
    plain = _plain()
    plain["y"].reshape(N, 3, 8)[:, 1] = so.FILL
    ans = gb.check(Columns(), "cpu", plain)
    assert ans["y"].size == 8 * 2 * N
    with pytest.raises(AssertionError, match="outside the written extent"):
        gb.check(Columns("writes into the column it leaves alone"), "cpu", plain)


# ------------------------------------------------------------------ arena arithmetic
@pytest.mark.parametrize("shape, itemsize, want", [((10,), 4, 4096), ((0,), 8, 4096), ((5000,), 8, 4096), ((7, 3), 8, 256 * 24), ((200, 30, 4), 4, 256 * 480),
                                                   ((0, 55, 3), 8, 256 * 1320), ((3, 2), 4, 4096)])
def test_guard_size_rule(shape, itemsize, want):
    assert gb.guard_bytes(shape, itemsize) == want


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("shape, tdt, ndt", [((7, 3), torch.float64, np.float64), ((13,), torch.float32, np.float32), ((5, 2), torch.int32, np.int32),
                                             ((9,), torch.int64, np.int64), ((101,), torch.uint8, np.uint8), ((0, 55, 3), torch.float64, np.float64)])
def test_arena_arithmetic(shape, tdt, ndt, host, shift):
    a = gb.Arena(shape, ndt if host else tdt, shift, None if host else "cpu")
    item = np.dtype(ndt).itemsize
    n = int(np.prod(shape)) * item
    raw_addr = a.raw.ctypes.data if host else a.raw.data_ptr()
    assert a.nbytes == n and tuple(a.view.shape) == shape                      # the payload is exact
    assert (raw_addr + a.base) % 256 == 0 and a.start == a.base + shift * item
    assert a.address == raw_addr + a.start
    if shift:
        assert a.address % 16 == item % 16
    else:
        assert a.address % 256 == 0
    if n:
        assert (a.view.ctypes.data if host else a.view.data_ptr()) == a.address
    g = gb.guard_bytes(shape, item)
    assert a.start >= g and len(a.raw) - (a.start + n) >= g
    a.fill(0x41)
    assert not a.guard_violations("a", 0x41) and (a.payload() == 0x41).all()
    if n:
        (a.view.reshape(-1) if host else a.view.reshape(-1).numpy())[...] = 0   # writing all of the payload touches no guard
        assert not a.guard_violations("a", 0x41) and (a.payload() == 0).all()


def test_a_zero_length_array_gets_a_usable_arena_and_a_null_pointer():
    case = so.Case()
    case.dev_in = {"x": (torch.empty((0, 3), dtype=F64), torch.empty((0, 3), dtype=F64))}
    case.host_in = {"t": (np.empty((0,), np.int32), np.empty((0,), np.int32))}
    case.out_spec = {"y": ((0, 3), F64)}
    case.host_out_spec = {}
    b = gb.GuardedBufs(case, "cpu", 0xFF, 1)
    b.load(case)
    assert b.dev["x"].shape == (0, 3) and b.out["y"].numel() == 0 and b.host["t"].size == 0
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731  (as the GPU tests' P())
    assert P(b.dev["x"]) is None and P(b.out["y"]) is None
    assert not b.violations()
    b.arenas["out:y"].raw[b.arenas["out:y"].start] = 0       # the byte a one-element store would hit: the guard behind
    assert b.violations() == [("out:y", "after", 0, 1)]
