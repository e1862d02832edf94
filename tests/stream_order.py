"""Late-producer harness for the stream-order contract of include/gmr_amd.h.

A *case* is one call of one entry point with everything it reads in two versions: the true inputs and a decoy -- a complete,
valid input of the same shapes that gives a different answer.  The harness runs the call under four schedules and compares
bytes:

  serial        default stream, synchronised before and after: the true answer (twice: the call must be deterministic), the answer
                to the decoy device inputs and the answer to the decoy host arrays.  Both decoy answers must differ from the true
                one, or the schedules below could not tell an ordering error from a correct run.
  late          on a side stream S: the device inputs hold the decoy, a bounded spin (torch.cuda._sleep) and then device-to-device
                copies of the true inputs are enqueued, the call is issued behind them with no host synchronisation, and every
                host array (and struct) it was given by pointer is overwritten with its decoy as soon as it returns.  A snapshot
                enqueued on S must equal the true answer.  The producer must still be running when the call is issued, or the run
                proves nothing and fails as vacuous.
  control       the same, but the call goes on a second stream that does not wait for S: it must see the decoy device inputs.
                This is the proof that the harness can fail.
  two streams   two cases of the same handle, each behind its own late producer on its own stream, two calls each, issued
                A, B, A, B, one synchronise at the end.

Because every decoy is valid, a library that reads early, late or on the wrong stream computes a wrong answer, never an address
out of range.  Plain torch; nothing here is a fixture."""
import ctypes as C
import json
import time

import numpy as np

try:
    import torch
except ImportError:  # the host checks import this module for its constants only
    torch = None

FILL = 0xA5                 # byte pattern of an output nothing wrote
SPIN_FACTOR = 10.0          # spin = SPIN_FACTOR x the case's own serial time: host jitter between arming and issuing cannot drain S
SPIN_MIN_MS, SPIN_MAX_MS = 5.0, 250.0


class Bufs:
    """One working set of a case: device inputs, host arrays, outputs (device and host)."""

    def __init__(self, case, device):
        self.dev = {k: torch.empty_like(t) for k, (t, _) in case.dev_in.items()}
        self.host = {k: np.empty_like(t) for k, (t, _) in case.host_in.items()}
        self.out = {k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in case.out_spec.items()}
        self.snap = {k: torch.empty_like(t) for k, t in self.out.items()}
        self.host_out = {k: np.empty(shape, dtype=dt) for k, (shape, dt) in case.host_out_spec.items()}

    def load(self, case, dev_decoy: bool, host_decoy: bool):
        """Fill the inputs (on the current stream) and put the fill pattern into every output."""
        for k, pair in case.dev_in.items():
            self.dev[k].copy_(pair[1 if dev_decoy else 0])
        self.load_host(case, host_decoy)
        for t in list(self.out.values()) + list(self.snap.values()):
            if t.numel():
                t.view(torch.uint8).fill_(FILL)
        for a in self.host_out.values():
            a.view(np.uint8).fill(FILL)

    def load_host(self, case, decoy: bool):
        for k, pair in case.host_in.items():
            self.host[k][...] = pair[1 if decoy else 0]


class Case:
    """One entry point's call.  Subclasses (tests/test_gpu_stream_order.py) set

      dev_in         name -> (true tensor, decoy tensor): device arrays the call reads
      host_in        name -> (true array, decoy array): host arrays the call receives by pointer
      out_spec       name -> (shape, torch dtype): device arrays the call writes
      host_out_spec  name -> (shape, numpy dtype): host arrays the call fills before it returns (only entries that synchronise)
      sort_rows      names of outputs whose row order is defined by atomics: compared with their rows sorted
      synchronises   the header says that the entry synchronises the stream before it returns
      launches, h2d  kernels and host-to-device table copies one call of this case enqueues (read off api.hip)

    and implement ``new_struct()`` (storage for the structs the call passes by pointer, or None), ``fill(st, b, decoy)`` (point the
    structs at working set ``b``; ``decoy``: the by-value fields take their decoy values too) and ``invoke(b, st, stream)``."""

    entry = ""
    synchronises = False
    struct_values = False   # the structs carry by-value fields that have a decoy of their own (fill's ``decoy``)
    launches = h2d = 0
    sort_rows = ()

    def __init__(self):
        self.dev_in, self.host_in, self.out_spec, self.host_out_spec = {}, {}, {}, {}

    def new_struct(self):
        return None

    def fill(self, st, b, decoy):
        pass

    def invoke(self, b, st, stream):
        raise NotImplementedError


def sptr(stream):
    return C.c_void_p(stream.cuda_stream if stream is not None else 0)


def _answer(case, b, from_snap: bool):
    """The outputs as bytes: name -> numpy uint8 array (rows sorted where the order is defined by atomics)."""
    res = {}
    for k, t in (b.snap if from_snap else b.out).items():
        a = t.cpu().numpy()
        if k in case.sort_rows and a.size:
            n = case.sort_rows_count(b, a) if hasattr(case, "sort_rows_count") else a.shape[0]
            head = a[:n]
            a = np.concatenate([head[np.lexsort(head.T[::-1])], a[n:]])
        res[k] = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    for k, a in b.host_out.items():
        a = a.copy()
        if k in case.sort_rows and a.size:
            n = case.sort_rows_count(b, a)
            head = a[:n]
            a = np.concatenate([head[np.lexsort(head.T[::-1])], a[n:]])
        res["host:" + k] = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    return res


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


class Slot:
    """A working set plus, for a case that passes structs, the struct storage and the *bin*: a second, complete working set holding
    the decoy inputs, which the structs are pointed at once the call has returned (a late read of a struct then computes into the
    bin and leaves the compared outputs at the fill pattern)."""

    def __init__(self, case, device):
        self.main = Bufs(case, device)
        self.st = case.new_struct()
        self.bin = Bufs(case, device) if self.st is not None else None

    def arm(self, case, dev_decoy: bool):
        self.main.load(case, dev_decoy, False)
        if self.bin is not None:
            self.bin.load(case, True, True)

    def call(self, case, stream):
        case.fill(self.st, self.main, False)
        rc = case.invoke(self.main, self.st, sptr(stream))
        assert rc == 0, f"{case.entry} returned {rc}"

    def poison(self, case):
        """Overwrite every host array and struct the call received by pointer with its decoy."""
        self.main.load_host(case, True)
        if self.st is not None:
            case.fill(self.st, self.bin, True)


def serial_answers(case, device):
    """The serial answers of a case and the event-timed duration of its call: dict(true=, dev_decoy=, host_decoy=, ms=).
    ``deterministic`` is False when two true-input runs differ; the decoy answers are then not computed."""
    res = {}
    slot = Slot(case, device)
    runs = [("true", False, False), ("true2", False, False)]
    if case.dev_in:
        runs.append(("dev_decoy", True, False))
    if case.host_in or case.struct_values:
        runs.append(("host_decoy", False, True))
    for name, dd, hd in runs:
        slot.main.load(case, dd, hd)
        case.fill(slot.st, slot.main, hd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rc = case.invoke(slot.main, slot.st, sptr(None))
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, f"{case.entry} ({name}) returned {rc}"
        res[name] = _answer(case, slot.main, False)
        if name == "true2":
            res["ms"] = e0.elapsed_time(e1)   # the second run: code objects loaded, pool blocks cached
            res["deterministic"] = same(res["true"], res["true2"])
            if not res["deterministic"]:
                break
    return res


def calibrate_spin():
    """Milliseconds per cycle of torch.cuda._sleep, from two event-timed spins of different lengths."""
    ms = []
    cycles = (2_000_000, 20_000_000)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    for c in cycles:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(c)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    slope = (ms[1] - ms[0]) / (cycles[1] - cycles[0])
    assert slope > 0, ms
    return {"cycles": list(cycles), "ms": ms, "ms_per_cycle": slope}


def spin_ms_for(serial_ms):
    return float(min(SPIN_MAX_MS, max(SPIN_MIN_MS, SPIN_FACTOR * serial_ms)))


_STREAMS = {}


def streams(device):
    """The module's three side streams, made once (consecutively, so that the runtime spreads them over its hardware queues)."""
    key = str(device)
    if key not in _STREAMS:
        _STREAMS[key] = [torch.cuda.Stream(device) for _ in range(3)]
        for s in _STREAMS[key]:   # first use of a stream sets up its hardware queue, which takes longer than a short spin lasts
            with torch.cuda.stream(s):
                torch.cuda._sleep(1000)
        torch.cuda.synchronize()
    return _STREAMS[key]


def _produce(case, slot, stream, cycles):
    """Steps 2-4: spin, the true inputs, the event."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles))
        for k, (t, _) in case.dev_in.items():
            slot.main.dev[k].copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def _snapshot(slot, stream):
    with torch.cuda.stream(stream):
        for k, t in slot.main.out.items():
            slot.main.snap[k].copy_(t, non_blocking=True)


def run_late(case, device, cycles, control=False):
    """The late-producer schedule (``control``: the call goes on a stream that does not wait for the producer).
    Returns dict(answer=, vacuous=, returned_before_producer=, issue_ms=, overtook_producer=); the last one says, for the control,
    that the call had finished before the producer did -- otherwise the control saw the true inputs and shows nothing."""
    S = streams(device)[0]
    call_stream = streams(device)[2] if control else S
    slot = Slot(case, device)
    slot.arm(case, True)
    torch.cuda.synchronize()
    ev = _produce(case, slot, S, cycles)
    vacuous = ev.query()
    t0 = time.perf_counter()
    slot.call(case, call_stream)
    issue_ms = (time.perf_counter() - t0) * 1e3
    before = not ev.query()
    slot.poison(case)
    _snapshot(slot, call_stream)
    call_stream.synchronize()
    overtook = not ev.query()   # control: the call and its snapshot were through while the producer was still spinning
    S.synchronize()
    torch.cuda.synchronize()
    return {"answer": _answer(case, slot.main, True), "vacuous": vacuous, "returned_before_producer": before, "issue_ms": issue_ms,
            "overtook_producer": overtook}


def run_two_streams(case_a, case_b, device, cycles_a, cycles_b):
    """A on S1 and B on S2, each behind its own late producer, two calls each into separate working sets, issued A, B, A, B.
    Returns (answers of A's two calls, answers of B's two calls, vacuous)."""
    S = streams(device)[:2]
    cases, cycles = [case_a, case_b], [cycles_a, cycles_b]
    slots = [[Slot(c, device), Slot(c, device)] for c in cases]
    for c, pair in zip(cases, slots):
        for s in pair:
            s.arm(c, True)
    torch.cuda.synchronize()
    evs = []
    for c, pair, st, cyc in zip(cases, slots, S, cycles):
        with torch.cuda.stream(st):
            torch.cuda._sleep(int(cyc))
            for s in pair:
                for k, (t, _) in c.dev_in.items():
                    s.main.dev[k].copy_(t, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        evs.append(ev)
    vacuous = any(e.query() for e in evs)
    for rnd in range(2):
        for i in range(2):
            slots[i][rnd].call(cases[i], S[i])
            slots[i][rnd].poison(cases[i])
            _snapshot(slots[i][rnd], S[i])
    torch.cuda.synchronize()
    ans = [[_answer(cases[i], slots[i][r].main, True) for r in range(2)] for i in range(2)]
    return ans[0], ans[1], vacuous


def write_profile(path, calibration, entries, large_tables, sweep):
    with open(path, "w") as f:
        json.dump({"what": "stream-order harness (tests/stream_order.py): spin calibration and, per entry, the serial time of the test's "
                           "case, the spin its late producer used and whether the call returned before the producer had finished",
                   "spin_calibration": calibration, "entries": entries, "large_host_tables": large_tables,
                   "pageable_copy_sweep_gmr_fk_min_height": sweep}, f, indent=1, sort_keys=True)
        f.write("\n")
