"""Guard-band harness: does a call stay inside the arrays it was given?

The comparisons of the suite look at the elements of the declared outputs only, and torch's caching allocator rounds every
request up and packs small ones into shared blocks: a store one row behind an output, or a load 16 bytes behind an input, lands
in slack or in a neighbouring live tensor and nothing notices.  Here every array of a case (tests/stream_order.py: ``Case``) is a
view into an arena of its own,

    [ guard | payload | guard ]        the payload has exactly the declared number of bytes

and the whole arena -- guards, output payloads, everything -- is filled with one byte value before the inputs are written.  After
the call

  * every guard byte must still hold the fill               (a write outside a declared array),
  * every input payload must still hold what was loaded     (a modified input),

and the call is repeated under three fills, 0x00, 0xFF and 0x41: as float32 / float64 zero, NaN and a large finite value (about
12.08 and 2.26e6), as integers 0, -1 and about 1.09e9.  Whatever type a stray element is read as, at least two of the three give
it decisively different values, so a result that depends on bytes outside a declared input differs between the fills; so does an
output element that nothing wrote, because the output payload held the fill.  Every check is byte equality between runs of the
same call; nothing here has a tolerance.

``shift`` moves a payload off its 256-byte boundary by that many elements: 0 is a 256-byte-aligned array, 1 one that has the
alignment of its element type only (the contract of include/gmr_amd.h).

What this cannot show: an over-read whose bytes are discarded, and any access beyond the guard.  A guard is
max(4096, 256 rows of the array) bytes: no kernel of the library handles more than 256 rows per workgroup, so an overrun by one
whole tile of rows still falls inside it.  Plain torch and numpy; nothing here is a fixture or specific to the library."""
import numpy as np

try:
    import torch
except ImportError:
    torch = None

from tests import stream_order as so

FILLS = (0x00, 0xFF, 0x41)
ALIGN = 256
MIN_GUARD = 4096
GUARD_ROWS = 256


def guard_bytes(shape, itemsize):
    """Bytes of each guard of an array: at least 4096, and at least 256 leading-dimension rows."""
    row = int(itemsize)
    for d in tuple(shape)[1:]:
        row *= int(d)
    return max(MIN_GUARD, GUARD_ROWS * row)


class Arena:
    """One array inside its own guarded block of bytes.  ``raw`` is the uint8 block (a device tensor or a numpy array),
    ``view`` the array itself, ``start`` / ``nbytes`` the payload's place in ``raw``."""

    def __init__(self, shape, dtype, shift, device=None):
        """dtype: a torch dtype and a device for a device array, a numpy dtype and ``device=None`` for a host array."""
        shape = tuple(int(d) for d in shape)
        self.host = device is None
        if self.host:
            dtype = np.dtype(dtype)
            itemsize = dtype.itemsize
        else:
            itemsize = torch.empty((), dtype=dtype).element_size()
        self.shape, self.itemsize = shape, itemsize
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        self.guard = guard_bytes(shape, itemsize)
        total = self.guard + ALIGN + shift * itemsize + self.nbytes + self.guard
        if self.host:
            self.raw = np.empty(total, np.uint8)
            addr = self.raw.ctypes.data
        else:
            self.raw = torch.empty(total, dtype=torch.uint8, device=device)
            addr = self.raw.data_ptr()
        self.base = self.guard + (-(addr + self.guard)) % ALIGN    # offset of the 256-byte boundary behind the first guard
        self.start = self.base + shift * itemsize
        assert (addr + self.base) % ALIGN == 0 and self.start >= self.guard and total - (self.start + self.nbytes) >= self.guard
        body = self.raw[self.start:self.start + self.nbytes]
        self.view = body.view(dtype).reshape(shape)
        self.address = addr + self.start

    def _np(self):
        return self.raw if self.host else self.raw.cpu().numpy()

    def fill(self, value):
        if self.host:
            self.raw.fill(value)
        else:
            self.raw.fill_(value)

    def payload(self):
        return self._np()[self.start:self.start + self.nbytes].copy()

    def guard_violations(self, name, value):
        """[(name, "before" | "after", first byte offset, number of bytes)]: offsets count away from the payload's first byte
        (before: negative, -1 is the byte in front of it) resp. from the byte behind its last one (after: 0 is that byte)."""
        a = self._np()
        res = []
        bad = np.flatnonzero(a[:self.start] != value)
        if bad.size:
            res.append((name, "before", int(bad[0]) - self.start, int(bad.size)))
        bad = np.flatnonzero(a[self.start + self.nbytes:] != value)
        if bad.size:
            res.append((name, "after", int(bad[0]), int(bad.size)))
        return res


class GuardedBufs:
    """A working set like ``stream_order.Bufs`` (``dev``, ``host``, ``out``, ``host_out``) whose every array sits in an Arena.
    ``shift``: one number, or (shift of the inputs, shift of the outputs)."""

    def __init__(self, case, device, fill, shift=0):
        shift_in, shift_out = shift if isinstance(shift, tuple) else (shift, shift)
        self.fill_value = fill
        self.arenas = {}
        for k, (t, _) in case.dev_in.items():
            self.arenas["dev:" + k] = Arena(t.shape, t.dtype, shift_in, device)
        for k, (a, _) in case.host_in.items():
            self.arenas["host:" + k] = Arena(a.shape, a.dtype, shift_in)
        for k, (shape, dt) in case.out_spec.items():
            self.arenas["out:" + k] = Arena(shape, dt, shift_out, device)
        for k, (shape, dt) in case.host_out_spec.items():
            self.arenas["host_out:" + k] = Arena(shape, dt, shift_out)
        pick = lambda prefix: {k[len(prefix):]: a.view for k, a in self.arenas.items() if k.startswith(prefix)}  # noqa: E731
        self.dev, self.host, self.out, self.host_out = pick("dev:"), pick("host:"), pick("out:"), pick("host_out:")
        self.loaded = {}

    def load(self, case):
        """The fill into every byte of every arena, then the true inputs into their payloads."""
        for a in self.arenas.values():
            a.fill(self.fill_value)
        for k, (t, _) in case.dev_in.items():
            self.dev[k].copy_(t)
        for k, (a, _) in case.host_in.items():
            self.host[k][...] = a
        self.loaded = {k: a.payload() for k, a in self.arenas.items() if k.startswith(("dev:", "host:"))}

    def violations(self):
        res = []
        for k, a in self.arenas.items():
            res += a.guard_violations(k, self.fill_value)
            if k in self.loaded:
                bad = np.flatnonzero(a.payload() != self.loaded[k])
                if bad.size:
                    res.append((k, "input modified", int(bad[0]), int(bad.size)))
        return res


def _written_only(case, b, ans, fill):
    """Cut every answer down to what the case declares as written -- ``case.written(b, name)``: None for all of it, a number of
    leading rows, or a boolean mask over the array's elements (broadcast to its shape); the other bytes must still hold the fill."""
    res, viol = {}, []
    for name, a in ans.items():
        w = case.written(b, name) if hasattr(case, "written") else None
        if w is None:
            res[name] = a
            continue
        arr = b.host_out[name[5:]] if name.startswith("host:") else b.out[name]
        shape = tuple(arr.shape)
        if isinstance(w, (int, np.integer)):
            mask = np.zeros(shape, bool)
            mask[:int(w)] = True
        else:
            mask = np.broadcast_to(np.asarray(w, bool), shape)
        n_el = int(np.prod(shape, dtype=np.int64))
        mask = np.repeat(mask.reshape(-1), a.size // n_el if n_el else 1)
        res[name] = a[mask]
        bad = np.flatnonzero((a != fill) & ~mask)
        if bad.size:
            viol.append((name, "outside the written extent", int(bad[0]), int(bad.size)))
    return res, viol


def run(case, device, fill, shift_in=0, shift_out=0):
    """One call on the default stream in guarded arrays.  Returns (answer as ``stream_order._answer`` gives it, violations)."""
    b = GuardedBufs(case, device, fill, (shift_in, shift_out))
    st = case.new_struct()
    b.load(case)
    case.fill(st, b, False)
    cuda = torch is not None and torch.device(device).type == "cuda"
    if cuda:
        torch.cuda.synchronize()
    rc = case.invoke(b, st, so.sptr(None))
    if cuda:
        torch.cuda.synchronize()
    assert rc == 0, f"{case.entry} returned {rc}"
    ans, viol = _written_only(case, b, so._answer(case, b, False), fill)
    return ans, b.violations() + viol


def written_part(case, device, plain_answer):
    """A plain answer (``stream_order.serial_answers``) cut to the extents the case declares as written."""
    if not hasattr(case, "written"):
        return plain_answer
    b = GuardedBufs(case, device, so.FILL)       # only its shapes are used, and the host outputs ``written`` may consult
    for k, arr in b.host_out.items():
        arr.reshape(-1).view(np.uint8)[...] = plain_answer["host:" + k]
    return _written_only(case, b, plain_answer, so.FILL)[0]




def check(case, device, plain_answer, shift_in=0, shift_out=0):
    """The three assertions of the harness; returns the answer."""
    runs = {fill: run(case, device, fill, shift_in, shift_out) for fill in FILLS}
    what = f"{case.entry} (shift {shift_in} in, {shift_out} out)"
    for fill, (_, viol) in runs.items():
        assert not viol, f"{what}, fill {fill:#04x}: {viol}"
    first = runs[FILLS[0]][0]
    for fill in FILLS[1:]:
        ans = runs[fill][0]
        assert so.same(first, ans), (f"{what}: the answers under fills {FILLS[0]:#04x} and {fill:#04x} differ in {so.differing(first, ans)}: "
                                     "bytes outside a declared input reached a result, or an output element was not written")
    plain = plain_answer                         # whole, or already cut to the written extents
    if any(plain[k].size != first[k].size for k in first if k in plain):
        plain = written_part(case, device, plain_answer)
    assert so.same(first, plain), f"{what}: differs from the answer in ordinary allocations in {so.differing(first, plain)}"
    return first
