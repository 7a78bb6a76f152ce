"""Guard-band arenas for the memory behaviour of a call at the C-ABI.

An arena is one flat byte buffer that holds every caller-owned buffer of one call, each with a guard band of GUARD bytes on both
sides.  The device arena is a torch.uint8 tensor on the GPU; the numpy backend serves the host forms of the calls and the helper's
own test.  Before the call the guard bands and the output buffers hold a poison; snapshot() / check_untouched() copy the whole arena
to the host before and after the call and compare every byte outside the declared outputs: guard bands and inputs in one compare.

    P1  0xFF in every guard and output byte: a NaN as a float, 0xFFFFFFFF as a key, a label or a count.
    P2  chosen so that a stray read changes the answer: guards take zeros (floats), or a cycle of values given as `guard=` (labels
        the index really holds, r_in for counts), laid so that the elements in front of and behind the buffer are whole elements of
        the cycle; output buffers take 0x5A bytes.

A call that reads only its inputs gives the same outputs under both poisons; one that writes all of its outputs leaves none of either
poison where the header documents a value.

GUARD is a condition, not a measurement: 64 KiB is 16 times the largest step a 256-thread workgroup makes with 16-byte loads (4 KiB),
so an access that is off by a row or by a workgroup stays inside the arena and can never leave the allocation."""
import numpy as np

GUARD = 64 * 1024
P1, P2 = "P1", "P2"
POISONS = (P1, P2)
P1_BYTE, P2_OUT_BYTE = 0xFF, 0x5A


class GuardError(AssertionError):
    pass


def bits(a):
    """an array's bytes, so that NaN payloads and -0 take part in a compare"""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(got, want):
    """None, or the first key of two dicts of arrays (or scalars) whose values differ in shape, type or bit pattern"""
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(bits(g), bits(w)):
            return k
    return None


def under_both_poisons(call, **arena):
    """Property R: call(Arena) -> a dict of host arrays, once under P1 and once under P2 on fresh arenas of the same layout.  The
    two dicts must be bit-identical; -> the dict."""
    got = [call(Arena(p, **arena)) for p in POISONS]
    diff = same(got[0], got[1])
    assert diff is None and set(got[0]) == set(got[1]), "%s depends on the poison around the buffers: the call reads outside its inputs, " \
                                                         "or leaves an output element unwritten" % diff
    return got[1]


class _Placement:
    __slots__ = ("name", "role", "off", "nbytes", "lead", "end", "dtype", "shape")


class Arena:
    """Arena(poison, backend="numpy" | "torch", capacity=bytes, device=0).  place() the buffers, snapshot(), make the call,
    check_untouched(outputs)."""

    def __init__(self, poison, backend="numpy", capacity=4 << 20, device=0):
        if poison not in POISONS:
            raise ValueError("poison is P1 or P2")
        self.poison, self.backend, self.capacity = poison, backend, int(capacity)
        fill = P1_BYTE if poison == P1 else 0
        if backend == "numpy":
            self.buf = np.full(self.capacity, fill, np.uint8)
            self.base = self.buf.ctypes.data
        elif backend == "torch":
            import torch
            self._torch = torch
            self.buf = torch.full((self.capacity,), fill, dtype=torch.uint8, device=torch.device("cuda", device))
            self.base = self.buf.data_ptr()
        else:
            raise ValueError("backend is numpy or torch")
        self.cursor = 0                                      # the end of the last guard band
        self.placed = []
        self._before = None

    # ---- layout ----
    def _write(self, off, host_bytes):
        host_bytes = np.ascontiguousarray(host_bytes, np.uint8)
        if self.backend == "numpy":
            self.buf[off:off + host_bytes.size] = host_bytes
        else:
            self.buf[off:off + host_bytes.size] = self._torch.from_numpy(host_bytes).to(self.buf.device)

    def _guard_bytes(self, lo, hi, off, cycle):
        """the poison of arena bytes [lo, hi) around a buffer at `off`: byte i holds cycle[(i - off) mod len]"""
        if self.poison == P1 or cycle is None:
            return np.full(hi - lo, P1_BYTE if self.poison == P1 else 0, np.uint8)
        return cycle[(np.arange(lo, hi, dtype=np.int64) - off) % cycle.size]

    def place(self, array, align, role, guard=None, name=None):
        """Puts a buffer of array's shape and dtype behind a guard band of at least GUARD bytes, at the smallest offset whose ADDRESS
        is align (mod 2 * align): aligned to `align` and to nothing coarser.  role "in": the buffer holds array's values; "out": it
        holds the output poison.  guard: the values P2 cycles through in this buffer's guard bands (array's dtype; no byte of them
        may be 0xFF, so that the two poisons differ everywhere); None: zeros.  -> a typed view (numpy array or torch tensor)."""
        array = np.ascontiguousarray(array)
        if role not in ("in", "out"):
            raise ValueError("role is in or out")
        if align < 1 or align & (align - 1):
            raise ValueError("align is a power of two")
        cycle = None
        if guard is not None:
            cycle = np.ascontiguousarray(guard, array.dtype).reshape(-1).view(np.uint8)
            if cycle.size == 0 or (cycle == P1_BYTE).any():
                raise ValueError("the P2 guard values must exist and hold no 0xFF byte")
        addr = self.base + self.cursor + GUARD
        addr += (align - addr) % (2 * align)
        p = _Placement()
        p.name, p.role = name or "buffer %d" % len(self.placed), role
        p.lead, p.off, p.nbytes = self.cursor, addr - self.base, array.nbytes
        p.end = p.off + p.nbytes + GUARD
        p.dtype, p.shape = array.dtype, array.shape
        if p.end > self.capacity:
            raise ValueError("arena of %d bytes is full" % self.capacity)
        self._write(p.lead, self._guard_bytes(p.lead, p.off, p.off, cycle))
        if role == "in":
            self._write(p.off, array.reshape(-1).view(np.uint8))
        else:
            self._write(p.off, np.full(p.nbytes, P1_BYTE if self.poison == P1 else P2_OUT_BYTE, np.uint8))
        self._write(p.off + p.nbytes, self._guard_bytes(p.off + p.nbytes, p.end, p.off, cycle))
        self.cursor = p.end
        self.placed.append(p)
        return self._view(p)

    def _view(self, p):
        raw = self.buf[p.off:p.off + p.nbytes]
        if self.backend == "numpy":
            return raw.view(p.dtype).reshape(p.shape)
        t = self._torch
        kinds = {"float32": t.float32, "float16": t.float16, "int32": t.int32, "uint32": t.int32, "uint8": t.uint8, "int8": t.int8,
                 "uint16": t.int16, "int64": t.int64, "uint64": t.int64}
        return raw.view(kinds[p.dtype.name]).reshape(p.shape)

    def _placement(self, view):
        addr = view.ctypes.data if self.backend == "numpy" else view.data_ptr()
        for p in self.placed:
            if p.off == addr - self.base:
                return p
        raise KeyError("not a buffer of this arena")

    def ptr(self, view):
        """the address that goes to the C call"""
        return self.base + self._placement(view).off

    def host(self, view):
        """the buffer's contents now, as a numpy array of the placed dtype (uint32 stays uint32)"""
        p = self._placement(view)
        return self._host()[p.off:p.off + p.nbytes].view(p.dtype).reshape(p.shape).copy()

    def guards(self):
        """-> (mask, image): the guard bytes of the arena (everything outside the buffers) as a bool mask, and the arena's bytes"""
        mask = np.ones(self.capacity, bool)
        for p in self.placed:
            mask[p.off:p.off + p.nbytes] = False
        return mask, self._host()

    # ---- the compare ----
    def _host(self):
        if self.backend == "numpy":
            return self.buf.copy()
        self._torch.cuda.synchronize(self.buf.device)        # every fill and every stream of the device is complete
        return self.buf.cpu().numpy()

    def snapshot(self):
        self._before = self._host()

    def check_untouched(self, outputs=()):
        """Every byte outside the declared outputs equals the snapshot.  outputs: placed views — the whole buffer may be written — or
        (view, n): only its first n elements may.  A refused call declares none.  Raises GuardError naming the first byte."""
        if self._before is None:
            raise RuntimeError("snapshot() comes first")
        after = self._host()
        may = np.zeros(self.capacity, bool)
        for o in outputs:
            view, n = o if isinstance(o, tuple) else (o, None)
            p = self._placement(view)
            if p.role != "out":
                raise ValueError("%s is an input" % p.name)
            nbytes = p.nbytes if n is None else int(n) * p.dtype.itemsize
            if nbytes > p.nbytes:
                raise ValueError("%s holds fewer than %d elements" % (p.name, n))
            may[p.off:p.off + nbytes] = True
        bad = np.flatnonzero((after != self._before) & ~may)
        if bad.size:
            raise GuardError("%d bytes outside the declared outputs changed; the first: %s" % (bad.size, self.describe(int(bad[0]))))
        return after

    def describe(self, byte):
        for p in self.placed:
            if p.lead <= byte < p.off:
                return "%d bytes in front of %s" % (p.off - byte, p.name)
            if p.off <= byte < p.off + p.nbytes:
                return "byte %d of %s (%s)" % (byte - p.off, p.name, "input" if p.role == "in" else "outside its declared part")
            if byte < p.end:
                return "%d bytes behind the end of %s" % (byte - p.off - p.nbytes + 1, p.name)
        return "arena byte %d, behind the last guard band" % byte
