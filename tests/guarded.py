"""Guard bands around the buffers a C-ABI call is given (tests/test_guard_bands_gpu.py, tests/test_guarded.py).

A torch tensor handed to a kernel sits inside the caching allocator's rounded-up block, next to other tensors of
the same process, so a store a few bytes past its end neither faults nor changes the value a test compares.  A
Guarded buffer is one flat allocation

    band | lead | interior | band

with 64 KiB bands of a known content on both sides of the interior the kernel is given: a stray write changes a
band (check() finds it and says where), a stray read picks up the band's content (NaN for an input, so it shows in
the values).  `lead` elements shift the interior off its 16-byte alignment.  Works on CPU and CUDA tensors.
"""
import ctypes

import torch

BAND = 64 * 1024          # bytes on either side; a multiple of 256 keeps the interior 16-byte aligned
OUT_BYTE = 0x5A           # "out" bands and never-written interiors: 0x5A5A.. is finite in every float format
WS_BYTES = (0xFF, 0x00)   # the two pre-fills of an "uninitialised" workspace

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# quiet NaNs with a recognisable payload, as the signed integer of the same width
_NAN_BITS = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FCAFE5A,
             torch.float64: 0x7FF8CAFE5A5A5A5A}
_INT_EXTREME = {torch.int16: 32767, torch.int32: -1, torch.int64: -1, torch.uint8: 0xFF, torch.int8: -1}


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def band_value(dtype, kind):
    """(integer view dtype, integer fill value) of a band of `kind` around an interior of `dtype`."""
    es = _esize(dtype)
    iv = _INT_VIEW[es]
    if kind == "in":
        v = _NAN_BITS[dtype] if dtype.is_floating_point else _INT_EXTREME[dtype]
        return iv, v
    pat = int.from_bytes(bytes([OUT_BYTE]) * es, "little", signed=False)
    if iv != torch.uint8 and pat >= 1 << (8 * es - 1):
        pat -= 1 << (8 * es)
    return iv, pat


class GuardError(AssertionError):
    pass


class Guarded:
    """One buffer of n_elems elements of dtype between two bands.  kind: "in" (bands NaN / extreme integer, the
    interior must come back unchanged), "out" (bands and interior a fixed non-zero byte pattern), "ws" (bands as
    "out", the interior filled with the byte `ws_byte`).  `.t` is the interior."""

    def __init__(self, n_elems, dtype, device, kind, lead=0, ws_byte=WS_BYTES[0]):
        assert kind in ("in", "out", "ws"), kind
        self.kind, self.dtype, self.n, self.lead = kind, dtype, int(n_elems), int(lead)
        es = self.es = _esize(dtype)
        assert BAND % 256 == 0 and BAND % es == 0
        self.front = BAND + self.lead * es            # bytes before the interior (band + lead)
        self.nbytes = self.n * es
        self.raw = torch.empty(self.front + self.nbytes + BAND, dtype=torch.uint8, device=device)
        iv, val = band_value(dtype, kind)
        self._iv, self._val = iv, val
        self._front_view().fill_(val)
        self._rear_view().fill_(val)
        inner = self.raw[self.front:self.front + self.nbytes]
        self.t = inner.view(dtype) if self.n else torch.empty(0, dtype=dtype, device=device)
        if kind == "out":
            inner.fill_(OUT_BYTE)
        elif kind == "ws":
            inner.fill_(ws_byte)
        self._snap = None

    def _front_view(self):
        return self.raw[:self.front].view(self._iv)

    def _rear_view(self):
        return self.raw[self.front + self.nbytes:].view(self._iv)

    def set(self, src):
        """Copy `src` (any shape, n_elems elements) into the interior; an "in" buffer remembers the bytes."""
        self.t.copy_(src.reshape(-1).to(self.t.device))
        return self.freeze()

    def freeze(self):
        """Remember the interior's bytes: check() of an "in" buffer compares against them."""
        if self.kind == "in":
            self._snap = self.raw[self.front:self.front + self.nbytes].clone()
        return self

    def data_ptr(self):
        return self.raw.data_ptr() + self.front

    def _changed(self, region, expect=None):
        """Byte offsets (sorted, int64 CPU tensor) within `region` (a uint8 view) whose value changed."""
        if expect is None:
            es = self.es
            want = torch.tensor([self._val], dtype=self._iv).view(torch.uint8).repeat(region.numel() // es)
            expect = want.to(region.device)
        return torch.nonzero(region != expect).flatten().cpu()

    def check(self, name="buffer"):
        inner = self.raw[self.front:self.front + self.nbytes]
        dirty = (self._front_view() != self._val).any() | (self._rear_view() != self._val).any()
        if self.kind == "in" and self._snap is not None:
            dirty = dirty | (inner != self._snap).any()
        if not bool(dirty):     # one device round trip when all is well; the details only on a failure
            return
        front = self._changed(self.raw[:self.front])
        if front.numel():
            dist = self.front - int(front[-1])      # nearest changed byte, counted back from the interior
            raise GuardError("`%s`: %d B written before the start (%d bytes of the front band changed)"
                             % (name, dist, front.numel()))
        rear = self._changed(self.raw[self.front + self.nbytes:])
        if rear.numel():
            raise GuardError("`%s`: %d B written past the end (%d bytes of the rear band changed)"
                             % (name, int(rear[0]) + 1, rear.numel()))
        if self.kind == "in" and self._snap is not None:
            inner = self._changed(self.raw[self.front:self.front + self.nbytes], self._snap)
            if inner.numel():
                raise GuardError("`%s`: const input modified (%d bytes, first at byte offset %d)"
                                 % (name, inner.numel(), int(inner[0])))


class Plain:
    """The same interface on an ordinary, generously sized torch tensor (the plain run of a guard-band case)."""

    def __init__(self, n_elems, dtype, device, kind, lead=0, ws_byte=WS_BYTES[1]):
        self.kind, self.dtype, self.n = kind, dtype, int(n_elems)
        es = _esize(dtype)
        self.front = int(lead) * es                   # the same misalignment as the guarded run: the same code path
        self.raw = torch.zeros(self.front + (self.n + 4096) * es, dtype=torch.uint8, device=device)
        inner = self.raw[self.front:self.front + self.n * es]
        self.t = inner.view(dtype) if self.n else torch.empty(0, dtype=dtype, device=device)
        if kind != "in":
            inner.fill_(OUT_BYTE if kind == "out" else ws_byte)

    def set(self, src):
        self.t.copy_(src.reshape(-1).to(self.t.device))
        return self

    def freeze(self):
        return self

    def data_ptr(self):
        return self.raw.data_ptr() + self.front

    def check(self, name="buffer"):
        pass


class Arena:
    """The buffers of one run of a case: every pointer argument comes from inp() / out() / ws(), call() passes them
    to an srk_* entry point on the current stream, synchronises and checks every buffer made so far (so a forward
    workspace is checked again after the backward).  guarded = False gives the plain run with the same code."""

    def __init__(self, guarded=True, ws_byte=WS_BYTES[0], device="cuda"):
        self.guarded, self.ws_byte, self.device = guarded, ws_byte, torch.device(device)
        self.bufs = []

    def _make(self, name, n, dtype, kind, lead):
        cls = Guarded if self.guarded else Plain
        b = cls(n, dtype, self.device, kind, lead=lead, ws_byte=self.ws_byte)
        self.bufs.append((name, b))
        return b

    def inp(self, name, tensor, lead=0):
        """A const input holding `tensor`'s elements (flattened, contiguous)."""
        t = tensor.contiguous()
        return self._make(name, t.numel(), t.dtype, "in", lead).set(t)

    def out(self, name, n_elems, dtype=torch.float32, init=None, lead=0):
        """An output of n_elems elements; init: the values of an in-out argument (C with beta, .grad, state)."""
        b = self._make(name, n_elems, dtype, "out", lead)
        if init is not None:
            b.set(init.contiguous())
        return b

    def ws(self, name, n_elems, dtype=torch.float32):
        """A caller-sized workspace of exactly n_elems elements, pre-filled with this run's ws_byte."""
        return self._make(name, n_elems, dtype, "ws", 0)

    def check(self):
        for name, b in self.bufs:
            b.check(name)

    def call(self, entry, *args):
        from speechrecognitionproject_amd import _lib
        conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, (Guarded, Plain)) else a for a in args]
        stream = None
        if self.device.type == "cuda":
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.call(entry, *conv, stream)
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        self.check()


def guarded_call(name, spec, guarded=True, ws_byte=WS_BYTES[0], device="cuda"):
    """One entry-point call with every pointer argument in a buffer of its own.  spec: the call's arguments in
    order without the trailing stream; a pointer argument is ("in", tensor[, lead]), ("out", n_elems, dtype[, init
    tensor or None[, lead]]), ("ws", n_elems[, dtype]) or None, everything else is passed as it is.  Calls through
    _lib.call on the current stream, synchronises, runs every check and returns the interiors of the "out" (and
    "ws") arguments in argument order."""
    a = Arena(guarded, ws_byte, device)
    args, outs = [], []
    for i, s in enumerate(spec):
        if isinstance(s, tuple) and s and s[0] in ("in", "out", "ws"):
            tag = "%s arg %d" % (name, i)
            if s[0] == "in":
                args.append(a.inp(tag, s[1], *s[2:]))
            elif s[0] == "out":
                args.append(a.out(tag, s[1], s[2], *s[3:]))
                outs.append(args[-1].t)
            else:
                args.append(a.ws(tag, s[1], *s[2:]))
                outs.append(args[-1].t)
        else:
            args.append(s)
    a.call(name, *args)
    return outs


def same_bits(a, b):
    """Bitwise equality of two tensors of one dtype and size (NaN payloads included)."""
    if a.dtype != b.dtype or a.numel() != b.numel():
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
