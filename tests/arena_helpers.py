"""Guard bands and poison around every device buffer a native entry point is given: the bounds check of the C ABI.

Four parts, none of which holds a kernel or edits product code:

Arena        one allocation filled with a poison byte; a bump allocator hands out bodies of EXACTLY the requested byte count, each
             on a 512-byte boundary (what torch's caching allocator gives, so alignment assumptions hold) with at least 64 KiB of
             poison on either side -- the bytes between a body's exact end and the next boundary are guard too.  Nothing is reused.
             check() synchronises and asserts that every byte outside the bodies still holds the poison; a failure names the nearest
             body and the offset of the first changed byte relative to it (before its start / past its end).
patch()      a context manager (pytest's monkeypatch) that makes the allocation names the wrappers of gscream_amd/ use -- torch.empty,
             zeros, ones, full, their *_like and Tensor.new_* forms, and the copies .to / .cuda / .clone / .contiguous / .float make --
             return views of arena bodies for the arena's device.  empty() leaves the poison in the body; zeros / ones / full fill the
             body only.  Other devices and pinned memory pass through.  Copies are adopted only where autograd does not track them.
header_table the parameter lists gscream_amd/_abi.py reads from include/gsraster.h: {function: [(type, name, is_pointer, is_const)]}.
LibProxy     stands in for _native._lib (both _native.load() and _native.run() go through it).  On every call each non-NULL pointer
             argument declared non-const must lie inside an arena body ("unguarded writable buffer: function, parameter"), and each
             const pointer argument that lies in a body is copied before the call and compared bit for bit after it.  The pointers
             inside the host arrays `weights` / `grads16` are checked the same way.  HOST_PARAMS lists, by (function, parameter) and
             with a reason, the parameters that are host memory; it holds host parameters only, never a workspace, an output or
             anything sized by a *_bytes or capacity formula.

Device pointers inside host struct tables are invisible to a proxy that knows the header alone.  Where the wrappers pass such a
table as a ctypes array of the binding's own structures (gsr_adam_tensor, gsr_adjust_copy, gsr_frame_panel: STRUCT_TABLES) the proxy
reads the pointers out of it and checks them like arguments.  It cannot see gsr_tuning.walk_depths (the struct arrives by reference)
nor what the DEVICE tables of gsr_png_decode (gsr_png_file, gsr_png_piece: offsets into `bytes`, `out` and the workspace) lead to.
Those tensors are covered by the arena's own guard check, provided the test allocated them under patch().  Nor does any of this see
an out-of-bounds READ that changes no output, or a write beyond the 64 KiB guard that lands in another body.
"""
import bisect
import contextlib
import ctypes

import torch

from gscream_amd import _abi

ALIGN = 512
GUARD = 64 * 1024

#: (function, parameter) -> why it is host memory.  ("*", "stream") stands for the `void* stream` every launching entry point ends in.
HOST_PARAMS = {
    ("*", "stream"): "hipStream_t handle, not memory",
    ("gsr_forward_stage1", "result_host"): "gsr_stage1_result in pinned host memory",
    ("gsr_forward", "result_host"): "gsr_stage1_result in pinned host memory",
    ("gsr_forward_stage1", "tuning"): "gsr_tuning struct on the host",
    ("gsr_forward_stage2", "tuning"): "gsr_tuning struct on the host",
    ("gsr_forward", "tuning"): "gsr_tuning struct on the host",
    ("gsr_backward", "tuning"): "gsr_tuning struct on the host",
    ("gsr_profile_end", "out_host"): "gsr_profile struct on the host",
    ("gsr_workspace_layout", "out_host"): "array of gsr_layout_piece on the host: the query runs no kernel and touches no device memory",
    ("gsr_decode_count", "weights"): "host array of 16 device pointers (each checked as const)",
    ("gsr_decode_emit", "weights"): "host array of 16 device pointers (each checked as const)",
    ("gsr_decode_backward", "weights"): "host array of 16 device pointers (each checked as const)",
    ("gsr_decode_backward", "grads16"): "host array of 16 device pointers (each checked as writable)",
    ("gsr_anchor_adjust_gather", "copies"): "host table of gsr_adjust_copy, travels in the kernel arguments",
    ("gsr_adam_step", "tensors"): "host table of gsr_adam_tensor, travels in the kernel arguments",
    ("gsr_frame_compose", "panels"): "host table of gsr_frame_panel, travels in the kernel arguments",
}
#: host struct tables the wrappers pass as ctypes arrays: (function, parameter) -> (the parameter that holds the entry count, the fields
#: that are writable device pointers, the fields that are const device pointers).  Read where the argument is such an array.
STRUCT_TABLES = {("gsr_adam_step", "tensors"): ("n_tensors", ("p", "m", "v"), ("g",)),
                 ("gsr_anchor_adjust_gather", "copies"): ("n_copies", ("dst",), ("src",)),
                 ("gsr_frame_compose", "panels"): ("n", (), ("src", "src2", "lut"))}
#: host arrays of device pointers: (function, parameter) -> (entries, the entries are const)
POINTER_ARRAYS = {("gsr_decode_count", "weights"): (16, True), ("gsr_decode_emit", "weights"): (16, True),
                  ("gsr_decode_backward", "weights"): (16, True), ("gsr_decode_backward", "grads16"): (16, False)}


class GuardError(AssertionError):
    """.kind: 'guard' (a byte outside every body changed), 'unguarded', 'const', 'differ';  .buffer: the body's or output's name;
    .where / .offset: 'before' its start (offset -1 = the byte in front of it), 'past' its end (offset 0 = the first byte behind it), or
    'inside' (offset from its start)."""

    def __init__(self, message, kind=None, buffer=None, where=None, offset=None):
        super().__init__(message)
        self.kind, self.buffer, self.where, self.offset = kind, buffer, where, offset


# ---- the header table ----------------------------------------------------------------------------------------------------------

def header_table():
    """{function: [(type, name, is_pointer, is_const)]} of every function include/gsraster.h declares: the package's own reading."""
    return {name: params for name, (_, params) in _abi.header().functions.items()}


# ---- the arena -----------------------------------------------------------------------------------------------------------------

class Arena:
    def __init__(self, nbytes, poison, device):
        self.device = torch.device(device)
        self.poison = int(poison) & 0xFF
        self.nbytes = (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN
        self.whole = _REAL["full"]((self.nbytes + ALIGN,), self.poison, dtype=torch.uint8, device=self.device)
        skip = -self.whole.data_ptr() % ALIGN  # (host memory comes 64-byte aligned; device memory needs no skip)
        self.skip = skip
        self.buf = self.whole[skip:skip + self.nbytes]
        self.base = self.buf.data_ptr()
        assert self.base % ALIGN == 0, "the arena itself must start on a 512-byte boundary"
        self.cursor = 0
        self.starts, self.sizes, self.names = [], [], []

    # -- allocation
    def alloc_bytes(self, nbytes, name=None, dtype=torch.uint8, shape=None):
        """A fresh body of exactly `nbytes` bytes (still poisoned), as a uint8 tensor or with `dtype` and `shape`.  The tensor shares
        the arena's storage but is no view of it: autograd gives it a version counter of its own, as it does a torch.empty tensor."""
        nbytes = int(nbytes)
        start = (self.cursor + GUARD + ALIGN - 1) // ALIGN * ALIGN
        if start + nbytes + GUARD > self.nbytes:
            raise GuardError(f"arena of {self.nbytes} bytes exhausted by a request of {nbytes} (make the test's arena larger)")
        self.cursor = start + nbytes
        self.starts.append(start)
        self.sizes.append(nbytes)
        self.names.append(name or f"#{len(self.starts) - 1}")
        item = _itemsize(dtype)
        t = _REAL["empty"]((0,), dtype=dtype, device=self.device)
        return t.set_(self.whole.untyped_storage(), (self.skip + start) // item, (nbytes // item,) if shape is None else shape)

    def alloc(self, shape, dtype, name=None):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = _itemsize(dtype)
        if n == 0:
            return _REAL["empty"](shape, dtype=dtype, device=self.device)  # no bytes: nothing to guard (the wrappers pass NULL)
        name = name or f"#{len(self.starts)} {str(dtype).replace('torch.', '')}{list(shape)}"
        return self.alloc_bytes(n * item, name, dtype, shape)

    def put(self, t, name=None):
        """A copy of tensor (or numpy array) `t` in a body of its own."""
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(t)
        out = self.alloc(t.shape, t.dtype, name)
        if out.numel():
            out.copy_(t.detach())
        return out

    # -- lookup
    def body_of(self, address, nbytes=1):
        """Index of the body that holds [address, address + nbytes), or None."""
        off = address - self.base
        i = bisect.bisect_right(self.starts, off) - 1
        if i >= 0 and off + nbytes <= self.starts[i] + self.sizes[i]:
            return i
        return None

    def body_bytes(self, i):
        return self.buf[self.starts[i]:self.starts[i] + self.sizes[i]]

    def owns(self, t):
        return t.numel() == 0 or (t.device.type == self.device.type and self.body_of(t.data_ptr()) is not None)

    # -- the check
    def _gaps(self):
        edges, prev = [], 0
        for s, n in zip(self.starts, self.sizes):
            edges.append((prev, s))
            prev = s + n
        edges.append((prev, self.nbytes))
        return [(a, b) for a, b in edges if b > a]

    def check(self):
        """Synchronise; every byte outside the bodies must still hold the poison."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        gaps = self._gaps()
        flags = torch.stack([(self.buf[a:b] != self.poison).any() for a, b in gaps]).cpu().tolist()
        for (a, b), bad in zip(gaps, flags):
            if bad:
                off = a + int((self.buf[a:b] != self.poison).nonzero()[0, 0])
                raise self.describe(off)

    def describe(self, off):
        """GuardError for the arena offset `off` of a changed guard byte: the nearest body and the offset relative to it."""
        got = int(self.buf[off])
        best = None
        for i, (s, n) in enumerate(zip(self.starts, self.sizes)):
            d, where, rel = (s - off, "before", off - s) if off < s else (off - (s + n) + 1, "past", off - (s + n))
            if best is None or d < best[0]:
                best = (d, where, rel, i)
        tail = f"(0x{got:02x}, poison 0x{self.poison:02x})"
        if best is None:
            return GuardError(f"guard byte changed at arena offset {off} {tail}; no buffer was allocated", "guard")
        _, where, rel, i = best
        text = f"offset {rel} before its start" if where == "before" else f"offset +{rel} past its end"
        return GuardError(f"guard byte changed: buffer {self.names[i]} ({self.sizes[i]} bytes), {text} {tail}", "guard", self.names[i],
                          where, rel)

    def unwritten(self, t):
        """Number of bytes of tensor `t` (a whole arena body or part of one) that still hold the poison byte."""
        return int((t.contiguous().view(torch.uint8) == self.poison).sum())


def _itemsize(dtype):
    return torch.tensor([], dtype=dtype).element_size()


# ---- the allocation patch ------------------------------------------------------------------------------------------------------

_REAL = {name: getattr(torch, name) for name in ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")}
_REAL_T = {name: getattr(torch.Tensor, name) for name in ("new_empty", "new_zeros", "new_ones", "new_full", "to", "cuda", "clone",
                                                             "contiguous", "float")}


def _shape_of(args, kwargs):
    if "size" in kwargs:
        return tuple(kwargs["size"])
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    return tuple(args)


def _finish(t, kwargs):
    if kwargs.get("requires_grad"):
        t.requires_grad_(True)
    return t


@contextlib.contextmanager
def patch(arena, monkeypatch):
    """Route the wrappers' device allocations into `arena` for the duration of the block."""
    kind = arena.device.type

    def mine(device, kwargs=None):
        if kwargs and (kwargs.get("pin_memory") or kwargs.get("out") is not None):
            return False
        if kwargs and kwargs.get("layout", torch.strided) is not torch.strided:
            return False
        if isinstance(device, int):
            return kind == "cuda"
        return device is not None and torch.device(device).type == kind

    def creator(name, fill):
        real = _REAL[name]

        def make(*args, **kwargs):
            device = kwargs.get("device", "cpu")
            if not mine(device, kwargs):
                return real(*args, **kwargs)
            if name == "full":
                shape, value = (kwargs["size"] if "size" in kwargs else args[0]), (kwargs["fill_value"] if "fill_value" in kwargs else args[1])
                dtype = kwargs.get("dtype") or torch.tensor(value).dtype
                t = arena.alloc(tuple(shape), dtype)
                return _finish(t.fill_(value) if t.numel() else t, kwargs)
            t = arena.alloc(_shape_of(args, kwargs), kwargs.get("dtype") or torch.get_default_dtype())
            if fill is not None and t.numel():
                t.fill_(fill)
            return _finish(t, kwargs)
        return make

    def like(name, fill):
        real = _REAL[name]

        def make(src, *args, **kwargs):
            device = kwargs.get("device", src.device)
            if not mine(device, kwargs) or src.layout is not torch.strided:
                return real(src, *args, **kwargs)
            t = arena.alloc(src.shape, kwargs.get("dtype") or src.dtype)
            value = (args[0] if args else kwargs["fill_value"]) if name == "full_like" else fill
            if value is not None and t.numel():
                t.fill_(value)
            return _finish(t, kwargs)
        return make

    def new(name, fill):
        real = _REAL_T[name]

        def make(self, *args, **kwargs):
            device = kwargs.get("device", self.device)
            if not mine(device, kwargs):
                return real(self, *args, **kwargs)
            if name == "new_full":
                shape, value = (kwargs["size"] if "size" in kwargs else args[0]), (kwargs["fill_value"] if "fill_value" in kwargs else args[1])
            else:
                shape, value = _shape_of(args, kwargs), fill
            t = arena.alloc(shape, kwargs.get("dtype") or self.dtype)
            if value is not None and t.numel():
                t.fill_(value)
            return _finish(t, kwargs)
        return make

    def copier(name):
        real = _REAL_T[name]

        def make(self, *args, **kwargs):
            out = real(self, *args, **kwargs)
            # a fresh, dense buffer on the arena's device that autograd does not track: move it into a body of its own
            if (out is not self and isinstance(out, torch.Tensor) and out.device.type == kind and out.layout is torch.strided
                    and out.grad_fn is None and not out.requires_grad and out.numel() and out.is_contiguous()
                    and out.data_ptr() != self.data_ptr() and not arena.owns(out)):
                moved = arena.alloc(out.shape, out.dtype)
                moved.copy_(out)
                return moved
            return out
        return make

    with monkeypatch.context() as m:
        for name, fill in (("empty", None), ("zeros", 0), ("ones", 1), ("full", None)):
            m.setattr(torch, name, creator(name, fill))
        for name, fill in (("empty_like", None), ("zeros_like", 0), ("ones_like", 1), ("full_like", None)):
            m.setattr(torch, name, like(name, fill))
        for name, fill in (("new_empty", None), ("new_zeros", 0), ("new_ones", 1), ("new_full", None)):
            m.setattr(torch.Tensor, name, new(name, fill))
        if kind != "cpu":  # (on the CPU arena of the harness' own tests .to / .clone of ordinary tensors are left alone)
            for name in ("to", "cuda", "clone", "contiguous", "float"):
                m.setattr(torch.Tensor, name, copier(name))
        yield arena


# ---- the library proxy ---------------------------------------------------------------------------------------------------------

def _address(arg):
    """Integer address of a pointer argument as the wrappers pass it (None, int, c_void_p, a ctypes pointer or array), or None."""
    if arg is None:
        return None
    if isinstance(arg, int):
        return arg or None
    if isinstance(arg, ctypes.c_void_p):
        return arg.value
    if isinstance(arg, ctypes.Array):
        return ctypes.addressof(arg)
    if isinstance(arg, ctypes._Pointer):
        return ctypes.cast(arg, ctypes.c_void_p).value
    return None  # byref() objects: host structs


class LibProxy:
    """Checks the pointer arguments of every call against `arena` and the header table, then calls the real function."""

    def __init__(self, lib, arena, table=None, struct_tables=None):
        self._real, self._arena, self._table = lib, arena, table or header_table()
        self._struct_tables = STRUCT_TABLES if struct_tables is None else struct_tables
        self.calls = {}          # function -> number of calls intercepted
        self.guarded = set()     # (function, parameter, body index) of every writable buffer seen
        self._wrapped = {}

    def stats(self):
        return sum(self.calls.values()), len({b for _, _, b in self.guarded}), len(self._arena.starts)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = self._wrapped.get(name)
        if fn is None:
            real = getattr(self._real, name)
            fn = self._wrapped[name] = self._wrap(name, real) if name in self._table else real
        return fn

    def _is_host(self, fn, ctype, pname):
        return (fn, pname) in HOST_PARAMS or (pname == "stream" and ctype == "void*" and ("*", "stream") in HOST_PARAMS)

    def _wrap(self, fn, real):
        params, arena = self._table[fn], self._arena

        def call(*args):
            if len(args) != len(params):
                raise GuardError(f"{fn}: called with {len(args)} arguments, the header declares {len(params)}")
            self.calls[fn] = self.calls.get(fn, 0) + 1
            writable, const = [], []  # (parameter, address)
            for (ctype, pname, is_ptr, is_const), arg in zip(params, args):
                if not is_ptr:
                    continue
                if (fn, pname) in POINTER_ARRAYS:
                    n, inner_const = POINTER_ARRAYS[(fn, pname)]
                    for k in range(n):
                        a = arg[k]
                        a = a.value if isinstance(a, ctypes.c_void_p) else a
                        if a:
                            (const if inner_const else writable).append((f"{pname}[{k}]", int(a)))
                    continue
                if (fn, pname) in self._struct_tables and isinstance(arg, ctypes.Array):
                    count, w_fields, c_fields = self._struct_tables[(fn, pname)]
                    n = int(args[[p[1] for p in params].index(count)])
                    for k in range(min(n, len(arg))):
                        for fields, into in ((w_fields, writable), (c_fields, const)):
                            for f in fields:
                                a = getattr(arg[k], f)
                                if a:
                                    into.append((f"{pname}[{k}].{f}", int(a)))
                    continue
                if self._is_host(fn, ctype, pname):
                    continue
                a = _address(arg)
                if a is None:
                    if arg is not None and not isinstance(arg, (int, ctypes.c_void_p)):
                        raise GuardError(f"{fn}: {pname}: a device pointer passed as {type(arg).__name__}")
                    continue
                (const if is_const else writable).append((pname, a))
            written = set()
            for pname, a in writable:
                b = arena.body_of(a)
                if b is None:
                    raise GuardError(f"unguarded writable buffer: {fn}, {pname}", "unguarded", pname)
                written.add(b)
                self.guarded.add((fn, pname, b))
            before = {}
            for pname, a in const:
                b = arena.body_of(a)
                if b is not None and b not in written and b not in before:
                    before[b] = (pname, _REAL_T["clone"](arena.body_bytes(b)))
            rc = real(*args)
            for b, (pname, snap) in before.items():
                now = arena.body_bytes(b)
                if not torch.equal(now, snap):
                    off = int((now != snap).nonzero()[0, 0])
                    raise GuardError(f"const input changed: {fn}, {pname}: buffer {arena.names[b]}, first changed byte at offset {off}",
                                     "const", pname, "inside", off)
            return rc
        return call


@contextlib.contextmanager
def guarded(monkeypatch, nbytes, poison, device="cuda"):
    """`with guarded(monkeypatch, bytes, poison) as (arena, proxy):` -- the allocation patch and the library proxy together; on a clean
    exit the arena is checked."""
    from gscream_amd import _native
    lib = _native.load()
    arena = Arena(nbytes, poison, device)
    proxy = LibProxy(lib, arena)
    with monkeypatch.context() as m:
        m.setattr(_native, "_lib", proxy)
        with patch(arena, monkeypatch):
            yield arena, proxy
    arena.check()


def assert_same_bits(runs, what=""):
    """runs: {run name: {output name: tensor or array}}.  Every run must hold the same outputs with the same bytes; the failure names
    the output and the byte offset of the first difference."""
    import numpy as np
    names = list(runs)
    as_bytes = lambda v: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).reshape(-1).view(np.uint8)
    first = runs[names[0]]
    for other in names[1:]:
        got = runs[other]
        if sorted(first) != sorted(got):
            raise GuardError(f"{what}: runs {names[0]} and {other} return different outputs: {sorted(first)} / {sorted(got)}", "differ")
        for key in first:
            a, b = first[key], got[key]
            if a is None and b is None:
                continue
            if a is None or b is None or tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
                raise GuardError(f"{what}: {key}: runs {names[0]} and {other} differ in shape or type", "differ", key)
            a, b = as_bytes(a), as_bytes(b)
            if not np.array_equal(a, b):
                off = int(np.flatnonzero(a != b)[0])
                raise GuardError(f"{what}: {key}: runs {names[0]} and {other} differ, first at byte offset {off} "
                                 f"(0x{a[off]:02x} / 0x{b[off]:02x})", "differ", key, "inside", off)
