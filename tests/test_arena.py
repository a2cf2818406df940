"""The guard harness of tests/arena_helpers.py, held against a fake "library" on CPU tensors: every kind of failure it exists to
find is injected once and must be reported with the right buffer and offset, and a clean call must pass.  The fake functions take
the same kind of pointer arguments as the C ABI (integer addresses) and act on the arena through torch indexing."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena_helpers as A  # noqa: E402
from gscream_amd import _native  # noqa: E402

# the fake ABI, in the header's terms: rows of 3 floats, dst[r] = 2 * src[r]
FAKE_TABLE = {"fake_rows": [("int", "n", False, False), ("const float*", "src", True, True), ("float*", "dst", True, False),
                            ("void*", "workspace", True, False), ("void*", "stream", True, False)]}


class FakeLib:
    """fake_rows with one defect switched on by `bug`."""

    def __init__(self, arena, bug=None):
        self.arena, self.bug = arena, bug

    def _floats(self, address, n):
        off = (address.value if isinstance(address, ctypes.c_void_p) else address) - self.arena.base
        return self.arena.buf[off:off + 4 * n].view(torch.float32)

    def fake_rows(self, n, src, dst, workspace, stream):
        a, bug = self.arena, self.bug
        s, d = self._floats(src, 3 * n).view(n, 3), self._floats(dst, 3 * n).view(n, 3)
        rows = [r for r in range(n) if not (bug == "skip_row" and r == 2)]
        d[rows] = 2 * s[rows]
        off = (dst.value if isinstance(dst, ctypes.c_void_p) else dst) - a.base
        if bug == "past":
            a.buf[off + 12 * n] = 0
        if bug == "before":
            a.buf[off - 1] = 0
        if bug == "float4_tail":  # every row stored as four floats: the last row's fourth lands behind the body
            a.buf[off + 12 * n:off + 12 * n + 4] = 0
        if bug == "touch_input":
            s[1, 1] += 1
        if bug == "reads_workspace":  # adds what it finds in the workspace without having written it
            d[0, 0] += self._floats(workspace, 1)[0].nan_to_num(1.0)
        return 0


def _run(monkeypatch, bug=None, poison=0xA5, n=5, outside=False):
    """One guarded call of the fake library -> (outputs, arena, proxy).  Raises what the harness raises."""
    arena = A.Arena(1 << 20, poison, "cpu")
    proxy = A.LibProxy(FakeLib(arena, bug), arena, FAKE_TABLE)
    with A.patch(arena, monkeypatch):
        src = arena.put(torch.arange(3 * n, dtype=torch.float32).view(n, 3), "src")
        dst = A._REAL["empty"]((n, 3)) if outside else arena.alloc((n, 3), torch.float32, "dst")
        ws = torch.empty(64, dtype=torch.uint8)
        assert arena.owns(ws), "torch.empty under the patch comes from the arena"
        rc = proxy.fake_rows(n, src.data_ptr(), ctypes.c_void_p(dst.data_ptr()), ws.data_ptr(), None)
    assert rc == 0
    arena.check()
    return {"dst": dst.clone()}, arena, proxy


def test_clean_call_passes(monkeypatch):
    runs = {}
    for poison in (0xA5, 0xFF):
        out, arena, proxy = _run(monkeypatch, poison=poison)
        runs[hex(poison)] = out
        assert torch.equal(out["dst"], 2 * torch.arange(15, dtype=torch.float32).view(5, 3))
        calls, guarded, bodies = proxy.stats()
        assert (calls, guarded, bodies) == (1, 2, 3) and proxy.calls == {"fake_rows": 1}
    A.assert_same_bits(runs, "fake_rows")
    assert torch.empty is A._REAL["empty"] and torch.Tensor.new_empty is A._REAL_T["new_empty"], "the patch is undone"


def test_one_byte_past_a_body(monkeypatch):
    with pytest.raises(A.GuardError, match="guard byte changed: buffer dst") as e:
        _run(monkeypatch, "past")
    assert (e.value.kind, e.value.buffer, e.value.where, e.value.offset) == ("guard", "dst", "past", 0)


def test_one_byte_before_a_body(monkeypatch):
    with pytest.raises(A.GuardError, match="before its start") as e:
        _run(monkeypatch, "before")
    assert (e.value.kind, e.value.buffer, e.value.where, e.value.offset) == ("guard", "dst", "before", -1)


@pytest.mark.parametrize("n", [5, 128])  # 60 bytes: the store lands in the slack before the next boundary; 1536: on the boundary
def test_float4_store_over_a_3_float_row(monkeypatch, n):
    with pytest.raises(A.GuardError, match="past its end") as e:
        _run(monkeypatch, "float4_tail", n=n)
    assert (e.value.buffer, e.value.where, e.value.offset) == ("dst", "past", 0)


def test_const_input_changed(monkeypatch):
    with pytest.raises(A.GuardError, match="const input changed: fake_rows, src") as e:
        _run(monkeypatch, "touch_input")
    assert (e.value.kind, e.value.buffer, e.value.where) == ("const", "src", "inside")
    assert e.value.offset // 4 == 4  # element [1, 1]


def test_writable_pointer_outside_the_arena(monkeypatch):
    with pytest.raises(A.GuardError, match="unguarded writable buffer: fake_rows, dst") as e:
        _run(monkeypatch, outside=True)
    assert (e.value.kind, e.value.buffer) == ("unguarded", "dst")


class FakeEntry(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int32)]


def test_pointers_inside_a_host_struct_table(monkeypatch):
    """A host table passed as a ctypes array: its writable pointers must lie in bodies, its const ones are compared."""
    table = {"fake_table": [("int", "n", False, False), ("const fake_entry*", "entries", True, True), ("void*", "stream", True, False)]}
    tables = {("fake_table", "entries"): ("n", ("dst",), ("src",))}
    arena = A.Arena(1 << 20, 0xA5, "cpu")
    spoil = []

    class Lib:
        def fake_table(self, n, entries, stream):
            for e in entries[:n]:
                if spoil:
                    arena.buf[e.src - arena.base] ^= 1
            return 0
    proxy = A.LibProxy(Lib(), arena, table, tables)
    src, dst = arena.put(torch.arange(4.0), "src"), arena.alloc((4,), torch.float32, "dst")
    outside = A._REAL["empty"](4)
    good = (FakeEntry * 2)(FakeEntry(src.data_ptr(), dst.data_ptr(), 4), FakeEntry(None, None, 0))
    assert proxy.fake_table(2, good, None) == 0 and proxy.stats()[:2] == (1, 1)
    bad = (FakeEntry * 2)(FakeEntry(src.data_ptr(), dst.data_ptr(), 4), FakeEntry(src.data_ptr(), outside.data_ptr(), 4))
    with pytest.raises(A.GuardError, match=r"unguarded writable buffer: fake_table, entries\[1\].dst"):
        proxy.fake_table(2, bad, None)
    assert proxy.fake_table(1, bad, None) == 0, "entries beyond the count are not read"
    spoil.append(1)
    with pytest.raises(A.GuardError, match=r"const input changed: fake_table, entries\[0\].src") as e:
        proxy.fake_table(1, good, None)
    assert (e.value.kind, e.value.offset) == ("const", 0)


def test_output_row_left_unwritten(monkeypatch):
    runs = {hex(p): _run(monkeypatch, "skip_row", poison=p)[0] for p in (0xA5, 0xFF)}
    with pytest.raises(A.GuardError, match="dst: runs 0xa5 and 0xff differ") as e:
        A.assert_same_bits(runs, "fake_rows")
    assert (e.value.kind, e.value.buffer, e.value.offset) == ("differ", "dst", 2 * 12)  # row 2, its first byte
    out, arena, _ = _run(monkeypatch, "skip_row")
    assert arena.unwritten(out["dst"]) >= 12 and arena.unwritten(_run(monkeypatch)[0]["dst"]) == 0


def test_output_depends_on_workspace_content(monkeypatch):
    runs = {hex(p): _run(monkeypatch, "reads_workspace", poison=p)[0] for p in (0xA5, 0xFF)}
    with pytest.raises(A.GuardError, match="dst: runs 0xa5 and 0xff differ") as e:
        A.assert_same_bits(runs, "fake_rows")
    assert (e.value.buffer, e.value.offset // 4) == ("dst", 0)


def test_bodies_are_exact_aligned_and_apart(monkeypatch):
    arena = A.Arena(1 << 20, 0xA5, "cpu")
    with A.patch(arena, monkeypatch):
        a = torch.empty(7, dtype=torch.uint8)
        b = torch.zeros((3, 5), dtype=torch.float32)
        c = torch.full((9,), -3, dtype=torch.int32)
        d = torch.ones(2, dtype=torch.float64)
        e = torch.zeros_like(b)
        f = b.new_empty((4,))
        g = torch.full_like(c, 7)
        z = torch.empty((0, 3))
        pinned_like = torch.empty(3, device="meta")  # another device passes through
    assert pinned_like.device.type == "meta" and z.numel() == 0 and len(arena.starts) == 7
    assert arena.sizes == [7, 60, 36, 16, 60, 16, 36]
    for s in arena.starts:
        assert s % A.ALIGN == 0 and (arena.base + s) % A.ALIGN == 0
    for (s0, n0), s1 in zip(zip(arena.starts, arena.sizes), arena.starts[1:]):
        assert s1 - (s0 + n0) >= A.GUARD
    assert arena.starts[0] >= A.GUARD and arena.nbytes - arena.cursor >= A.GUARD
    # empty keeps the poison; zeros / ones / full hold their values; every guard byte is still poison
    assert (a == 0xA5).all() and (f.view(torch.uint8) == 0xA5).all()
    assert not b.any() and not e.any() and (c == -3).all() and (d == 1).all() and (g == 7).all()
    assert f.dtype is torch.float32 and c.dtype is torch.int32 and g.shape == c.shape
    arena.check()
    assert int((arena.buf != 0xA5).sum()) == 60 + 36 + 16 + 60 + 36
    assert arena.body_of(b.data_ptr()) == 1 and arena.body_of(b.data_ptr() + 59) == 1 and arena.body_of(b.data_ptr() + 60) is None


def test_bodies_are_tensors_of_their_own_for_autograd(monkeypatch):
    """A write into one body must not invalidate what autograd saved of another: bodies share storage, not a version counter."""
    arena = A.Arena(1 << 20, 0xFF, "cpu")
    with A.patch(arena, monkeypatch):
        x = torch.ones(4, requires_grad=True)
        other, scalar = torch.empty(4), torch.empty((), dtype=torch.float64)
        y = (x * x).sum()
        before = x._version
        other.fill_(2.0)
        scalar.fill_(3.0)
        y.backward()
    assert x.grad.tolist() == [2.0] * 4 and x._base is None and x._version == before and float(scalar) == 3.0
    arena.check()


def test_header_table_covers_the_exported_symbols():
    table = A.header_table()
    assert sorted(table) == sorted(_native.EXPORTED_SYMBOLS)
    assert table["gsr_version"] == [] and len(table["gsr_backward"]) == 41
    assert ("float* const*", "grads16", True, False) in table["gsr_decode_backward"]
    assert ("const gsr_tuning*", "tuning", True, True) in table["gsr_forward"]
    assert ("size_t", "out_stride", False, False) in table["gsr_png_encode"]


def test_exception_list_holds_host_parameters_only():
    """Every entry names a declared parameter; none is a workspace, an output buffer or anything a *_bytes / capacity formula sizes."""
    table = A.header_table()
    device_words = ("workspace", "scratch", "geom", "image", "binning", "out", "radii", "dL_", "d_", "block_scratch")
    for (fn, pname), reason in A.HOST_PARAMS.items():
        assert reason
        if fn == "*":
            assert pname == "stream"
            continue
        assert pname in [p[1] for p in table[fn]], (fn, pname)
        assert pname in ("result_host", "out_host", "tuning", "weights", "grads16", "copies", "tensors", "panels"), (fn, pname)
        assert not any(pname.startswith(w) for w in device_words if w != "out") and pname not in device_words
    for key in A.POINTER_ARRAYS:
        assert key in A.HOST_PARAMS
