"""CPU tests of the workspace layouts: every size query of the built library returns, to the byte, what
tests/golden/workspace_sizes.json records (tools/record_workspace_sizes.py wrote it from the commit before the layouts moved
onto gscream_amd/csrc/gsr_carve.h); the carver itself, compiled into tests/carve_check.cpp with AddressSanitizer and UBSan
and run as a child process (nothing is loaded into Python under a sanitizer); gsr_png_decode's workspace check, which is
the size of the tables as the launcher lays them out; and where the pieces of the rasterizer's four workspaces lie: what
gscream_amd/_layout.py shows is what tests/golden/workspace_layouts.json records (tools/record_workspace_layouts.py wrote it with
the hand-written _layout.py of the commit before the library answered the question), and what gsr_workspace_layout reports is
ordered, aligned, apart and as large as the size query says."""
import ctypes
import json
import os
import subprocess

import pytest

from gscream_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as _f:
    GOLDEN = json.load(_f)
with open(os.path.join(ROOT, "tests", "golden", "workspace_layouts.json")) as _f:
    LAYOUTS = json.load(_f)


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_golden_file_covers_the_grid():
    tool = _tool("record_workspace_sizes")
    assert {q: [list(a) for a in args] for q, args in tool.grid().items()} == {q: [a for a, _ in rows] for q, rows in GOLDEN.items()}


def test_every_size_query_is_exported_and_recorded(native_lib):
    from gscream_amd import _native
    queries = {s for s in _native.EXPORTED_SYMBOLS if s.endswith("_bytes") or s.endswith("_capacity")}
    assert queries == set(GOLDEN)


@pytest.mark.parametrize("query", sorted(GOLDEN))
def test_size_query_returns_the_recorded_bytes(native_lib, query):
    fn = getattr(native_lib, query)
    got = [[args, int(fn(*args))] for args, _ in GOLDEN[query]]
    assert got == GOLDEN[query]
    assert any(b == 0 for _, b in got) or query in ("gsr_geom_bytes", "gsr_binning_bytes", "gsr_image_bytes", "gsr_backward_scratch_bytes",
                                                     "gsr_loss_workspace_bytes", "gsr_knn_workspace_bytes", "gsr_depth_loss_workspace_bytes",
                                                     "gsr_decode_weight_grad_workspace_bytes")  # (these reject nothing)


def test_the_layout_file_covers_the_grid():
    tool = _tool("record_workspace_layouts")
    assert {w: [list(a) for a in args] for w, args in tool.grid().items()} == {w: [a for a, _ in LAYOUTS[w]] for w in ("geom", "image", "binning")}
    assert [t for t, _, _ in LAYOUTS["xcd"]] == list(tool.TILE_COUNTS) and [p for p, _ in LAYOUTS["num_chunks"]] == list(tool.CHUNK_COUNTS)
    assert sorted(LAYOUTS["ckpt_pos"]) == sorted(str(L) for L in tool.SEG_LENGTHS)


def test_layout_views_are_the_recorded_ones(native_lib):
    """Every offset, dtype and shape _layout shows on meta buffers of the library's own sizes, its four constants and its position
    formulas: exactly what the hand-written layout of the recording commit gave, over the whole grid."""
    got = _tool("record_workspace_layouts").record()
    assert sorted(got) == sorted(LAYOUTS)
    for part in LAYOUTS:
        assert got[part] == LAYOUTS[part], part


def _pieces(lib, which, P=0, W=0, H=0, R=0, capacity=64):
    out = (_native.LayoutPiece * capacity)()
    n = lib.gsr_workspace_layout(_native._ABI.constants["GSR_LAYOUT_" + which], P, W, H, R, out, capacity)
    assert 0 < n <= capacity, lib.gsr_last_error()
    return [(ctypes.string_at(p.name).decode(), p.offset, p.count * p.elem_size) for p in out[:n]]


WORKSPACES = {"GEOM": ("gsr_geom_bytes", ("P",), ()), "IMAGE": ("gsr_image_bytes", ("P", "W", "H"), ("ckpt", "occ_mass")),
              "BINNING": ("gsr_binning_bytes", ("R",), ()), "BACKWARD_SCRATCH": ("gsr_backward_scratch_bytes", ("P", "R"), ())}


@pytest.mark.parametrize("which", sorted(WORKSPACES))
def test_layout_query_pieces_are_ordered_aligned_apart_and_fill_the_size(native_lib, which):
    """Over the recorded grid of the workspace's size query (the sizes it accepts): pieces in ascending offset order, each on a
    multiple of 256, no two overlapping but the declared ckpt / occ_mass pair, the last one ending in the final 256 bytes of
    gsr_*_bytes, and the same names in the same order whatever the sizes."""
    query, params, shared = WORKSPACES[which]
    names = None
    cases = [args for args, nbytes in GOLDEN[query] if nbytes and min(args) >= 0]
    assert len(cases) >= 8
    for args in cases:
        pieces = _pieces(native_lib, which, **dict(zip(params, args)))
        assert names in (None, [n for n, _, _ in pieces]), args
        names = [n for n, _, _ in pieces]
        offsets = [o for _, o, _ in pieces]
        assert offsets == sorted(offsets) and all(o % 256 == 0 for o in offsets), args
        for i, (a, a_off, a_bytes) in enumerate(pieces):
            for b, b_off, _ in pieces[i + 1:]:
                assert a_off + a_bytes <= b_off or (a, b) == shared and a_off == b_off, (args, a, b)
        end = max(o + n for _, o, n in pieces)
        total = getattr(native_lib, query)(*args)
        assert pieces[-1][1] + pieces[-1][2] == end and 0 <= total - end < 256, (args, end, total)
    assert len(set(names)) == len(names) and set(shared) <= set(names)


def test_layout_query_counts_past_a_short_array_and_refuses_an_unknown_workspace(native_lib):
    which = _native._ABI.constants["GSR_LAYOUT_IMAGE"]
    full = _pieces(native_lib, "IMAGE", P=5000, W=112, H=71)
    assert native_lib.gsr_workspace_layout(which, 5000, 112, 71, 0, None, 0) == len(full) > 8
    out = (_native.LayoutPiece * 8)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    assert native_lib.gsr_workspace_layout(which, 5000, 112, 71, 0, out, 3) == len(full)
    assert [(ctypes.string_at(p.name).decode(), p.offset) for p in out[:3]] == [(n, o) for n, o, _ in full[:3]]
    assert bytes(out)[3 * ctypes.sizeof(_native.LayoutPiece):] == b"\xa5" * (5 * ctypes.sizeof(_native.LayoutPiece)), "written past the capacity"
    for bad in (-1, 4, 1000):
        assert native_lib.gsr_workspace_layout(bad, 1, 16, 16, 1, out, 8) == -1 and b"unknown workspace" in native_lib.gsr_last_error()
    assert native_lib.gsr_workspace_layout(which, 1, 16, 16, 1, None, 8) == -1 and b"out_host" in native_lib.gsr_last_error()
    assert native_lib.gsr_layout_constant(99) == -1 and b"unknown constant" in native_lib.gsr_last_error()


def test_layout_view_refuses_a_dtype_that_is_not_the_piece(native_lib, monkeypatch):
    """A view whose dtype x width is not the library's element size raises; it never reinterprets."""
    import torch
    from gscream_amd import _layout
    buf = torch.empty(native_lib.gsr_geom_bytes(3), dtype=torch.uint8, device="meta")
    monkeypatch.setitem(_layout._GEOM, "rect", ("rect", torch.int32, 1))
    with pytest.raises(TypeError, match="rect"):
        _layout.geom_views(buf, 3)


def test_carver_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "carve_check")
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")  # the host compiler hipcc itself runs
    subprocess.run([cxx, "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    os.path.join(ROOT, "tests", "carve_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("carve_check OK")


def test_png_decode_rejects_a_workspace_between_the_unrounded_and_the_rounded_tables(native_lib):
    """One file, one piece: the tables are 12 + 4 bytes, each rounded up to 16 by the layout = 32.  20 bytes held the unrounded
    sum the argument check used to compare with, and the launcher then refused the call as a HIP error."""
    assert native_lib.gsr_png_decode_workspace_bytes(0, 1, 1) == 32
    raw = (ctypes.c_uint8 * 256)()
    buf = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    for workspace_bytes in (16, 20, 31):
        rc = native_lib.gsr_png_decode(buf, 64, buf, 1, buf, 1, 1, buf, 64, buf, buf, workspace_bytes, None)
        assert rc == -1 and b"below the tables' part alone" in native_lib.gsr_last_error(), workspace_bytes
