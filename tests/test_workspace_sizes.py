"""CPU tests of the workspace layouts: every size query of the built library returns, to the byte, what
tests/golden/workspace_sizes.json records (tools/record_workspace_sizes.py wrote it from the commit before the layouts moved
onto gscream_amd/csrc/gsr_carve.h); the carver itself, compiled into tests/carve_check.cpp with AddressSanitizer and UBSan
and run as a child process (nothing is loaded into Python under a sanitizer); and gsr_png_decode's workspace check, which is
the size of the tables as the launcher lays them out."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_covers_the_grid():
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_workspace_sizes", os.path.join(ROOT, "tools", "record_workspace_sizes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
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
