"""gscream_amd.frames without a GPU: the numpy oracle of tests/frames_helpers.py against matplotlib's stored imsave bytes, the fit against
the stored runs of the reference's compute_scale_and_shift, the torch path against the oracle byte for byte, the colour tables, the
agreement of header, binding and library, and everything the two C calls and the Python layer reject before anything is launched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import frames_helpers as O  # noqa: E402

from gscream_amd import frames as Fr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_frames.npz")
FITS = ("slanted", "inverse", "empty")


def t(a):
    return torch.from_numpy(np.array(a))


def viridis():
    return Fr.colormap_lut("viridis").numpy()


def inferno():
    return Fr.colormap_lut("inferno").numpy()


# ---- what is pinned ----
@pytest.mark.parametrize("name", FITS + ("constant", "nan"))
def test_the_oracle_gives_the_stored_imsave_bytes(name):
    z = np.load(GOLDEN)
    assert tuple(z["cases"]) == FITS and z["versions"][0].startswith("matplotlib ") and z["versions"][1].startswith("numpy ")
    panel, want = z[f"{name}/panel"], z[f"{name}/imsave"]
    assert panel.dtype == np.float32 and want.dtype == np.uint8 and want.shape == panel.shape + (4,)
    got = O.cmap_mpl(panel, *O.extrema(panel), viridis())
    assert np.array_equal(got, want), f"{(got != want).any(-1).sum()} pixels differ"
    if name == "nan":
        assert (want == 0).all()
    if name == "constant":
        assert (want == np.append(viridis()[0], 255)).all()


@pytest.mark.parametrize("name", FITS)
def test_the_stored_panel_is_the_rule_on_the_references_fit(name):
    """render_set's depth * |scale| + shift in fp32 is the `aligned` rule; the torch path's MPL panels on it are imsave's bytes."""
    z = np.load(GOLDEN)
    d, y = z[f"{name}/depth"], z[f"{name}/target"]
    scale, shift = np.abs(z[f"{name}/scale32"][0]), z[f"{name}/shift32"][0]
    w = d.shape[2]
    assert np.array_equal(O.aligned(d[0], scale, shift), z[f"{name}/panel"][:, :w]) and np.array_equal(y[0], z[f"{name}/panel"][:, w:])
    lo2, hi2 = O.extrema(z[f"{name}/panel"])
    params = t(np.array([[0, 0, scale, shift, lo2, hi2, 0, 0], ], np.float32))
    lut = Fr.colormap_lut("viridis")
    got = Fr.compose([Fr.Panel(Fr.CMAP_MPL_ALIGNED, t(d)[None], lut=lut), Fr.Panel(Fr.CMAP_MPL, t(y)[None], lut=lut)], channels=4, params=params)
    assert Fr.last_path == "torch" and np.array_equal(got[0].numpy(), z[f"{name}/imsave"])


@pytest.mark.parametrize("name", FITS)
def test_scale_and_shift_against_the_stored_reference_runs(name):
    """S = the reference's fp64 run.  The reference's fp32 run is off S by its fp32 sums; the package is held to be no further off."""
    z = np.load(GOLDEN)
    d, y, m = (t(z[f"{name}/{k}"]) for k in ("depth", "target", "mask"))
    stats, params = Fr.frame_stats(d, y, m)
    assert Fr.last_path == "torch" and stats.dtype == torch.float64 and params.dtype == torch.float32 and tuple(params.shape) == (1, 8)
    o = O.frame_params(d[0].numpy(), y[0].numpy(), m[0].numpy())
    for k, got, key in ((0, float(params[0, 2]), "scale"), (1, float(params[0, 3]), "shift")):
        s64, s32 = float(z[f"{name}/{key}64"][0]), float(z[f"{name}/{key}32"][0])
        if key == "scale":
            s64, s32 = abs(s64), abs(s32)
        got_off, ref_off, oracle_off = abs(got - s64), abs(s32 - s64), abs(float(o["params"][2 + k]) - s64)
        print(f"{name} {key}: fp64 {s64:.17g}; the reference's fp32 run off by {ref_off:.3g}, the torch path by {got_off:.3g}, the oracle by {oracle_off:.3g}")
        assert got_off <= ref_off and oracle_off <= ref_off
    if name == "inverse":
        assert float(stats[0, 6]) < 0 < float(params[0, 2])
    if name == "empty":
        assert float(stats[0, 5]) == 0 and (params[0, 2:4] == 0).all() and float(params[0, 4]) == min(0.0, float(y.min()))


# ---- the torch path against the oracle ----
def edge_image():
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    rng = np.random.default_rng(5)
    x = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1)),
                        np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.7, -0.3, 1e-9, 3e38, -3e38]),
                        (rng.random(3 * 19 * 23, dtype=np.float32) * 1.6 - 0.3)])[:3 * 19 * 23]
    return rng.permutation(x).astype(np.float32).reshape(3, 19, 23)


def test_quantise_edge_values():
    x = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.75 / 255, 0.25 / 255, 254.75 / 255, 2.0, -1.0])
    want = np.uint8([0, 255, 0, 0, 0, 255, 1, 0, 255, 255, 0])
    assert np.array_equal(O.quantise(x), want)
    assert np.array_equal(Fr._quantise_torch(t(x)).numpy(), want)
    assert np.array_equal(O.quantise(x, clamp=True), want)  # the clamp keeps the NaN, which then becomes 0
    assert np.array_equal(O.clamp01(x), torch.clamp(t(x), 0.0, 1.0).numpy(), equal_nan=True)


def test_to_uint8_equals_the_oracle_and_save_image_writes_it(tmp_path):
    from PIL import Image
    x = edge_image()
    for clamp in (False, True):
        got = Fr.to_uint8(t(x), clamp=clamp)
        assert Fr.last_path == "torch" and got.dtype == torch.uint8 and tuple(got.shape) == (19, 23, 3)
        assert np.array_equal(got.numpy(), O.quantise(x, clamp).transpose(1, 2, 0))
    one = Fr.to_uint8(t(x[:1]))  # make_grid's one-channel expansion
    assert tuple(one.shape) == (19, 23, 3) and np.array_equal(one.numpy(), np.repeat(O.quantise(x[:1]).transpose(1, 2, 0), 3, 2))
    batch = Fr.to_uint8(t(np.stack([x, x[::-1]])))
    assert tuple(batch.shape) == (2, 19, 23, 3) and np.array_equal(batch[1].numpy(), O.quantise(x[::-1]).transpose(1, 2, 0))
    with pytest.raises(ValueError):
        Fr.to_uint8(t(x[:2]))
    path = str(tmp_path / "x.png")
    Fr.save_image(t(x), path)
    assert np.array_equal(np.array(Image.open(path)), O.quantise(x).transpose(1, 2, 0))


def params_agree(params, o):
    """lo, hi, lo2, hi2 bit for bit (the torch path forms aligned from its own scale / shift: compared when those agree), scale and shift
    to one fp32 ulp of the fp64 quotients."""
    p = params.numpy()[0]
    assert np.array_equal(p[:2], o["params"][:2], equal_nan=True) and (p[6:] == 0).all()
    assert O.within_one_ulp(p[2], abs(o["x0"])) and O.within_one_ulp(p[3], o["x1"])
    if np.array_equal(p[2:4], o["params"][2:4]):
        assert np.array_equal(p[4:6], o["params"][4:6], equal_nan=True)


@pytest.mark.parametrize("flip", [True, False])
def test_rgbd_frame_equals_the_oracle(flip):
    H, W = 13, 18
    v = O.view_inputs(H, W, 3)
    _stats, params = Fr.frame_stats(t(v["depth"]))
    params_agree(params, O.frame_params(v["depth"][0]))
    want = O.rgbd_oracle(v, params.numpy(), inferno(), flip)
    rows = t(v["normals"])
    as_returned = rows.view(1, W, H, 3).permute(0, 3, 1, 2)  # what least_square_normal_regress_fast01 returns
    for normal in (rows, as_returned):
        got = Fr.rgbd_frame(t(v["render"]), t(v["depth"]), t(v["uncertainty"]), normal, flip=flip)
        assert Fr.last_path == "torch" and got.dtype == torch.uint8 and tuple(got.shape) == (H, 4 * W, 3)
        assert np.array_equal(got.numpy(), want), f"{(got.numpy() != want).any(-1).sum()} pixels differ"
    # the finished picture of normals.normal_map is quantised as it is
    picture = np.random.default_rng(1).random((3, H, W), dtype=np.float32)
    f = Fr.rgbd_frame(t(v["render"]), t(v["depth"]), t(v["uncertainty"]), t(picture), flip=flip, panels=True)
    q = O.quantise(picture).transpose(1, 2, 0)
    assert np.array_equal(f.normal.numpy(), q[:, ::-1] if flip else q)
    assert all(p.data_ptr() == f.rgbd.data_ptr() + 3 * W * k and tuple(p.shape) == (H, W, 3) for k, p in enumerate(f[1:]))
    assert np.array_equal(f.depth.numpy(), want[:, W:2 * W]) and np.array_equal(f.uncertainty.numpy(), want[:, 3 * W:])
    with pytest.raises(ValueError):
        Fr.rgbd_frame(t(v["render"]), t(v["depth"]), t(v["uncertainty"]), rows[:-1])


def test_the_cv_map_on_edge_frames():
    lut = inferno()
    flat = np.full((1, 4, 5), 2.5, np.float32)
    got = Fr.rgbd_frame(torch.zeros(3, 4, 5), t(flat), torch.zeros(1, 4, 5), torch.zeros(20, 3), panels=True)
    assert (got.depth.numpy() == lut[0]).all() and (got.normal.numpy() == 128).all()  # a zero normal: (0 / 1e-12 + 1) / 2
    bad = np.arange(20, dtype=np.float32).reshape(1, 4, 5)
    bad[0, 1, 2] = np.nan
    got = Fr.rgbd_frame(torch.zeros(3, 4, 5), t(bad), torch.zeros(1, 4, 5), torch.zeros(20, 3), panels=True)
    assert (got.depth.numpy() == lut[0]).all()
    ramp = np.arange(20, dtype=np.float32).reshape(1, 4, 5)
    got = Fr.rgbd_frame(torch.zeros(3, 4, 5), t(ramp), torch.zeros(1, 4, 5), torch.zeros(20, 3), flip=False, panels=True)
    idx = (255 * ((ramp[0] - 0) / np.float32(19))).astype(np.uint8)
    assert idx[0, 0] == 0 and idx[-1, -1] == 255 and np.array_equal(got.depth.numpy(), lut[idx])


def test_view_frames_equals_the_oracle():
    H, W = 13, 18
    v = O.view_inputs(H, W, 4)
    f = Fr.view_frames(*(t(v[k]) for k in ("render", "uncertainty", "gt", "depth", "midas", "mask")))
    assert Fr.last_path == "torch"
    params_agree(f.params, O.frame_params(v["depth"][0], v["midas"][0], 1 - v["mask"][0]))
    sheet, picture = O.view_oracle(v, f.params.numpy(), viridis())
    assert tuple(f.sheet.shape) == (H, 4 * W, 3) and tuple(f.depth.shape) == (H, 2 * W, 4) and f.depth.dtype == torch.uint8
    assert np.array_equal(f.sheet.numpy(), sheet) and np.array_equal(f.depth.numpy(), picture)
    for k, name in enumerate(("render", "uncertainty", "error", "gt")):
        p = getattr(f, name)
        assert p.data_ptr() == f.sheet.data_ptr() + 3 * W * k and np.array_equal(p.numpy(), sheet[:, k * W:(k + 1) * W])
    assert np.array_equal(f.error.numpy(), O.absdiff(v["render"], v["gt"]).transpose(1, 2, 0)) and (f.depth[..., 3] == 255).all()
    # an empty lsq mask: det = 0, the aligned half is constant 0;  a NaN depth: the whole picture is (0, 0, 0, 0)
    e = Fr.view_frames(*(t(v[k]) for k in ("render", "uncertainty", "gt", "depth", "midas")), torch.ones(1, H, W))
    assert (e.params[0, 2:4] == 0).all() and float(e.params[0, 4]) == 0.0
    assert np.array_equal(e.depth.numpy(), O.view_oracle(v, e.params.numpy(), viridis())[1]) and (e.depth[:, :W, :3].numpy() == viridis()[0]).all()
    bad = v["depth"].copy()
    bad[0, 2, 3] = np.nan
    n = Fr.view_frames(t(v["render"]), t(v["uncertainty"]), t(v["gt"]), t(bad), t(v["midas"]), t(v["mask"]))
    assert torch.isnan(n.params[0, [0, 1, 4, 5]]).all() and (n.depth == 0).all() and np.array_equal(n.sheet.numpy(), sheet)


def test_a_last_bit_of_params_moves_few_pixels():
    """The end-to-end GPU test lets the two paths' scale / shift differ in the last bit (the order of the fp64 sums) and caps the pixels
    that may move at 1 % of the panel; on its inputs a whole ulp either way moves far fewer."""
    v = O.view_inputs(37, 53, 11)
    o = O.frame_params(v["depth"][0], v["midas"][0], 1 - v["mask"][0])
    base = O.view_oracle(v, o["params"][None], viridis())[1]
    worst = 0.0
    for k in (2, 3):
        for to in (np.float32(np.inf), np.float32(-np.inf)):
            p = o["params"].copy()
            p[k] = np.nextafter(p[k], to)
            p[4:6] = O.extrema(np.concatenate([O.aligned(v["depth"][0], p[2], p[3]).ravel(), v["midas"].ravel()]))
            worst = max(worst, (O.view_oracle(v, p[None], viridis())[1] != base).any(-1).mean())
    print(f"37x53: one ulp of scale or shift moves at most {worst:.4%} of the depth picture's pixels")
    assert worst <= 0.01


# ---- the tables ----
def test_the_colour_tables_are_what_matplotlib_gives():
    matplotlib = pytest.importorskip("matplotlib")
    table = Fr.load_colormaps()  # gscream_amd/colormaps.json
    assert table.dtype == np.uint8 and table.shape == (2, 256, 3)
    for k, (name, rounded) in enumerate((("inferno", True), ("viridis", False))):
        c = np.asarray(matplotlib.colormaps[name].colors, np.float64) * 255.0
        assert np.array_equal(table[k], np.floor(c + 0.5).astype(np.uint8) if rounded else c.astype(np.uint8)), name
        assert np.array_equal(Fr.colormap_lut(name).numpy(), table[k])
    with pytest.raises(ValueError):
        Fr.colormap_lut("magma")


# ---- header, binding, library ----
def test_header_binding_and_library_agree(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and _native.ABI_VERSION == 9 and native_lib.gsr_abi_version() == 9
    assert hdr.constants["GSR_FRAME_MAX_PANELS"] == 8 and _native.FRAME_MAX_PANELS == 8 == Fr.MAX_PANELS
    for k, name in enumerate(("QUANT", "QUANT_CLAMP", "ABSDIFF", "NORMAL", "CMAP_CV", "CMAP_MPL_ALIGNED", "CMAP_MPL")):
        assert hdr.constants[f"GSR_FRAME_{name}"] == k and getattr(_native, f"FRAME_{name}") == k == getattr(Fr, name) == getattr(O, name)
    assert hdr.functions["gsr_frame_stats_workspace_bytes"][0] == "size_t" and hdr.functions["gsr_frame_stats"][0] == "int"
    assert hdr.functions["gsr_frame_compose"][0] == "int"
    for name in ("gsr_frame_stats_workspace_bytes", "gsr_frame_stats", "gsr_frame_compose"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
    assert len(native_lib.gsr_frame_stats.argtypes) == 10 and len(native_lib.gsr_frame_compose.argtypes) == 9
    declared = [f for _, f, _ in hdr.structs["gsr_frame_panel"]]
    assert declared == [f[0] for f in _native.FramePanel._fields_] and ctypes.sizeof(_native.FramePanel) == 72
    for lib in ("libgsraster_precise.so", "libgsraster_replayall.so"):  # the two test builds link the same objects
        path = os.path.join(os.path.dirname(_native.LIB_PATH), lib)
        if os.path.exists(path):
            assert hasattr(ctypes.CDLL(path), "gsr_frame_compose")


def test_frame_stats_rejections_without_a_gpu(native_lib):
    """Everything the call rejects, it rejects before launching (there is no device here to launch on)."""
    call, size, err = native_lib.gsr_frame_stats, native_lib.gsr_frame_stats_workspace_bytes, native_lib.gsr_last_error
    a, b, c, d, e, f = 256, 512, 768, 1024, 1280, 1536  # never dereferenced on the host

    def run(B=1, H=5, W=7, depth=a, target=b, mask=c, ws=d, stats=e, params=f):
        return call(B, H, W, depth, target, mask, ws, stats, params, None)

    for k in ("depth", "ws", "stats", "params"):
        assert run(**{k: None}) == -1 and b"NULL" in err(), k
    assert run(target=None) == -1 and b"needs a target" in err()
    for bhw in ((0, 5, 7), (1, 0, 7), (1, 5, 0), (-1, 5, 7), (1, -5, 7), (1, 5, -7)):
        assert run(*bhw) == -1 and b"need all > 0" in err(), bhw
        assert size(*bhw) == 0
    assert run(B=65536) == -1 and b"too many frames" in err() and size(65536, 5, 7) == 0
    for hw in ((23171, 23171), (1, 536870848), (536870848, 1), (1 << 20, 1 << 20), (2147483647, 2147483647)):  # (the last: H*W*4 passes 2^63)
        assert run(H=hw[0], W=hw[1]) == -1 and b"too many pixels" in err(), hw
        assert size(1, *hw) == 0
    assert size(1, 1, 536870847) > 0  # H*W*4 = 2^31 - 260: the largest frame
    assert size(1, 5, 7) == 64 and size(3, 64, 64) == 3 * 64 and size(2, 64, 65) == 2 * 2 * 64 and size(40, 567, 1008) == 40 * 140 * 64


def test_frame_compose_rejections_without_a_gpu(native_lib):
    from gscream_amd._native import FramePanel
    call, err = native_lib.gsr_frame_compose, native_lib.gsr_last_error
    src, src2, lut, params, out = 256, 512, 768, 1024, 1280  # never dereferenced on the host

    def panel(x0, width, mode=0, src=src, src2=src2, lut=lut):
        p = FramePanel()
        p.src, p.src2, p.lut, p.x0, p.width, p.mode = src, src2, lut, x0, width, mode
        p.stride_b, p.stride_c, p.stride_y, p.stride_x = 0, 0, 0, 1
        return p

    def run(panels, B=1, H=5, W_out=12, channels=3, n=None, params=params, out=out, table=True):
        arr = (FramePanel * max(len(panels), 1))(*panels)
        return call(B, H, W_out, channels, len(panels) if n is None else n, arr if table else None, params, out, None)

    good = [panel(0, 5), panel(5, 7)]
    for bhw in ((0, 5, 12), (1, 0, 12), (1, 5, 0), (-1, 5, 12), (1, 5, -12)):
        assert run(good, *bhw) == -1 and b"need all > 0" in err(), bhw
    assert run(good, B=65536) == -1 and b"too many frames" in err()
    assert run([panel(0, 23171)], H=23171, W_out=23171) == -1 and b"too many pixels" in err()
    assert run([panel(0, 2147483647)], H=2147483647, W_out=2147483647) == -1 and b"too many pixels" in err()
    for ch in (0, 1, 2, 5, -3):
        assert run(good, channels=ch) == -1 and b"need 3 or 4" in err(), ch
    for n in (0, -1, 9, 1 << 20):
        assert run(good, n=n) == -1 and b"need 1 .. 8" in err(), n
    assert run(good, table=False) == -1 and b"NULL" in err()
    assert run(good, out=None) == -1 and b"NULL" in err()
    for mode in (-1, 7, 100):
        assert run([panel(0, 5), panel(5, 7, mode)]) == -1 and b"unknown mode" in err(), mode
    assert run([panel(0, 5), panel(5, 7, src=None)]) == -1 and b"NULL src" in err()
    assert run([panel(0, 5), panel(5, 7, 2, src2=None)]) == -1 and b"NULL src2" in err()
    for mode in (4, 5, 6):
        assert run([panel(0, 5), panel(5, 7, mode, lut=None)]) == -1 and b"NULL lut or params" in err(), mode
        assert run([panel(0, 5), panel(5, 7, mode)], params=None) == -1 and b"NULL lut or params" in err(), mode
    for bad in ([panel(0, 5), panel(5, 0)], [panel(0, 5), panel(5, -7)], [panel(-1, 6), panel(5, 7)], [panel(0, 5), panel(5, 8)],
                [panel(0, 5), panel(2147483647, 7)]):
        assert run(bad) == -1 and b"outside [0, 12) or empty" in err()
    assert run([panel(0, 6), panel(5, 7)]) == -1 and b"overlap" in err()
    assert run([panel(5, 7), panel(0, 6)]) == -1 and b"overlap" in err()
    assert run([panel(0, 5), panel(0, 5), panel(5, 7)]) == -1 and b"overlap" in err()
    assert run([panel(0, 4), panel(5, 7)]) == -1 and b"leave a gap" in err()
    assert run([panel(1, 4), panel(5, 7)]) == -1 and b"leave a gap" in err()
    assert run([panel(0, 5), panel(5, 6)]) == -1 and b"leave a gap" in err()


def test_python_rejects_bad_panels_before_any_call(monkeypatch):
    from gscream_amd import _native

    def no_call(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "run", no_call)
    monkeypatch.setattr(Fr, "_compose_torch", no_call)
    x = torch.zeros(1, 3, 4, 5)
    one = torch.zeros(1, 1, 4, 5)
    lut = Fr.colormap_lut("viridis")
    P = Fr.Panel
    for panels, kw in (([P(0, x, x0=0), P(0, x, x0=4)], {}), ([P(0, x, x0=0), P(0, x, x0=6)], {}), ([P(0, x, x0=1)], {}), ([P(0, x)], {"width": 6}),
                       ([P(0, x)], {"width": 4}), ([], {}), ([P(0, x)] * 9, {}), ([P(7, x)], {}), ([P(0, one)], {}), ([P(4, x, lut=lut)], {}),
                       ([P(0, x), P(0, x[:, :, :3])], {}), ([P(2, x)], {}), ([P(2, x, x[..., :4])], {}), ([P(4, one)], {}),
                       ([P(4, one, lut=lut)], {}), ([P(4, one, lut=lut)], {"params": torch.zeros(2, 8)}), ([P(0, x)], {"channels": 2}),
                       ([P(0, x[0])], {})):
        with pytest.raises(ValueError):
            Fr.compose(panels, **kw)
    with pytest.raises(ValueError):
        Fr.frame_stats(torch.zeros(4, 5), None, torch.ones(4, 5))
    with pytest.raises(ValueError):
        Fr.frame_stats(torch.zeros(4, 5), torch.zeros(4, 6))
    # panels given out of order tile as well
    monkeypatch.undo()
    a, b = torch.rand(1, 3, 4, 5), torch.rand(1, 3, 4, 2)
    got = Fr.compose([P(0, a, x0=2), P(0, b, x0=0)])
    assert np.array_equal(got.numpy(), O.compose_oracle([{"mode": 0, "src": b.numpy()}, {"mode": 0, "src": a.numpy()}]))
