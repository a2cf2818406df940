"""gscream_amd.frames on the device: gsr_frame_stats and gsr_frame_compose against the numpy oracle of tests/frames_helpers.py.  Every
rule ends in an integer, so every output byte of every mode is held to equality -- no tolerance, no pixel left out -- with the
oracle given the fp32 `params` the device computed; the stats are held to numpy's extrema bit for bit, to exactly rounded sums within
the count of fp64 roundings, and to one fp32 ulp of the fp64 quotients.

Shapes: 5x7 (every row unaligned, panels narrower than one thread's four pixels), 37x53 (a byte-store tail), 24x32 (whole dwords
throughout), B = 1 and 3, 1, 4 and 8 panels, each with a flipped source, a stride-0 channel and the interleaved normal layout.  At 5x7
and 37x53 the three-channel cases of every panel count have a width that is no multiple of four, so they take the byte-store kernel
with a short last group that a panel edge crosses; separate mixes of the same odd panels that sum to a multiple of four take whole
dwords across panel edges.  Each case asserts the width that decides its path."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import frames_helpers as O  # noqa: E402

from gscream_amd import frames as Fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((5, 7), (37, 53), (24, 32))


@pytest.fixture
def HIP(monkeypatch):
    """The torch statements made to raise: these tests must run the kernels."""
    def no_fallback(*a, **k):
        raise AssertionError("took the torch path")
    monkeypatch.setattr(Fr, "_compose_torch", no_fallback)
    monkeypatch.setattr(Fr, "_stats_torch", no_fallback)
    return Fr


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lut(name):
    return Fr.colormap_lut(name, DEV)


def lut_np(name):
    return Fr.colormap_lut(name).numpy()


@functools.lru_cache(maxsize=None)
def batch(H, W, B):
    """B views of view_inputs stacked, with the quantiser's edge values sown into the images."""
    views = [O.view_inputs(H, W, 100 * H + 10 * B + b) for b in range(B)]
    out = {k: np.stack([v[k] for v in views]) for k in views[0]}
    edge = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.5 / 255, 254.5 / 255, 1e-9, 3e38, -3e38])
    flat = out["render"].reshape(-1)
    flat[np.random.default_rng(H).choice(flat.size, edge.size, replace=False)] = edge
    return out


def stats_of(d, y=None, m=None):
    """frame_stats on the device -> (stats, params) on the host."""
    s, p = Fr.frame_stats(dev(d), None if y is None else dev(y), None if m is None else dev(m))
    assert Fr.last_path == "hip" and s.dtype == torch.float64 and p.dtype == torch.float32 and s.shape == p.shape == (d.shape[0], 8)
    return s.cpu().numpy(), p.cpu().numpy()


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def check_stats(d, y, m, what):
    stats, params = stats_of(d, y, m)
    for b in range(d.shape[0]):
        o = O.frame_params(d[b], None if y is None else y[b], None if m is None else m[b])
        p = params[b]
        assert np.array_equal(bits(p[:2]), bits(o["params"][:2])), (what, b, p, o["params"])
        assert (p[6:] == 0).all()
        if y is None:
            assert (p[2:6] == 0).all() and (stats[b] == 0).all()
            continue
        off = np.abs(stats[b, :5] - o["sums"])
        print(f"{what} frame {b}: sums off the exactly rounded ones by {off.tolist()} of a bound {o['sum_bound'].tolist()}; scale {p[2]!r} shift {p[3]!r} "
              f"(fp64 {abs(o['x0'])!r}, {o['x1']!r})")
        assert (off <= o["sum_bound"]).all(), (what, b, off, o["sum_bound"])
        assert O.within_one_ulp(p[2], abs(o["x0"])) and O.within_one_ulp(p[3], o["x1"]), (what, b, p, o["x0"], o["x1"])
        # lo2 / hi2: numpy's extrema of the panel formed from the device's own rounded scale and shift
        want = O.extrema(np.concatenate([O.aligned(d[b], p[2], p[3]).ravel(), y[b].ravel()]))
        assert np.array_equal(bits(p[4:6]), bits(want)), (what, b, p, want)


# ---- stats ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES + ((67, 131),))  # 67 x 131: three chunks of 4096, the last one partial
def test_stats_against_the_oracle(shape, B, HIP):
    v = batch(*shape, B)
    d, y, m = v["depth"][:, 0], v["midas"][:, 0], 1 - v["mask"][:, 0]
    check_stats(d, y, m, f"{shape} masked")
    check_stats(d, y, None, f"{shape} no mask")
    check_stats(d, None, None, f"{shape} depth alone")


def test_stats_of_a_full_hd_frame(HIP):
    """1080 x 1920: 507 chunks, so the finishing workgroup's threads take two partials each."""
    rng = np.random.default_rng(8)
    i, j = np.meshgrid(np.arange(1080, dtype=np.float32), np.arange(1920, dtype=np.float32), indexing="ij")
    d = (2.0 + 0.001 * j + 0.0005 * i + 0.2 * rng.random((1080, 1920), dtype=np.float32)).astype(np.float32)[None]
    y = (0.4 * d + 0.7 + 0.05 * rng.random(d.shape, dtype=np.float32)).astype(np.float32)
    m = (rng.random(d.shape) < 0.8).astype(np.float32)
    check_stats(d, y, m, "1080x1920")


def test_stats_edge_frames(HIP):
    v = batch(37, 53, 3)
    d, y = v["depth"][:, 0].copy(), v["midas"][:, 0]
    d[1] = 2.5          # a constant depth: lo == hi, det = 0 under any mask
    d[2, 5, 7] = np.nan  # a NaN: lo, hi, the sums, scale, shift, lo2, hi2 are all NaN, in its frame only
    m = 1 - v["mask"][:, 0]
    m[0] = 0            # an empty lsq mask: det = 0
    stats, params = stats_of(d, y, m)
    assert np.array_equal(bits(params[0, :2]), bits(O.extrema(d[0]))) and (params[0, 2:4] == 0).all() and (stats[0] == 0).all()
    assert np.array_equal(bits(params[0, 4:6]), bits([min(0, y[0].min()), max(0, y[0].max())]))
    assert (params[1, :2] == 2.5).all() and stats[1, 5] == 0 and (params[1, 2:4] == 0).all()
    assert np.isnan(params[2, :6]).all() and np.isnan(stats[2, [0, 1, 3, 5, 6, 7]]).all() and (params[:, 6:] == 0).all()
    alone = stats_of(d[:1], y[:1], m[:1])
    assert np.array_equal(alone[0], stats[:1]) and np.array_equal(bits(alone[1]), bits(params[:1]))


# ---- compose ----
def widths_for(W, n, dwords):
    """n panel widths.  dwords: the full width (a multiple of four) every time.  Otherwise a mix with panels narrower than one thread's
    four pixels whose sum is no multiple of four -- three-channel output then takes the byte-store kernel -- and leaves three columns to
    the last thread of a row, with a panel edge between them: 2W + 1 for four panels, 4W + 7 for eight, W odd."""
    if dwords or n == 1:
        return [W] * n
    widths = {4: [W, 3, W - 3, 1], 8: [W, 3, W - 2, 1, W, 5, W - 2, 2]}[n]
    assert sum(widths) % 4 == 3 and widths[-1] < 3
    return widths


def build_panels(v, modes, widths, flip_every=2):
    """-> (device Panels, oracle dicts).  Sources are column slices of full-width tensors (their row stride stays the full width); every
    QUANT_CLAMP panel is a one-channel image expanded with stride 0, every NORMAL panel the interleaved [H*W, 3] rows, every second
    panel flipped."""
    B, _, H, W = v["render"].shape
    t = {k: dev(a) for k, a in v.items()}
    panels, dicts = [], []
    for k, (mode, w) in enumerate(zip(modes, widths)):
        flip = k % flip_every == 0
        x = (k * 3) % (W - w + 1)  # where the slice starts in its source
        sl = slice(x, x + w)
        if mode == O.QUANT:
            src, ref, kw = t["render"][..., sl], v["render"][..., sl], {}
        elif mode == O.QUANT_CLAMP:
            src, ref, kw = t["uncertainty"][..., sl].expand(-1, 3, -1, -1), v["uncertainty"][..., sl], {}
            assert src.stride(1) == 0
        elif mode == O.ABSDIFF:
            src, ref, kw = t["render"][..., sl], v["render"][..., sl], {"src2": (t["gt"][..., sl], v["gt"][..., sl])}
        elif mode == O.NORMAL:
            src = t["normals"].view(B, H, W, 3).permute(0, 3, 1, 2)[..., sl]
            ref, kw = v["normals"].reshape(B, H, W, 3).transpose(0, 3, 1, 2)[..., sl], {}
            assert src.stride()[1:] == (1, 3 * W, 3)
        else:
            key = "midas" if mode == O.CMAP_MPL else "depth"
            name = "inferno" if mode == O.CMAP_CV else "viridis"
            src, ref, kw = t[key][..., sl], v[key][..., sl], {"lut": (lut(name), lut_np(name))}
        panels.append(Fr.Panel(mode, src, kw["src2"][0] if "src2" in kw else None, kw["lut"][0] if "lut" in kw else None, flip))
        dicts.append({"mode": mode, "src": ref, "flip": flip, **{key: val[1] for key, val in kw.items()}})
    return panels, dicts


ALL = (O.QUANT, O.QUANT_CLAMP, O.ABSDIFF, O.NORMAL, O.CMAP_CV, O.CMAP_MPL_ALIGNED, O.CMAP_MPL)
MIXES = {4: (O.NORMAL, O.CMAP_CV, O.QUANT_CLAMP, O.CMAP_MPL_ALIGNED), 8: ALL + (O.QUANT,)}


def check_compose(v, params, modes, widths, channels, what):
    panels, dicts = build_panels(v, modes, widths)
    got = Fr.compose(panels, channels=channels, params=params)
    assert Fr.last_path == "hip" and got.dtype == torch.uint8 and tuple(got.shape) == (v["render"].shape[0], v["render"].shape[2], sum(widths), channels)
    assert got.data_ptr() % 4 == 0  # so the stores are whole dwords exactly when channels == 4 or the width is a multiple of four
    want = O.compose_oracle(dicts, params.cpu().numpy(), channels)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{what}: {(got != want).any(-1).sum()} of {want[..., 0].size} pixels differ, first at {np.argwhere((got != want).any(-1))[:3].tolist()}"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_compose_every_byte_of_every_mode(shape, B, HIP):
    H, W = shape
    v = batch(H, W, B)
    _stats, params = Fr.frame_stats(dev(v["depth"][:, 0]), dev(v["midas"][:, 0]), dev(1 - v["mask"][:, 0]))
    dwords = W % 4 == 0
    for channels in (3, 4):
        for mode in ALL:  # one panel: each mode alone, flipped
            check_compose(v, params, (mode,), [W], channels, f"{shape} B={B} mode {mode} alone, {channels} channels")
        for n in (4, 8):
            widths = widths_for(W, n, dwords)
            assert (sum(widths) % 4 == 0) == dwords  # 24x32: whole dwords throughout; 5x7, 37x53: with three channels, bytes
            check_compose(v, params, MIXES[n], widths, channels, f"{shape} B={B} {n} panels, {channels} channels")
    if not dwords:  # a width that is a multiple of four from panels that are not: whole dwords across panel edges
        for n, widths in ((4, [W, 3, W - 2, 1 + (2 - 2 * W) % 4]), (8, [W, 3, W - 2, 1, W, 5, W - 2, 1 + (2 - 4 * W) % 4])):
            assert sum(widths) % 4 == 0 and all(w % 4 for w in widths)
            check_compose(v, params, MIXES[n], widths, 3, f"{shape} B={B} {n} panels, dwords across panel edges")


def test_compose_edge_values(HIP):
    """NaN, +-inf and -0.0 through the quantiser; a constant depth and a NaN depth through both maps; an empty lsq mask."""
    x = np.float32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.75 / 255, 0.25 / 255, 254.75 / 255, 2.0, -1.0, 0.5]).reshape(1, 1, 3, 4)
    want = np.uint8([0, 255, 0, 0, 0, 255, 1, 0, 255, 255, 0, 128]).reshape(3, 4)
    for clamp in (False, True):
        got = Fr.to_uint8(dev(x)[0], clamp=clamp)
        assert Fr.last_path == "hip" and tuple(got.shape) == (3, 4, 3) and (got.cpu().numpy() == want[..., None]).all()
    H, W = 6, 9
    v = O.view_inputs(H, W, 2)
    inferno, viridis = lut_np("inferno"), lut_np("viridis")
    args = [dev(v[k]) for k in ("render", "uncertainty", "gt", "depth", "midas", "mask")]
    flat = torch.full((1, H, W), 2.5, device=DEV)
    f = Fr.rgbd_frame(args[0], flat, args[1], torch.zeros(H * W, 3, device=DEV), panels=True)
    assert (f.depth.cpu().numpy() == inferno[0]).all() and (f.normal.cpu().numpy() == 128).all()
    zero = torch.zeros(1, H, W, device=DEV)
    same = Fr.view_frames(args[0], args[1], args[2], zero, zero, args[5])  # det = 0, aligned = 0 = the target: hi2 == lo2
    assert (same.depth.cpu().numpy() == np.append(viridis[0], 255)).all()
    empty = Fr.view_frames(*args[:5], torch.ones(1, H, W, device=DEV))
    p = empty.params.cpu().numpy()
    assert (p[0, 2:4] == 0).all() and np.array_equal(empty.depth.cpu().numpy(), O.view_oracle(v, p, viridis)[1])
    assert (empty.depth[:, :W, :3].cpu().numpy() == viridis[0]).all()
    bad = args[3].clone()
    bad[0, 2, 3] = float("nan")
    n = Fr.view_frames(args[0], args[1], args[2], bad, args[4], args[5])
    assert (n.depth == 0).all() and torch.equal(n.sheet, empty.sheet)
    f = Fr.rgbd_frame(args[0], bad, args[1], dev(v["normals"]), panels=True)
    assert (f.depth.cpu().numpy() == inferno[0]).all() and Fr.last_path == "hip"


# ---- end to end ----
def test_rgbd_frame_and_view_frames_against_the_torch_path():
    """37 x 53.  The two paths may differ in the last bit of scale / shift (the order of the fp64 sums); a pixel whose colour index that bit
    decides may differ between them, is recomputed with the device's params, and such pixels are capped at 1 % of the panel."""
    H, W = 37, 53
    v = O.view_inputs(H, W, 11)
    t = {k: dev(a) for k, a in v.items()}
    as_returned = t["normals"].view(1, W, H, 3).permute(0, 3, 1, 2)  # least_square_normal_regress_fast01's return layout
    view_args = [t[k] for k in ("render", "uncertainty", "gt", "depth", "midas", "mask")]
    hip_rgbd = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], as_returned)
    hip_view = Fr.view_frames(*view_args)
    assert Fr.last_path == "hip"
    Fr.force_torch = True
    try:
        torch_rgbd = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], as_returned)
        torch_view = Fr.view_frames(*view_args)
        assert Fr.last_path == "torch"
    finally:
        Fr.force_torch = False
    assert torch.equal(hip_rgbd, torch_rgbd)  # lo and hi are exact on both paths
    assert torch.equal(hip_view.sheet, torch_view.sheet)
    p_hip, p_torch = hip_view.params.cpu().numpy(), torch_view.params.cpu().numpy()
    assert np.array_equal(p_hip[0, :2], p_torch[0, :2]) and O.within_one_ulp(p_hip[0, 2:4], p_torch[0, 2:4].astype(np.float64)).all()
    moved = (hip_view.depth != torch_view.depth).any(-1).cpu().numpy()
    print(f"params hip {p_hip[0, :6].tolist()} torch {p_torch[0, :6].tolist()}: {moved.sum()} of {moved.size} pixels differ between the paths")
    if np.array_equal(bits(p_hip), bits(p_torch)):
        assert not moved.any()
    assert moved.mean() <= 0.01
    want = O.view_oracle(v, p_hip, lut_np("viridis"))[1]
    assert np.array_equal(hip_view.depth.cpu().numpy()[moved], want[moved]) and np.array_equal(hip_view.depth.cpu().numpy(), want)
    assert np.array_equal(hip_rgbd.cpu().numpy(), O.rgbd_oracle(v, Fr.frame_stats(t["depth"][0])[1].cpu().numpy(), lut_np("inferno")))


# ---- call discipline ----
def test_the_calls_do_not_stop_the_host_and_repeat_bit_for_bit(HIP):
    H, W = 37, 53
    v = O.view_inputs(H, W, 12)
    t = {k: dev(a) for k, a in v.items()}
    view_args = [t[k] for k in ("render", "uncertainty", "gt", "depth", "midas", "mask")]
    first = (Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], t["normals"], panels=True), Fr.view_frames(*view_args),
             Fr.to_uint8(t["render"]))  # library loading, the colour tables and first allocations out of the way
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        f = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], t["normals"], panels=True)
        w = Fr.view_frames(*view_args)
        u = Fr.to_uint8(t["render"])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert Fr.last_path == "hip"
    assert torch.equal(f.rgbd, first[0].rgbd) and torch.equal(w.sheet, first[1].sheet) and torch.equal(w.depth, first[1].depth) and torch.equal(u, first[2])
    assert torch.equal(w.params.view(torch.int32), first[1].params.view(torch.int32))
    # the panels are views of the one buffer
    assert tuple(f.rgbd.shape) == (H, 4 * W, 3) and f.rgbd.is_contiguous()
    for k, p in enumerate(f[1:]):
        assert p.data_ptr() == f.rgbd.data_ptr() + 3 * W * k and tuple(p.shape) == (H, W, 3) and p.stride() == f.rgbd.stride()
        assert torch.equal(p, f.rgbd[:, k * W:(k + 1) * W])
    for k, p in enumerate(w[:4]):
        assert p.data_ptr() == w.sheet.data_ptr() + 3 * W * k and p.stride() == w.sheet.stride()


def test_the_current_stream_is_honoured(HIP):
    """On a side stream, behind a delay and the copy that fills the input: a launch on any other stream would read the zeros."""
    v = O.view_inputs(24, 32, 13)
    t = {k: dev(a) for k, a in v.items()}
    want = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], t["normals"])
    staged = torch.zeros_like(t["depth"])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(20_000_000)
        staged.copy_(t["depth"])
        got = Fr.rgbd_frame(t["render"], staged, t["uncertainty"], t["normals"])
    st.synchronize()
    assert Fr.last_path == "hip" and torch.equal(got, want) and not torch.equal(got[:, 32:64], got[:, 32:33].expand(-1, 32, -1))
