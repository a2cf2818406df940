"""gscream_amd.jpeg and gscream_amd.video on the device: every file must equal, byte for byte, the numpy statement of the rules
(tests/jpeg_helpers.py encode), which tests/test_jpeg.py holds against PIL; the buffers around the files must stay untouched."""
import io
import warnings

import numpy as np
import pytest
import torch

from tests import arena_helpers as A
from tests import jpeg_helpers as J
from gscream_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5


def _device(image):
    return image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image)).to(DEV)


def _encode(image, quality=95, subsampling="4:2:0", ri=None, **kw):
    from gscream_amd import jpeg
    batch = jpeg.encode(_device(image), quality, subsampling, ri, **kw)
    assert jpeg.last_path == "hip"
    return jpeg.to_bytes(batch)


def _load(data, H, W, C):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
    return im


def _check(image, quality=95, subsampling="4:2:0", ri=None):
    H, W, C = image.shape
    (data,) = _encode(image, quality, subsampling, ri)
    want = J.encode(image, quality, subsampling, ri)
    assert len(data) == len(want), (len(data), len(want))
    if data != want:
        a, b = np.frombuffer(data, np.uint8), np.frombuffer(want, np.uint8)
        first = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"the device's bytes differ from the rules', first at byte {first} of {len(want)} (0x{a[first]:02x} / 0x{b[first]:02x})")
    _load(data, H, W, C)
    from gscream_amd import jpeg
    assert len(data) <= jpeg.capacity(H, W, C, subsampling)
    return data


# (H, W, C, subsampling, Ri): the shapes where the kernels can still go wrong
SHAPES = [
    (1, 1, 1, "4:4:4", None), (1, 1, 3, "4:4:4", None), (1, 1, 3, "4:2:0", None),
    (5, 7, 3, "4:4:4", None), (5, 7, 3, "4:2:0", None),              # less than one block
    (37, 53, 3, "4:4:4", None), (37, 53, 3, "4:2:0", None),          # edge replication in both axes, a partial MCU
    (16, 16, 3, "4:2:0", None), (16, 16, 3, "4:4:4", None),          # exactly one 4:2:0 MCU
    (8, 264, 1, "4:4:4", None),                                      # 33 blocks a row
    (88, 24, 3, "4:4:4", 3),                                         # 11 intervals: RST wraps
    (37, 53, 3, "4:2:0", 1), (24, 40, 1, "4:4:4", 1),                # Ri = 1
    (64, 1024, 1, "4:4:4", 1024),                                    # an interval of exactly GSR_JPEG_INTERVAL_BLOCKS blocks
    (16, 8200, 1, "4:4:4", None),                                    # a row of 1025 blocks: the default interval is cut to 1024
    (16, 2736, 3, "4:2:0", None),                                    # 171 MCUs a row at 6 blocks: the default interval is 170
    (40, 120, 3, "4:2:0", 7), (40, 120, 3, "4:4:4", 50),             # intervals that cross MCU rows; 150 blocks: the 256-thread form
]


@pytest.mark.parametrize("H,W,C,subsampling,ri", SHAPES)
def test_shapes(H, W, C, subsampling, ri):
    data = _check(J.picture("texture", H, W, C, seed=H + W), 90, subsampling, ri)
    info = J.parse(data)
    assert info["intervals"] == J.geometry(H, W, C, subsampling, ri)["intervals"]
    if (H, W, ri) == (88, 24, 3):
        assert info["intervals"] == 11
    if W in (8200, 2736):
        assert info["dri"] == J.INTERVAL_BLOCKS // (6 if C == 3 else 1) < J.geometry(H, W, C, subsampling)["mcux"]


def test_contents_and_the_rare_tokens():
    """The five contents at 96 x 250 x 3, q in {1, 50, 100}, both subsamplings: ZRL, blocks without EOB, stuffed 0xFF bytes (also two
    in a row: the two-level picture at q = 100, 4:4:4) and 11-bit DC differences must all occur among them."""
    totals = dict(zrl=0, no_eob=0, stuffed=0, ff_pairs=0, dc11=0)
    for kind in J.KINDS:
        image = J.picture(kind, 96, 250, 3, seed=3)
        for quality in (1, 50, 100):
            for sub in ("4:2:0", "4:4:4"):
                _check(image, quality, sub)
                _, st = J.encode(image, quality, sub, stats=True)
                for k in totals:
                    totals[k] += st[k]
    assert all(v > 0 for v in totals.values()), totals


def test_batch_of_strided_panels():
    """B = 3 panels of a wider sheet, read in place through the row and picture strides, against their dense copies."""
    from gscream_amd import jpeg, png
    sheet = np.concatenate([J.picture(k, 37, 53, 3, seed=5) for k in ("texture", "edges", "noise")], 1)
    panels = png._panels(_device(sheet), 3)
    assert not panels.is_contiguous() and panels.stride(0) == 53 * 3
    files = jpeg.to_bytes(jpeg.encode(panels, 90))
    assert jpeg.last_path == "hip" and len(files) == 3 and len(set(files)) == 3
    for b, data in enumerate(files):
        dense = np.ascontiguousarray(sheet[:, 53 * b:53 * (b + 1)])
        assert data == J.encode(dense, 90) == _encode(dense, 90)[0]


def test_small_cap_reports_need_capacity_and_to_bytes_recovers():
    from gscream_amd import jpeg
    images = np.stack([J.picture("constant", 64, 96, 3), J.picture("noise", 64, 96, 3)])
    want = [J.encode(im, 100, "4:4:4") for im in images]
    cap = (len(want[0]) + len(want[1])) // 2  # the constant picture fits, the noise does not
    assert len(want[0]) + 3 < cap < len(want[1])
    out = torch.full((2, (jpeg.HEADER + cap + 3) & ~3), POISON, dtype=torch.uint8, device=DEV)
    batch = jpeg.encode(_device(images), 100, "4:4:4", out=out)
    host = out.cpu().numpy()
    words = host[:, :16].copy().view("<u4")
    assert words[0].tolist() == [len(want[0]), 0, 8, 0] and words[1].tolist() == [len(want[1]), jpeg.NEED_CAPACITY, 8, 0]
    assert host[0, 16:16 + len(want[0])].tobytes() == want[0]
    assert (host[0, 16 + len(want[0]):] == POISON).all(), "bytes behind the file's last were written"
    assert (host[1, 16:] == POISON).all(), "a file that did not fit wrote behind its header words"
    assert jpeg.to_bytes(batch) == want and jpeg.last_info["reencoded"] == 1


def test_nothing_is_written_behind_a_file():
    from gscream_amd import jpeg
    images = np.stack([J.picture(k, 37, 53, 3, seed=2) for k in ("texture", "ramp", "edges")])
    want = [J.encode(im, 95) for im in images]
    out = torch.full((3, (jpeg.HEADER + jpeg.capacity(37, 53, 3) + 8) & ~3), POISON, dtype=torch.uint8, device=DEV)
    jpeg.encode(_device(images), out=out)
    host = out.cpu().numpy()
    for b in range(3):
        assert host[b, 16:16 + len(want[b])].tobytes() == want[b]
        assert (host[b, 16 + len(want[b]):] == POISON).all()


@pytest.mark.parametrize("H,W", [(567, 4032), (567, 1008)])
def test_full_size(H, W):
    """The sheet and the render of the reference's scenes, once each, at the video's settings for a 567-row picture."""
    _check(S.picture("texture", H, W, 3, seed=7), 95, "4:4:4" if W == 4032 else "4:2:0")


def _three_runs(monkeypatch, run, expect):
    runs = {}
    for name, poison in (("plain", None), ("arena_a5", 0xA5), ("arena_ff", 0xFF)):
        if poison is None:
            out = run()
        else:
            with A.guarded(monkeypatch, 64 << 20, poison, DEV) as (arena, proxy):
                out = run()
            assert all(proxy.calls.get(fn) for fn in expect), proxy.calls
            assert proxy.stats()[1] > 0, "the proxy saw no writable buffer"
        runs[name] = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    A.assert_same_bits(runs, "jpeg_encode")
    return runs["plain"]


def test_jpeg_encode_in_guarded_buffers(monkeypatch):
    """gsr_jpeg_encode inside guarded, poisoned buffers: grey and RGB, both subsamplings, a strided panel batch, and a buffer too small
    (whose second encode is guarded too).  Defined: the 16 header bytes and each file up to its byte count."""
    from gscream_amd import jpeg, png

    def run():
        out = {}
        for name, (H, W, C, sub, ri) in dict(grey=(24, 264, 1, "4:4:4", None), rgb444=(37, 53, 3, "4:4:4", 3), rgb420=(37, 53, 3, "4:2:0", None),
                                             wide=(16, 2736, 3, "4:2:0", None)).items():
            batch = jpeg.encode(_device(J.picture("texture", H, W, C, seed=H)), 90, sub, ri)
            out[name + "/header"] = batch.data[0, :jpeg.HEADER]
            out[name + "/file"] = np.frombuffer(jpeg.to_bytes(batch)[0], np.uint8)
        sheet = _device(np.concatenate([J.picture(k, 37, 53, 3, seed=5) for k in ("texture", "edges", "noise", "ramp")], 1))
        out["panels"] = np.frombuffer(b"".join(jpeg.to_bytes(jpeg.encode(png._panels(sheet, 4), 100, cap=4000))), np.uint8)
        assert jpeg.last_info["reencoded"] >= 1
        return out

    got = _three_runs(monkeypatch, run, ("gsr_jpeg_encode",))
    assert got["rgb420/file"].tobytes() == J.encode(J.picture("texture", 37, 53, 3, seed=37), 90, "4:2:0")


def test_two_runs_give_identical_bytes():
    image = _device(J.picture("noise", 96, 250, 3, seed=9))
    assert _encode(image, 100) == _encode(image, 100)


def test_save_rgbd_video_on_device_sheets(tmp_path):
    """frames.rgbd_frame's sheets -> the AVI: the RIFF parser and PIL accept the file, the frames equal jpeg.encode's."""
    from gscream_amd import frames, jpeg, video
    H, W, n = 36, 52, 5
    g = torch.Generator().manual_seed(1)
    sheets = []
    for _ in range(n):
        render, depth, unc = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g) + 0.5, torch.rand(1, H, W, generator=g)
        normal = torch.rand(3, H, W, generator=g)
        sheets.append(frames.rgbd_frame(render.to(DEV), depth.to(DEV), unc.to(DEV), normal.to(DEV)))
    assert tuple(sheets[0].shape) == (H, 4 * W, 3) and sheets[0].is_cuda
    path = tmp_path / "spiral.avi"
    assert video.save_rgbd_video(iter(sheets), str(path), batch=2) == n
    avi = J.parse_avi(path.read_bytes())
    assert (avi["width"], avi["height"], avi["fps"], len(avi["frames"])) == (4 * W, H, 25, n)
    for sheet, data in zip(sheets, avi["frames"]):
        assert data == jpeg.to_bytes(jpeg.encode(sheet))[0] == J.encode(sheet.cpu().numpy())
        assert J.parse(data)["subsampling"] == "4:2:0"
        _load(data, H, 4 * W, 3)
