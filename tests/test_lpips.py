"""CPU tests of gscream_amd/lpips.py: the torch statement of the rule against the independent fp64 oracle of tests/lpips_helpers.py,
the package's call shapes, the weight loaders, chunking, evaluate_views' keys, and the C ABI's bookkeeping and argument checks.
No kernel runs here."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_helpers as LH  # noqa: E402
from gscream_amd import lpips as LP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    return LH.make_weights(0)


@pytest.fixture(scope="module")
def model(weights):
    return LP.LPIPS(weights)


def rel(got, want):
    return LH.deviation(got, want) / max(float(want.abs().max()), 1e-300)


def test_oracle_bilinear_is_torchs():
    """The oracle's index arithmetic against F.interpolate in fp64 on the CPU, for the size pairs of the odd chain and an identity."""
    g = torch.Generator().manual_seed(5)
    for (h, w), (H, W) in (((18, 26), (37, 53)), ((2, 3), (37, 53)), ((1, 1), (16, 16)), ((37, 53), (37, 53)), ((4, 6), (37, 53))):
        m = torch.rand((2, h, w), generator=g, dtype=torch.float64)
        want = F.interpolate(m[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        # |src| < 64, so src and the weight t = src - i0 carry up to 64 * 2^-52 = 1.4e-14 whichever way they are formed; values in [0, 1)
        assert LH.deviation(LH.bilinear_oracle(m, H, W), want) <= 4 * 1.4e-14, ((h, w), (H, W))


def test_oracle_conv_and_pool_are_torchs():
    g = torch.Generator().manual_seed(6)
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((2, 5, 7, 9), (64, 5, 3, 3), (64,)))
    assert LH.deviation(LH.conv_oracle(x, w, b), F.relu(F.conv2d(x, w, b, padding=1))) <= 1e-13
    assert torch.equal(LH.pool_oracle(x), F.max_pool2d(x, 2, 2))


@pytest.mark.parametrize("hw", [(16, 16), (37, 53)])
def test_torch_statement_against_the_oracle(weights, model, hw):
    in0, in1 = LH.make_images(1, 2, *hw)
    mask = LH.make_masks(1, 2, *hw)
    want = LH.lpips_oracle(weights, in0, in1, mask)
    got = LP._lpips_torch(model, in0, in1, mask, dtype=torch.float64, out_dtype=torch.float64)
    for key in ("plain", "layers", "masked", "spatial"):
        assert rel(got[key], want[key]) <= 1e-12, (key, rel(got[key], want[key]))
    assert float(want["plain"].min()) > 1e-4, "the pair must differ visibly for the comparison to mean anything"
    rounded = LP._lpips_torch(model, in0, in1, mask)
    assert rounded["plain"].dtype == torch.float32 and rel(rounded["plain"], want["plain"]) <= 2.0 ** -24


def test_identical_images_give_exactly_zero(model):
    a, _ = LH.make_images(2, 2, 16, 16)
    r = LP._lpips_torch(model, a, a.clone())
    assert torch.equal(r["plain"], torch.zeros(2)) and not r["spatial"].any() and not r["layers"].any()
    assert torch.equal(model(a, a), torch.zeros(2, 1, 1, 1)) and LP.last_path == "torch"


def test_call_shapes_are_the_packages(weights):
    a, b = LH.make_images(3, 2, 16, 20)
    plain, spatial = LP.LPIPS(weights), LP.LPIPS(weights, spatial=True)
    assert plain(a, b).shape == (2, 1, 1, 1) and spatial(a, b).shape == (2, 1, 16, 20)
    val, layers = plain(a, b, retPerLayer=True)
    assert val.shape == (2, 1, 1, 1) and len(layers) == 5 and all(t.shape == (2, 1, 1, 1) for t in layers)
    assert LH.deviation(sum(layers), val) <= 1e-7
    val, layers = spatial.forward(a, b, retPerLayer=True)
    assert val.shape == (2, 1, 16, 20) and len(layers) == 5 and all(t.shape == (2, 1, 16, 20) for t in layers)
    assert plain(a[0], b[0]).shape == (1, 1, 1, 1)
    for bad in ((a[:, :2], b[:, :2]), (a, b[:1]), (a[..., :15], b[..., :15])):
        with pytest.raises(ValueError):
            plain(*bad)


def test_normalize_is_feeding_2x_minus_1(model):
    a, b = LH.make_images(4, 2, 16, 16, lo=0.0, hi=1.0)
    assert torch.equal(model(a, b, normalize=True), model(2 * a - 1, 2 * b - 1))
    assert not torch.equal(model(a, b, normalize=True), model(a, b))


def _package_state_dict(weights, with_lins=True):
    convs, biases, lins = weights
    sd = {}
    for w, b, n, s in zip(convs, biases, LP.FEATURE_INDEX, LP.SLICE_OF):
        sd[f"net.slice{s}.{n}.weight"], sd[f"net.slice{s}.{n}.bias"] = w, b
    for l, v in enumerate(lins):
        sd[f"lin{l}.model.1.weight"] = v.view(1, -1, 1, 1)
        if with_lins:
            sd[f"lins.{l}.model.1.weight"] = v.view(1, -1, 1, 1)
    sd["scaling_layer.shift"] = torch.tensor(LP.SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(LP.SCALE).view(1, 3, 1, 1)
    return sd


def _same_model(m, weights):
    return all(torch.equal(a, b.reshape(a.shape)) for got, want in zip((m.convs, m.biases, m.lins), weights) for a, b in zip(got, want))


def test_loaders(weights, tmp_path):
    sd = _package_state_dict(weights)
    assert _same_model(LP.LPIPS.from_state_dict(sd), weights)
    assert _same_model(LP.LPIPS.from_state_dict(_package_state_dict(weights, with_lins=False)), weights)

    class Module:
        spatial = True

        def state_dict(self):
            return sd
    adopted = LP.LPIPS.from_module(Module())
    assert _same_model(adopted, weights) and adopted.spatial and not LP.LPIPS.from_module(Module(), spatial=False).spatial

    vgg = {}
    for w, b, n in zip(weights[0], weights[1], LP.FEATURE_INDEX):
        vgg[f"features.{n}.weight"], vgg[f"features.{n}.bias"] = w, b
    vgg["classifier.0.weight"] = torch.zeros(2, 2)  # ignored
    lin = {f"lin{l}.model.1.weight": v.view(1, -1, 1, 1) for l, v in enumerate(weights[2])}
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    assert _same_model(LP.LPIPS.from_files(tmp_path / "vgg16.pth", tmp_path / "vgg.pth"), weights)

    for key in ("net.slice3.12.weight", "net.slice5.28.bias", "lin4.model.1.weight"):
        broken = dict(sd)
        del broken[key]
        with pytest.raises(ValueError, match=re.escape(key)):
            LP.LPIPS.from_state_dict(broken)
        broken[key] = sd[key].reshape(-1)[:-1].clone()  # mis-shaped
        with pytest.raises(ValueError, match=re.escape(key)):
            LP.LPIPS.from_state_dict(broken)
    wrong = dict(sd)
    wrong["scaling_layer.shift"] = torch.tensor([0.0, -0.088, -0.188]).view(1, 3, 1, 1)
    with pytest.raises(ValueError, match="scaling_layer.shift"):
        LP.LPIPS.from_state_dict(wrong)
    del vgg["features.17.bias"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    with pytest.raises(ValueError, match=re.escape("features.17.bias")):
        LP.LPIPS.from_files(tmp_path / "vgg16.pth", tmp_path / "vgg.pth")


def test_random_model_is_seeded_and_well_formed():
    a, b, c = LP.LPIPS.random(3), LP.LPIPS.random(3), LP.LPIPS.random(4)
    assert _same_model(a, (b.convs, b.biases, b.lins)) and not torch.equal(a.convs[5], c.convs[5])
    assert all(float(v.min()) >= 0 for v in a.lins) and [tuple(w.shape[:2]) for w in a.convs] == [(co, ci) for ci, co in LP.WIDTHS]


def test_packed_layout():
    """pack_conv3x3: element [cb][chunk][tap][k][n] is w[64 cb + n][8 chunk + k][tap], zero beyond Cin."""
    g = torch.Generator().manual_seed(7)
    for ci, co in ((3, 64), (20, 128)):
        w = torch.randn((co, ci, 3, 3), generator=g)
        chunks = (ci + 7) // 8
        p = LP.pack_conv3x3(w).reshape(co // 64, chunks, 9, 8, 64)
        assert p.numel() == (co // 64) * chunks * 4608
        for cb, chunk, tap, k, n in ((0, 0, 0, 0, 0), (co // 64 - 1, chunks - 1, 8, 2, 63), (0, chunks - 1, 4, 7, 17), (0, 0, 5, 1, 33)):
            c = 8 * chunk + k
            want = float(w[64 * cb + n, c, tap // 3, tap % 3]) if c < ci else 0.0
            assert float(p[cb, chunk, tap, k, n]) == want, (ci, co, cb, chunk, tap, k, n)
    with pytest.raises(ValueError):
        LP.pack_conv3x3(torch.zeros(65, 3, 3, 3))


def test_chunking_gives_the_same_values(model):
    a, b = LH.make_images(5, 3, 16, 16, lo=0.0, hi=1.0)
    masks = LH.make_masks(5, 3, 16, 16)
    whole = LP.lpips_views(model, a, b, masks)
    per_view = 4 * 2 * 64 * 16 * 16 * 8
    pieces = LP.lpips_views(model, list(a), list(b), [m[None, None].expand(1, 3, -1, -1) for m in masks], max_workspace_bytes=per_view)
    assert whole[0].shape == (3,) and torch.equal(whole[0], pieces[0]) and torch.equal(whole[1], pieces[1])
    assert not torch.equal(whole[0], whole[1])
    want = LH.lpips_oracle((model.convs, model.biases, model.lins), a, b, masks, normalize=True)
    assert rel(whole[0], want["plain"]) <= 2.0 ** -23 and rel(whole[1], want["masked"]) <= 2.0 ** -23
    with pytest.raises(ValueError):
        LP.lpips_views(model, a, b, core="triton")
    with pytest.raises(ValueError):
        LP.lpips_views(model, a, b, core="hip")  # CPU tensors: the HIP core refuses, it does not fall back


def test_evaluate_views_keys(model):
    from gscream_amd import metrics as M
    a, b = LH.make_images(6, 2, 16, 16, lo=0.0, hi=1.0)
    masks = [m[None, None].expand(1, 3, -1, -1) for m in LH.make_masks(6, 2, 16, 16)]
    full, per_view = M.evaluate_views(list(a), list(b), masks, ["x", "y"])
    assert list(full) == ["SSIM", "PSNR", "masked SSIM", "masked PSNR"] == list(per_view)
    full6, per6 = M.evaluate_views(list(a), list(b), masks, ["x", "y"], lpips=model)
    assert list(full6) == ["SSIM", "PSNR", "masked SSIM", "masked PSNR", "LPIPS", "masked LPIPS"] == list(per6)
    assert all(full6[k] == full[k] and per6[k] == per_view[k] for k in full)
    plain, masked = LP.lpips_views(model, list(a), list(b), masks)
    assert [per6["LPIPS"][n] for n in ("x", "y")] == plain.tolist() and [per6["masked LPIPS"][n] for n in ("x", "y")] == masked.tolist()
    assert full6["LPIPS"] == plain.mean().item() and full6["masked LPIPS"] == masked.mean().item()


def test_header_binding_and_library_agree(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_LPIPS_NORMALIZE"] == 1 and hdr.constants["GSR_LPIPS_SCALING"] == 2
    assert (LP.NORMALIZE, LP.SCALING) == (1, 2)
    assert hdr.functions["gsr_lpips_workspace_bytes"][0] == "size_t" and hdr.functions["gsr_lpips"][0] == "int"
    assert hdr.functions["gsr_conv3x3_relu"][0] == "int"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import arena_helpers as A
    table = A.header_table()
    for name in ("gsr_lpips_workspace_bytes", "gsr_lpips", "gsr_conv3x3_relu"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
        assert len(getattr(native_lib, name).argtypes) == len(table[name]), name
    # scalars, device pointers and the trailing stream only: nothing the arena proxy would have to be told is host memory
    assert not any(fn in ("gsr_lpips", "gsr_conv3x3_relu") for fn, _ in A.HOST_PARAMS)
    writable = [p[1] for p in table["gsr_lpips"] if p[2] and not p[3]]
    assert writable == ["workspace", "out_plain", "out_layers", "out_masked", "out_spatial", "stream"]
    assert [p[1] for p in table["gsr_conv3x3_relu"] if p[2] and not p[3]] == ["out", "stream"]
    assert hdr.constants["GSR_ABI_VERSION"] == 9


def test_argument_checks_without_a_gpu(native_lib):
    """Everything the calls reject, they reject before launching (there is no device here to launch on)."""
    size, err = native_lib.gsr_lpips_workspace_bytes, native_lib.gsr_last_error
    p = [256 * (i + 1) for i in range(12)]  # never dereferenced on the host

    def run(B=1, H=16, W=16, in0=p[0], in1=p[1], flags=0, cw=p[2], cb=p[3], lw=p[4], mask=p[5], sb=0, ws=p[6], plain=p[7], layers=p[8],
            masked=p[9], spatial=p[10]):
        return native_lib.gsr_lpips(B, H, W, in0, in1, flags, cw, cb, lw, mask, sb, ws, plain, layers, masked, spatial, None)

    for k in ("in0", "in1", "cw", "cb", "lw", "ws", "plain"):
        assert run(**{k: None}) == -1 and b"NULL" in err(), k
    for B in (0, -1, 32768, 1 << 30):
        assert run(B=B) == -1 and b"need 1 .. 32767" in err() and size(B, 16, 16) == 0, B
    for hw in ((15, 16), (16, 15), (0, 100), (100, -3)):
        assert run(H=hw[0], W=hw[1]) == -1 and b"need both >= 16" in err() and size(1, *hw) == 0, hw
    assert run(H=46341, W=46341) == -1 and b"too many pixels" in err()
    for flags in (2, 4, 3, -1):
        assert run(flags=flags) == -1 and b"unknown flag" in err(), flags
    assert run(sb=-1) == -1 and b"negative mask stride" in err()
    # the workspace: two buffers of 2B*64*H*W floats, then maps and partials, each piece on a 512-byte boundary
    for B, H, W in ((1, 16, 16), (2, 37, 53), (3, 96, 160), (1, 567, 1008)):
        got, buffers = size(B, H, W), 2 * (-(-2 * B * 64 * H * W * 4 // 512) * 512)
        assert got % 512 == 0 and buffers < got <= buffers + B * H * W * 8 + 11 * 512 + B * 4096, (B, H, W, got)
    assert 580e6 < size(1, 567, 1008) < 600e6

    def conv(B=1, Cin=64, Cout=64, H=5, W=7, x=p[0], w=p[1], b=p[2], out=p[3], flags=0):
        return native_lib.gsr_conv3x3_relu(B, Cin, Cout, H, W, x, w, b, out, flags, None)

    for k in ("x", "w", "b", "out"):
        assert conv(**{k: None}) == -1 and b"NULL" in err(), k
    for B in (0, -2, 65536):
        assert conv(B=B) == -1 and b"need 1 .. 65535" in err(), B
    for cc in ((0, 64), (64, 0), (64, 32), (64, 96), (-1, 64), (3, 65)):
        assert conv(Cin=cc[0], Cout=cc[1]) == -1 and b"multiple of 64" in err(), cc
    for hw in ((0, 7), (5, 0), (-1, 7)):
        assert conv(H=hw[0], W=hw[1]) == -1 and b"need both > 0" in err(), hw
    for flags in (4, 8, -1):
        assert conv(Cin=3, flags=flags) == -1 and b"unknown flag" in err(), flags
    assert conv(flags=1) == -1 and b"Cin = 3" in err()
