"""render_set's output frames on the HIP path: what train.py:710-848 does between the render and the PNG, as finished uint8 pictures
on the device, in HWC order, ready for one D2H copy and a PNG encoder -- or for gscream_amd.png (INTEGRATION U), which encodes them
where they are.

Integration is a handful of rebindings in render_set (INTEGRATION S):

    torchvision.utils.save_image(x, path)             ->  gscream_amd.frames.save_image(x, path)
    the spiral branch, :804-834                       ->  rgbd_frame(render, depth, uncertainty, normal, panels=True), one .cpu()
    the train / test branch, :776-800                 ->  view_frames(render, uncertainty, gt, depth, midas_depth, gt_mask), two .cpu()

The rules (include/gsraster.h has them in full); fp32, one rounding per operation, correctly rounded division and sqrt:

  quantise   q(x) = (uint8) trunc(min(max(x*255 + 0.5, 0), 255)), NaN -> 0 (a choice: the reference's conversion is unspecified there);
             clamp, where it applies, first: x := min(max(x, 0), 1)
  abs-diff   q(|clamp(a) - b|)                                                            the error map
  normal     s = (x*x + y*y) + z*z; r = max(sqrt(s), 1e-12); q((v/r + 1) / 2)             F.normalize and the map to [0, 1]
  stats      lo, hi = min, max of the depth; a00 .. b1 of compute_scale_and_shift in fp64, det == 0 -> scale = shift = 0, else the two
             quotients in fp64 rounded to fp32 once, scale := |scale|; lo2, hi2 over the panel [depth*scale + shift | target]
  CV map     i = trunc(255 (d - lo) / (hi - lo)); hi == lo or a non-finite lo / hi -> i = 0 (a choice: the reference has 0/0 there)
  MPL map    den = (float)((double) hi2 - (double) lo2); i = min(trunc(256 (v - lo2) / den), 255); RGBA = (lut[i], 255); hi2 == lo2 -> i = 0;
             a NaN in the panel -> every pixel (0, 0, 0, 0)

What pins what: the MPL map is pinned by matplotlib's imsave and the fit by train.py's compute_scale_and_shift
(tests/golden/ref_frames.npz); save_image's quantisation and the CV map are written rules.  The "viridis" table is matplotlib's own
bytes.  The "inferno" table is NOT pinned by a run of cv2 (it is not on this stack): it is matplotlib's listed colours rounded to
nearest, which is what OpenCV's table-to-bytes conversion does to the same colours; a caller with cv2 can pass
`cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_INFERNO)[:, 0, ::-1]` as a uint8 tensor on the device, made once (a
table on the host is copied to the device on every call, which stops the host).

The HIP path (gscream_amd/csrc/frames.hip; `last_path = "hip"`) takes fp32 tensors on a HIP device through their strides -- a flip, a
stride-0 channel and the interleaved [h*w, 3] normals are read in place, nothing is materialised -- launches on torch's current
stream, allocates its outputs and a workspace, reads nothing back and never synchronises.  Everything else -- CPU tensors, other
dtypes, `force_torch = True` -- takes a torch statement of the same rules (`last_path = "torch"`).  A missing library raises;
nothing falls back quietly."""
import json
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native

__all__ = ["Panel", "RgbdFrame", "ViewFrames", "colormap_lut", "compose", "frame_stats", "rgbd_frame", "save_image", "to_uint8", "view_frames"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last call took

MAX_PANELS = _native.FRAME_MAX_PANELS
MAX_FRAMES = 65535        # both calls: B
MAX_BYTES = 0x7FFFFF00    # both calls: H*W*4 below this
QUANT, QUANT_CLAMP, ABSDIFF, NORMAL, CMAP_CV, CMAP_MPL_ALIGNED, CMAP_MPL = range(7)  # GSR_FRAME_*
_CMAP_MODES = (CMAP_CV, CMAP_MPL_ALIGNED, CMAP_MPL)
_LUT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormaps.json")
_LUT_NAMES = ("inferno", "viridis")
_luts = {}


class Panel(NamedTuple):
    """One panel of `compose`: `src` is a [B, C, H, w] view (C = 3; C = 1 for the CMAP modes) read through its strides, `src2` the second
    image of ABSDIFF, `lut` a uint8 [256, 3] table for the CMAP modes, `flip` mirrors the panel left to right, `x0` is its first output
    column (None: where the panel before it ends)."""
    mode: int
    src: torch.Tensor
    src2: Optional[torch.Tensor] = None
    lut: Optional[torch.Tensor] = None
    flip: bool = False
    x0: Optional[int] = None


class RgbdFrame(NamedTuple):
    """rgbd [H, 4W, 3] and its four panels [H, W, 3], views of the same buffer."""
    rgbd: torch.Tensor
    render: torch.Tensor
    depth: torch.Tensor
    normal: torch.Tensor
    uncertainty: torch.Tensor


class ViewFrames(NamedTuple):
    """The five files of a train / test view: render, uncertainty, error, gt [H, W, 3] (views of `sheet` [H, 4W, 3]: one copy brings all
    four) and depth [H, 2W, 4] (aligned | MiDaS, RGBA); params [1, 8] = {lo, hi, scale, shift, lo2, hi2, 0, 0} stays on the device."""
    render: torch.Tensor
    uncertainty: torch.Tensor
    error: torch.Tensor
    gt: torch.Tensor
    depth: torch.Tensor
    sheet: torch.Tensor
    params: torch.Tensor


def load_colormaps():
    """gscream_amd/colormaps.json -> uint8 [2, 256, 3] (inferno, viridis; RGB).  The file is text: per table, rows of 16 colours as
    "rrggbb" hex digits."""
    with open(_LUT_FILE) as f:
        doc = json.load(f)
    table = np.stack([np.frombuffer(bytes.fromhex("".join(doc[name])), np.uint8).reshape(-1, 3) for name in _LUT_NAMES])
    if table.shape != (2, 256, 3):
        raise RuntimeError(f"{_LUT_FILE}: tables of {table.shape} (need [2, 256, 3])")
    return table


def colormap_lut(name, device=None):
    """"inferno" (rounded to nearest: the cv2 table, unpinned -- see the module text) or "viridis" (truncated: plt.imsave's bytes) as a
    uint8 [256, 3] RGB tensor on `device`, from gscream_amd/colormaps.json (tools/make_colormaps.py writes it); cached per device."""
    if name not in _LUT_NAMES:
        raise ValueError(f"colormap_lut: {name!r} (have {_LUT_NAMES})")
    device = torch.device("cpu" if device is None else device)
    key = (name, device)
    if key not in _luts:
        _luts[key] = torch.from_numpy(load_colormaps()[_LUT_NAMES.index(name)].copy()).to(device)
    return _luts[key]


def _hip_tensor(t):
    return t.is_cuda and t.dtype == torch.float32


# ---- the torch statement ----
def _quantise_torch(x, clamp=False):
    """fp32 -> uint8 by the quantise rule; each eager operation rounds once, torch.clamp keeps a NaN."""
    x = x.to(torch.float32)
    if clamp:
        x = torch.clamp(x, 0.0, 1.0)
    q = x * 255.0
    q = q + 0.5
    q = torch.clamp(q, 0.0, 255.0)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).to(torch.uint8)  # (.to(uint8) truncates)


def _stats_torch(depth, target=None, mask=None):
    """depth, target, mask [B, H, W] -> (stats [B, 8] fp64, params [B, 8] fp32) by the stats rule (torch's own summation order)."""
    B = depth.shape[0]
    d = depth.to(torch.float32).reshape(B, -1)
    stats = torch.zeros((B, 8), dtype=torch.float64, device=d.device)
    params = torch.zeros((B, 8), dtype=torch.float32, device=d.device)
    params[:, 0], params[:, 1] = d.amin(1), d.amax(1)
    if target is None:
        return stats, params
    y = target.to(torch.float32).reshape(B, -1)
    m = torch.ones_like(d) if mask is None else mask.to(torch.float32).reshape(B, -1)
    d64, y64, m64 = d.double(), y.double(), m.double()
    md = m64 * d64
    a00, a01, a11, b0, b1 = (md * d64).sum(1), md.sum(1), m64.sum(1), (md * y64).sum(1), (m64 * y64).sum(1)
    det = a00 * a11 - a01 * a01
    zero = det == 0
    safe = torch.where(zero, torch.ones_like(det), det)
    x0 = torch.where(zero, torch.zeros_like(det), (a11 * b0 - a01 * b1) / safe)
    x1 = torch.where(zero, torch.zeros_like(det), (-a01 * b0 + a00 * b1) / safe)
    stats = torch.stack([a00, a01, a11, b0, b1, det, x0, x1], 1)
    params[:, 2], params[:, 3] = x0.to(torch.float32).abs(), x1.to(torch.float32)
    aligned = d * params[:, 2:3]
    aligned = aligned + params[:, 3:4]
    panel = torch.cat([aligned, y], 1)
    params[:, 4], params[:, 5] = panel.amin(1), panel.amax(1)
    return stats, params


def _map_mpl_torch(v, lo, hi, lut):
    """v [B, 1, H, w], lo / hi [B, 1, 1, 1] -> uint8 [B, H, w, 4]."""
    den = (hi.double() - lo.double()).to(torch.float32)
    t = (v - lo) / den
    t = t * 256.0
    flat = hi == lo
    blank = torch.isnan(lo) | torch.isnan(hi) | (torch.isnan(t) & ~flat)
    i = torch.clamp(torch.where(torch.isnan(t), torch.zeros_like(t), t), 0.0, 255.0).to(torch.int64)  # (.to(int64) truncates)
    i = torch.where(flat, torch.zeros_like(i), i)
    rgb = lut.to(v.device)[i[:, 0]]
    out = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], -1)
    return torch.where(blank[:, 0, :, :, None], torch.zeros_like(out), out)


def _panel_torch(p, params):
    """One panel by the rules -> uint8 [B, H, w, 4]."""
    s = p.src.to(torch.float32)
    B = s.shape[0]
    col = (lambda k: None) if params is None else (lambda k: params[:, k].reshape(B, 1, 1, 1))
    if p.mode in (QUANT, QUANT_CLAMP):
        rgb = _quantise_torch(s, p.mode == QUANT_CLAMP)
    elif p.mode == ABSDIFF:
        rgb = _quantise_torch((torch.clamp(s, 0.0, 1.0) - p.src2.to(torch.float32)).abs())
    elif p.mode == NORMAL:
        x, y, z = s[:, 0:1], s[:, 1:2], s[:, 2:3]
        q = x * x
        q = q + y * y
        q = q + z * z
        r = torch.sqrt(q)
        r = torch.where(r < 1e-12, torch.full_like(r, 1e-12), r)  # max(r, 1e-12) that keeps a NaN
        c = s / r
        c = c + 1.0
        rgb = _quantise_torch(c / 2.0)
    elif p.mode == CMAP_CV:
        lo, hi = col(0), col(1)
        t = (s - lo) / (hi - lo)
        t = torch.clamp(255.0 * t, 0.0, 255.0)
        usable = (hi != lo) & torch.isfinite(lo) & torch.isfinite(hi) & ~torch.isnan(t)
        i = torch.where(usable, t, torch.zeros_like(t)).to(torch.int64)  # (.to(int64) truncates)
        rgb = p.lut.to(s.device)[i[:, 0]].permute(0, 3, 1, 2)
    else:
        v = s
        if p.mode == CMAP_MPL_ALIGNED:
            v = s * col(2)
            v = v + col(3)
        out = _map_mpl_torch(v, col(4), col(5), p.lut)
        return out.flip(2) if p.flip else out
    rgb = rgb.expand(-1, 3, -1, -1).permute(0, 2, 3, 1)
    out = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], -1)
    return out.flip(2) if p.flip else out


def _compose_torch(panels, spans, W_out, channels, params):
    B, _, H, _ = panels[0].src.shape
    out = torch.empty((B, H, W_out, channels), dtype=torch.uint8, device=panels[0].src.device)
    for p, (x0, w) in zip(panels, spans):
        out[:, :, x0:x0 + w] = _panel_torch(p, params)[..., :channels]
    return out


# ---- the calls ----
def _three(t, what):
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError(f"{what} is {tuple(t.shape)} (need [H, W] or [B, H, W])")
    return t


def frame_stats(depth, target=None, lsq_mask=None):
    """depth [H, W] or [B, H, W], target and lsq_mask (fp32; None = ones) alike or None -> (stats [B, 8] fp64 = {a00, a01, a11, b0, b1, det,
    x0, x1}, params [B, 8] fp32 = {lo, hi, scale, shift, lo2, hi2, 0, 0}) on the depth's device.  Without a target only lo and hi are set."""
    global last_path
    depth = _three(depth, "frame_stats: depth")
    if lsq_mask is not None and target is None:
        raise ValueError("frame_stats: an lsq_mask needs a target")
    others = []
    for t, what in ((target, "target"), (lsq_mask, "lsq_mask")):
        if t is not None:
            t = _three(t, f"frame_stats: {what}")
            if t.shape != depth.shape or t.device != depth.device:
                raise ValueError(f"frame_stats: {what} is {tuple(t.shape)} on {t.device}, depth is {tuple(depth.shape)} on {depth.device}")
        others.append(t)
    target, lsq_mask = others
    B, H, W = depth.shape
    if (force_torch or not all(_hip_tensor(t) for t in (depth, target, lsq_mask) if t is not None) or B == 0 or B > MAX_FRAMES or H * W == 0
            or H * W * 4 >= MAX_BYTES):
        last_path = "torch"
        return _stats_torch(depth, target, lsq_mask)
    last_path = "hip"
    dev = depth.device
    depth, target, lsq_mask = (None if t is None else t.contiguous() for t in (depth, target, lsq_mask))
    lib = _native.load()
    workspace = torch.empty(int(lib.gsr_frame_stats_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    stats = torch.empty((B, 8), dtype=torch.float64, device=dev)
    params = torch.empty((B, 8), dtype=torch.float32, device=dev)
    _native.run("gsr_frame_stats", dev, B, H, W, _native.ptr(depth), _native.ptr(target), _native.ptr(lsq_mask), _native.ptr(workspace),
                _native.ptr(stats), _native.ptr(params))
    return stats, params


def _check_panels(panels, width):
    """-> ([(x0, w)], W_out); ValueError unless the panels are well formed and tile [0, W_out) exactly."""
    if not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError(f"compose: {len(panels)} panels (need 1 .. {MAX_PANELS})")
    first = panels[0].src
    spans, at = [], 0
    for k, p in enumerate(panels):
        if p.mode not in range(7):
            raise ValueError(f"compose: panel {k} has the unknown mode {p.mode}")
        channels = 1 if p.mode in _CMAP_MODES else 3
        s = p.src
        if not isinstance(s, torch.Tensor) or s.dim() != 4 or s.shape[1] != channels or s.shape[0] != first.shape[0] or s.shape[2] != first.shape[2]:
            raise ValueError(f"compose: panel {k} (mode {p.mode}) has a src of {tuple(s.shape)} (need [{first.shape[0]}, {channels}, {first.shape[2]}, w])")
        if s.device != first.device or s.shape[3] == 0:
            raise ValueError(f"compose: panel {k} is empty or on {s.device}, panel 0 on {first.device}")
        if p.mode == ABSDIFF and (p.src2 is None or p.src2.shape != s.shape or p.src2.device != s.device):
            raise ValueError(f"compose: panel {k} is ABSDIFF: src2 has src's shape and device")
        if p.mode in _CMAP_MODES and (p.lut is None or tuple(p.lut.shape) != (256, 3) or p.lut.dtype != torch.uint8):
            raise ValueError(f"compose: panel {k} has a CMAP mode: lut is a uint8 [256, 3] tensor")
        x0 = at if p.x0 is None else int(p.x0)
        spans.append((x0, int(s.shape[3])))
        at = x0 + int(s.shape[3])
    W_out = max(x + w for x, w in spans) if width is None else int(width)
    nxt = 0
    for x0, w in sorted(spans):
        if x0 != nxt:
            raise ValueError(f"compose: a panel starts at column {x0} where {nxt} is next (the panels {'overlap' if x0 < nxt else 'leave a gap'})")
        nxt = x0 + w
    if nxt != W_out:
        raise ValueError(f"compose: the panels end at column {nxt} of {W_out}")
    return spans, W_out


def compose(panels, channels=3, params=None, width=None):
    """panels: 1 .. 8 `Panel`s that tile the output width exactly -> uint8 [B, H, W_out, channels] on their device.  params [B, 8] fp32 as
    frame_stats returns it; needed by the CMAP modes only.  channels = 4 adds alpha (255, or the MPL map's)."""
    global last_path
    panels = [p if isinstance(p, Panel) else Panel(*p) for p in panels]
    spans, W_out = _check_panels(panels, width)
    if channels not in (3, 4):
        raise ValueError(f"compose: channels={channels} (need 3 or 4)")
    B, _, H, _ = panels[0].src.shape
    dev = panels[0].src.device
    needs_params = any(p.mode in _CMAP_MODES for p in panels)
    if needs_params and (params is None or tuple(params.shape) != (B, 8) or params.device != dev):
        raise ValueError(f"compose: a CMAP mode needs params [{B}, 8] on {dev}")
    tensors = [t for p in panels for t in (p.src, p.src2) if t is not None]
    if (force_torch or not all(_hip_tensor(t) for t in tensors) or (needs_params and not (_hip_tensor(params) and params.is_contiguous()))
            or B == 0 or B > MAX_FRAMES or H == 0 or H * W_out * 4 >= MAX_BYTES):
        last_path = "torch"
        return _compose_torch(panels, spans, W_out, channels, params)
    last_path = "hip"
    table = (_native.FramePanel * len(panels))()
    keep = []  # what the table points into, referenced until the launch is enqueued
    for k, (p, (x0, w)) in enumerate(zip(panels, spans)):
        src, src2 = p.src, p.src2
        if src2 is not None and src2.stride() != src.stride():
            src, src2 = src.contiguous(), src2.contiguous()
        lut = None if p.lut is None else p.lut.to(dev).contiguous()
        keep += [src, src2, lut]
        sb, sc, sy, sx = src.stride()
        first = (w - 1) * sx if p.flip else 0  # the row's last element, walked backwards
        e = table[k]
        e.src = src.data_ptr() + 4 * first
        e.src2 = None if src2 is None else src2.data_ptr() + 4 * first
        e.lut = None if lut is None else lut.data_ptr()
        e.stride_b, e.stride_c, e.stride_y, e.stride_x = sb, sc, sy, (-sx if p.flip else sx)
        e.x0, e.width, e.mode = x0, w, p.mode
    out = torch.empty((B, H, W_out, channels), dtype=torch.uint8, device=dev)
    _native.run("gsr_frame_compose", dev, B, H, W_out, channels, len(panels), table, _native.ptr(params) if needs_params else None, _native.ptr(out))
    return out


# ---- render_set's pictures ----
def _image4(image, what):
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what}: a tensor")
    if image.dim() == 2:
        image = image[None]
    if image.dim() == 3:
        image = image[None]
    if image.dim() != 4 or image.shape[1] not in (1, 3):
        raise ValueError(f"{what} is {tuple(image.shape)} (need [C, H, W] or [B, C, H, W] with C = 1 or 3)")
    return image.expand(-1, 3, -1, -1)  # a one-channel image: stride 0, as make_grid repeats it


def _plane4(t, what):
    """[H, W], [1, H, W] or [1, 1, H, W] -> [1, 1, H, W]."""
    while t.dim() < 4:
        t = t[None]
    if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 1:
        raise ValueError(f"{what} is {tuple(t.shape)} (need [H, W] or [1, H, W])")
    return t


def to_uint8(image, clamp=False):
    """[C, H, W] or [B, C, H, W] with C = 1 or 3 -> uint8 [.., H, W, 3]: save_image's tensor half (make_grid's one-channel expansion,
    mul(255).add_(0.5).clamp_(0, 255), HWC order, uint8); clamp=True applies render_set's torch.clamp(x, 0, 1) first."""
    batched = isinstance(image, torch.Tensor) and image.dim() == 4
    out = compose([Panel(QUANT_CLAMP if clamp else QUANT, _image4(image, "to_uint8: image"))])
    return out if batched else out[0]


def save_image(tensor, path):
    """torchvision.utils.save_image(tensor, path) for a single image: to_uint8, one copy to the host, PIL's encoder."""
    from PIL import Image
    if tensor.dim() == 4:
        if tensor.shape[0] != 1:
            raise ValueError(f"save_image: a single image, not a batch of {tensor.shape[0]}")
        tensor = tensor[0]
    Image.fromarray(to_uint8(tensor).cpu().numpy()).save(path)


def _normal_panel(normal, H, W, flip):
    """[3, H, W]: the finished picture of normals.normal_map -> QUANT.  [1, 3, W, H]: what least_square_normal_regress_fast01 returns (the
    reference's view of its [h*w, 3] rows), or the [H*W, 3] rows themselves -> NORMAL, read in place through strides (1, 3 W, 3)."""
    if normal.dim() == 3 and tuple(normal.shape) == (3, H, W):
        return Panel(QUANT, normal[None], flip=flip)
    if normal.dim() == 4 and tuple(normal.shape) == (1, 3, W, H):
        normal = normal.permute(0, 2, 3, 1).reshape(H * W, 3)  # a view of the rows when the tensor is the function's own return
    if normal.dim() == 2 and tuple(normal.shape) == (H * W, 3):
        return Panel(NORMAL, normal.view(1, H, W, 3).permute(0, 3, 1, 2), flip=flip)
    raise ValueError(f"rgbd_frame: normal is {tuple(normal.shape)} (need [3, {H}, {W}], [1, 3, {W}, {H}] or [{H * W}, 3])")


def rgbd_frame(render, depth, uncertainty, normal, flip=True, lut=None, panels=False):
    """The rgbd picture of train.py:804-827: render | INFERNO depth | normal | uncertainty, each flipped left to right -> uint8
    [H, 4W, 3].  render [3, H, W] and uncertainty [1, H, W] are clamped to [0, 1] as render_set clamps them; depth [1, H, W] is
    normalised by its own min and max; normal is what normals.normal_map ([3, H, W], finished) or
    least_square_normal_regress_fast01 ([1, 3, W, H], normalised here) returns.  lut: a uint8 [256, 3] RGB table (default
    colormap_lut("inferno"): not pinned by cv2, see the module text).  panels=True returns RgbdFrame: the picture and its four panels
    -- the files render_set also saves alone -- as views of the one buffer, so nothing is composed twice."""
    render = _image4(render, "rgbd_frame: render")
    _, _, H, W = render.shape
    depth, uncertainty = _plane4(depth, "rgbd_frame: depth"), _plane4(uncertainty, "rgbd_frame: uncertainty")
    lut = colormap_lut("inferno", render.device) if lut is None else torch.as_tensor(lut).to(render.device)  # (no copy for a device table)
    _stats, params = frame_stats(depth[0])
    out = compose([Panel(QUANT_CLAMP, render, flip=flip), Panel(CMAP_CV, depth, lut=lut, flip=flip), _normal_panel(normal, H, W, flip),
                   Panel(QUANT_CLAMP, uncertainty.expand(-1, 3, -1, -1), flip=flip)], params=params)[0]
    if not panels:
        return out
    return RgbdFrame(out, *(out[:, k * W:(k + 1) * W] for k in range(4)))


def view_frames(render, uncertainty, gt, depth, midas_depth, gt_mask, lut=None):
    """The five files of a train / test view (train.py:776-800) -> ViewFrames.  render [3, H, W] and uncertainty [1, H, W] are clamped as
    render_set clamps them, error = |clamp(render) - gt|, gt [3, H, W]; the depth picture is plt.imsave(cmap="viridis") of
    [depth*scale + shift | midas_depth] with the fit of compute_scale_and_shift over 1 - gt_mask (one eager torch
    operation, as render_set forms it).  Then one stats call and one compose call per output shape."""
    render, gt = _image4(render, "view_frames: render"), _image4(gt, "view_frames: gt")
    depth, midas, mask = (_plane4(t, f"view_frames: {what}") for t, what in ((depth, "depth"), (midas_depth, "midas_depth"), (gt_mask, "gt_mask")))
    uncertainty = _plane4(uncertainty, "view_frames: uncertainty")
    W = render.shape[3]
    lut = colormap_lut("viridis", render.device) if lut is None else torch.as_tensor(lut).to(render.device)
    valid = 1 - mask.to(torch.float32)
    _stats, params = frame_stats(depth[0], midas[0], valid[0])
    sheet = compose([Panel(QUANT_CLAMP, render), Panel(QUANT_CLAMP, uncertainty.expand(-1, 3, -1, -1)), Panel(ABSDIFF, render, gt), Panel(QUANT, gt)])[0]
    picture = compose([Panel(CMAP_MPL_ALIGNED, depth, lut=lut), Panel(CMAP_MPL, midas, lut=lut)], channels=4, params=params)[0]
    return ViewFrames(*(sheet[:, k * W:(k + 1) * W] for k in range(4)), picture, sheet, params)
