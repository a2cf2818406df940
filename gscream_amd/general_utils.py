"""The picture loaders of utils/general_utils.py:35-75 on the HIP path: PILtoTorch, PILtoTorch_01mask and PILtoTorch_depth, which loadCam
(utils/camera_utils.py:19-102) calls for every image, mask and monocular depth map of a scene.

The reference resizes with PIL on the host (pil_image.resize(resolution): PIL's default filter, BICUBIC for L, RGB and F), applies
`/ 255.0`, `> 0` or nothing, permutes to CHW, and Camera.__init__ uploads the result.  Here the picture's bytes are uploaded once, the
resize runs on the device (gscream_amd.resize: PIL's rule, exact) and the last step is fused into the last launch: one upload and at
most two launches per picture, at equal sizes one.  The results are float32 [C, H, W] or [1, H, W] on `device`, so Camera.__init__'s
.to(data_device) and clamp cost nothing.

Same arguments as the reference plus a trailing device="cuda"; on a CPU device (and for the modes PIL treats specially: palette,
1-bit, alpha) the reference's own lines run on the host and the result is moved to `device`.  PILtoTorch_normal has no counterpart:
the reference feeds it np.random.rand ("fake one normal").

Integration (INTEGRATION X):

    from utils.general_utils import PILtoTorch, PILtoTorch_01mask, PILtoTorch_depth
    ->  from gscream_amd.general_utils import PILtoTorch, PILtoTorch_01mask, PILtoTorch_depth"""
import numpy as np
import torch

from . import _native, resize as _resize

__all__ = ["PILtoTorch", "PILtoTorch_01mask", "PILtoTorch_depth"]

last_path = None  # "hip" / "pil": the path the last loader took


def _chw(t):
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(dim=-1).permute(2, 0, 1)


def _device_route(pil_image, device):
    device = torch.device(device)
    route, resample = _resize.pil_route(pil_image.mode, None)
    return device, resample, route == "hip" and device.type == "cuda" and not _resize.force_host


def _load_u8(pil_image, resolution, device, epilogue, host_step):
    global last_path
    device, resample, on_device = _device_route(pil_image, device)
    if not on_device or pil_image.mode == "F":
        last_path = "pil"
        return _chw(host_step(np.array(pil_image.resize(resolution)))).to(device)
    last_path = "hip"
    return _resize.to_float_chw(torch.from_numpy(np.array(pil_image)).to(device), resolution, resample, epilogue)


def PILtoTorch(pil_image, resolution, device="cuda"):
    """pil_image.resize(resolution) / 255.0 as float32 [C, H, W] ([1, H, W] for one channel)."""
    return _load_u8(pil_image, resolution, device, _native.RESIZE_DIV255, lambda a: torch.from_numpy(a) / 255.0)


def PILtoTorch_01mask(pil_image, resolution, device="cuda"):
    """(pil_image.resize(resolution) > 0) as float32 [C, H, W] ([1, H, W] for one channel)."""
    return _load_u8(pil_image, resolution, device, _native.RESIZE_GT0, lambda a: torch.from_numpy((a > 0).astype(np.float32)))


def PILtoTorch_depth(pil_image, resolution, device="cuda"):
    """pil_image.resize(resolution) as float32 [1, H, W]: a mode-F depth map is resized on the device; other modes take PIL on the host
    and the reference's astype(np.float32)."""
    global last_path
    device, resample, on_device = _device_route(pil_image, device)
    if not on_device or pil_image.mode != "F":
        last_path = "pil"
        return _chw(torch.from_numpy(np.array(pil_image.resize(resolution)).astype(np.float32))).to(device)
    last_path = "hip"
    return _resize.resize(torch.from_numpy(np.array(pil_image)).to(device), resolution, resample)[None]
