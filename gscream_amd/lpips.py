"""LPIPS on the HIP path: the third metric of the reference's evaluate() (train.py:905-987), plain and masked, from one VGG-16 pass.

    from gscream_amd.lpips import LPIPS, lpips_views
    lpips_fn = LPIPS.from_module(lpips.LPIPS(net='vgg'))                   # for: lpips_fn = lpips.LPIPS(net='vgg').to('cuda')
    spatial  = LPIPS.from_module(lpips.LPIPS(net='vgg'), spatial=True)     # for: loss_fn_vgg_spatial = lpips.LPIPS(net='vgg', spatial=True)
    plain, masked = lpips_views(lpips_fn, renders, gts, masks)             # for: train.py:948,952-953, every view in one call

`LPIPS(weights, spatial=False)` keeps the package's call, `forward(in0, in1, retPerLayer=False, normalize=False)`, and its return
shapes ([B,1,1,1], or [B,1,H,W] when spatial).  The rule (include/gsraster.h has it in full) is LPIPS v0.1, net='vgg', lpips=True,
eval mode: the scaling layer, thirteen 3x3 convolutions with bias and ReLU and four 2x2 max-pools, five taps, unit normalisation over
the channels with eps 1e-10, squared difference, the bias-free 1x1 `lin` convolution, spatial mean (plain) or bilinear upsampling
(spatial), the sum over the taps.

The rule is pinned AS WRITTEN ONLY.  Neither the `lpips` package nor torchvision nor any VGG or LPIPS weights are on this stack, so
no run of the package stands behind the rule, and the key layouts the loaders below accept are written down from memory of the
package and torchvision and are unpinned in the same way.  Users bring their own weights; tests use seeded random weights at the
real VGG-16 widths.

The HIP path (gscream_amd/csrc/lpips.hip; `last_path = "hip"`) takes fp32, contiguous tensors on a HIP device with H, W >= 16: the
convolutions are fp32 fma chains on the f32 matrix cores, the head and every sum are fp64.  It launches on torch's current stream,
allocates its workspace and outputs, reads nothing back and never synchronises.  CPU tensors, other dtypes and `force_torch = True`
take `_lpips_torch(..., dtype=torch.float64)`, a torch statement of the same rule rounded to fp32 at the end (`last_path = "torch"`).
A missing library raises; nothing falls back quietly."""
import torch
import torch.nn.functional as F

from . import _native

__all__ = ["LPIPS", "lpips_views", "pack_conv3x3", "conv3x3_relu"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last call took

NORMALIZE, SCALING = _native.LPIPS_NORMALIZE, _native.LPIPS_SCALING
CONV_KC, CONV_NB = 8, 64   # LPIPS_CONV_KC, LPIPS_CONV_NB: the packed layout of include/gsraster.h
WIDTHS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
          (512, 512), (512, 512), (512, 512))
GROUP_END = (1, 3, 6, 9, 12)           # the layer whose ReLU output is tap l
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
MIN_SIZE, MAX_VIEWS = 16, 32767
DEFAULT_WORKSPACE_CAP = 8 << 30
#: torchvision's vgg16().features indices of the 13 convolutions, and where the package keeps them (net.sliceK.N) -- from memory of
#: both, unpinned by any run of either on this stack
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)


def pack_conv3x3(weight):
    """[Cout,Cin,3,3] -> the flat [Cout/64][ceil(Cin/8)][9][8][64] fp32 blob gsr_conv3x3_relu reads (zeros where ci >= Cin)."""
    Cout, Cin = weight.shape[:2]
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or Cout % CONV_NB:
        raise ValueError(f"pack_conv3x3: weight is {tuple(weight.shape)} (need [Cout,Cin,3,3] with Cout a multiple of {CONV_NB})")
    chunks = (Cin + CONV_KC - 1) // CONV_KC
    w = weight.detach().to(torch.float32).reshape(Cout, Cin, 9)
    w = F.pad(w, (0, 0, 0, chunks * CONV_KC - Cin))
    w = w.reshape(Cout // CONV_NB, CONV_NB, chunks, CONV_KC, 9).permute(0, 2, 4, 3, 1)
    return w.contiguous().reshape(-1)


def conv3x3_relu(x, packed, bias, flags=0):
    """One layer on the HIP path: x [B,Cin,H,W] fp32 on a HIP device -> relu(conv3x3(x) + bias) [B,Cout,H,W]."""
    B, Cin, H, W = x.shape
    Cout = bias.numel()
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    _native.run("gsr_conv3x3_relu", x.device, B, Cin, Cout, H, W, _native.ptr(x), _native.ptr(packed), _native.ptr(bias), _native.ptr(out),
                int(flags))
    return out


def _want(sd, key, shape):
    if key not in sd:
        raise ValueError(f"LPIPS weights: missing key {key!r}")
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"LPIPS weights: key {key!r} is {got}, need {tuple(shape)}")
    return t.detach()


def _check_scaling(sd, prefix=""):
    for name, want in (("shift", SHIFT), ("scale", SCALE)):
        key = f"{prefix}scaling_layer.{name}"
        if key in sd:
            got = sd[key].detach().reshape(-1).to(torch.float32).cpu()
            if got.numel() != 3 or not torch.equal(got, torch.tensor(want, dtype=torch.float32)):
                raise ValueError(f"LPIPS weights: key {key!r} is {got.tolist()}, the rule has {list(want)}")


def _lin_keys(sd, prefix=""):
    """lin{l}.model.1.weight [1,C,1,1] (the `lins.{l}.` duplicates a module's state_dict carries are ignored)."""
    return [_want(sd, f"{prefix}lin{l}.model.1.weight", (1, c, 1, 1)).reshape(c) for l, c in enumerate(TAP_CHANNELS)]


class LPIPS:
    """weights = (convs, biases, lins): 13 [Cout,Cin,3,3], 13 [Cout] and 5 [C] tensors.  The fp32 copies, the packed blob of the HIP
    path and the fp64 copies of the torch path are made per device on first use and kept."""

    def __init__(self, weights, spatial=False):
        convs, biases, lins = weights
        if len(convs) != 13 or len(biases) != 13 or len(lins) != 5:
            raise ValueError("LPIPS: weights are (13 convolution weights, 13 biases, 5 lin vectors)")
        for i, (ci, co) in enumerate(WIDTHS):
            if tuple(convs[i].shape) != (co, ci, 3, 3) or tuple(biases[i].shape) != (co,):
                raise ValueError(f"LPIPS: convolution {i} is {tuple(convs[i].shape)} / {tuple(biases[i].shape)}, need {(co, ci, 3, 3)} / {(co,)}")
        for l, c in enumerate(TAP_CHANNELS):
            if lins[l].numel() != c:
                raise ValueError(f"LPIPS: lin {l} has {lins[l].numel()} weights, need {c}")
        self.convs = [w.detach().to(torch.float32).contiguous() for w in convs]
        self.biases = [b.detach().to(torch.float32).contiguous() for b in biases]
        self.lins = [v.detach().to(torch.float32).reshape(-1).contiguous() for v in lins]
        self.spatial = bool(spatial)
        self._cache = {}
        dev = self.convs[0].device
        if dev.type == "cuda":
            self.packed(dev)  # packed once, at construction, off the hot path

    # -- constructors
    @classmethod
    def from_state_dict(cls, sd, spatial=False):
        """The package's layout: net.slice{1..5}.{N}.weight / .bias with torchvision's indices N, lin{0..4}.model.1.weight
        ([1,C,1,1]; duplicates under lins.N. are ignored), scaling_layer.shift / .scale checked against the rule if present."""
        convs, biases = [], []
        for (ci, co), n, s in zip(WIDTHS, FEATURE_INDEX, SLICE_OF):
            convs.append(_want(sd, f"net.slice{s}.{n}.weight", (co, ci, 3, 3)))
            biases.append(_want(sd, f"net.slice{s}.{n}.bias", (co,)))
        _check_scaling(sd)
        return cls((convs, biases, _lin_keys(sd)), spatial)

    @classmethod
    def from_module(cls, module, spatial=None):
        """Adopt a real lpips.LPIPS instance by its state_dict(); `spatial` defaults to the module's."""
        return cls.from_state_dict(module.state_dict(), bool(getattr(module, "spatial", False)) if spatial is None else spatial)

    @classmethod
    def from_files(cls, vgg16_path, lin_path, spatial=False, map_location="cpu"):
        """torchvision's vgg16 checkpoint (features.N.weight / features.N.bias) plus the package's weights/v0.1/vgg.pth."""
        vgg, lin = torch.load(vgg16_path, map_location=map_location), torch.load(lin_path, map_location=map_location)
        convs = [_want(vgg, f"features.{n}.weight", (co, ci, 3, 3)) for (ci, co), n in zip(WIDTHS, FEATURE_INDEX)]
        biases = [_want(vgg, f"features.{n}.bias", (co,)) for (ci, co), n in zip(WIDTHS, FEATURE_INDEX)]
        _check_scaling(lin)
        return cls((convs, biases, _lin_keys(lin)), spatial)

    @classmethod
    def random(cls, seed=0, device="cpu", spatial=False):
        """He-normal convolution weights, small biases, non-negative lin weights; for tests and tools/lpips_bench.py."""
        g = torch.Generator().manual_seed(int(seed))
        convs = [torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (9 * ci)) ** 0.5 for ci, co in WIDTHS]
        biases = [0.05 * torch.randn((co,), generator=g) for _, co in WIDTHS]
        lins = [torch.rand((c,), generator=g) / c for c in TAP_CHANNELS]
        return cls(([w.to(device) for w in convs], [b.to(device) for b in biases], [v.to(device) for v in lins]), spatial)

    # -- per-device copies
    def weights(self, device, dtype=torch.float32):
        key = (str(device), dtype)
        if key not in self._cache:
            self._cache[key] = tuple([t.to(device=device, dtype=dtype) for t in group] for group in (self.convs, self.biases, self.lins))
        return self._cache[key]

    def packed(self, device):
        """(conv_weights, conv_bias, lin_weights) of gsr_lpips on `device`."""
        key = (str(device), "packed")
        if key not in self._cache:
            convs, biases, lins = self.weights(device)
            self._cache[key] = (torch.cat([pack_conv3x3(w) for w in convs]), torch.cat(biases), torch.cat(lins))
        return self._cache[key]

    def to(self, device):
        self.convs, self.biases, self.lins = ([t.to(device) for t in group] for group in (self.convs, self.biases, self.lins))
        if torch.device(device).type == "cuda":
            self.packed(torch.device(device))
        return self

    cuda = lambda self, device="cuda": self.to(device)  # noqa: E731
    eval = lambda self: self  # noqa: E731

    # -- the package's call
    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        in0, in1 = _images(in0, in1)
        r = _run(self, in0, in1, None, normalize, spatial=self.spatial, layer_maps=self.spatial and retPerLayer)
        B, _, H, W = in0.shape
        if self.spatial:
            val = r["spatial"].reshape(B, 1, H, W)
            layers = [m.reshape(B, 1, H, W) for m in r["layer_maps"]] if retPerLayer else None
        else:
            val = r["plain"].reshape(B, 1, 1, 1)
            layers = [r["layers"][:, l].reshape(B, 1, 1, 1) for l in range(5)]
        return (val, layers) if retPerLayer else val

    __call__ = forward


# ---- arguments ----
def _images(in0, in1):
    if not (isinstance(in0, torch.Tensor) and isinstance(in1, torch.Tensor)):
        raise TypeError("lpips: in0 and in1 are tensors")
    if in0.dim() == 3:
        in0 = in0[None]
    if in1.dim() == 3:
        in1 = in1[None]
    if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
        raise ValueError(f"lpips: in0 is {tuple(in0.shape)}, in1 is {tuple(in1.shape)} (need equal [3,H,W] or [B,3,H,W])")
    if in0.shape[2] < MIN_SIZE or in0.shape[3] < MIN_SIZE:
        raise ValueError(f"lpips: images of {tuple(in0.shape[2:])} (need H, W >= {MIN_SIZE}: four 2x2 pools)")
    if in0.device != in1.device:
        raise ValueError(f"lpips: in0 is on {in0.device}, in1 on {in1.device}")
    return in0, in1


def _mask3(mask, B, H, W, device):
    """A bool mask [H,W], [1,H,W], [B,H,W], [B,1,H,W] or [B,C,H,W] (the first channel speaks, as evaluate()'s masks[idx][0,0]) ->
    a [B,H,W] view, stride 0 over the views where it is one mask for all."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise TypeError("lpips: the mask is a torch.bool tensor")
    if mask.device != device:
        raise ValueError(f"lpips: the mask is on {mask.device}, the images on {device}")
    if mask.dim() == 4:
        mask = mask[:, 0]
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or tuple(mask.shape[1:]) != (H, W) or mask.shape[0] not in (1, B):
        raise ValueError(f"lpips: the mask is {tuple(mask.shape)} (need [H,W], [1,H,W], [B,H,W] or [B,C,H,W] for {B} images of {(H, W)})")
    return mask.expand(B, H, W)


def _hip_tensor(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


# ---- the torch statement ----
def _lpips_torch(model, in0, in1, mask=None, normalize=False, dtype=torch.float64, layer_maps=False, out_dtype=torch.float32):
    """The rule in torch, every step in `dtype`, the results rounded to fp32 at the end: {"plain" [B], "layers" [B,5], "masked" [B],
    "spatial" [B,H,W]} (+ "layer_maps": the five upsampled maps).  dtype=float64 is the product's fallback; dtype=float32 is the eager
    statement tools/lpips_bench.py times and the GPU tests measure the fp32 error scale with.  out_dtype=float64 leaves the results
    unrounded (the tests hold them against their oracle).  Synchronises nowhere."""
    in0, in1 = _images(in0, in1)
    B, _, H, W = in0.shape
    m3 = _mask3(mask, B, H, W, in0.device)
    convs, biases, lins = model.weights(in0.device, dtype)
    x = torch.cat([in0, in1]).to(dtype)
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    x = (x - shift) / scale
    means, maps, layer = [], [], 0
    for l in range(5):
        if l:
            x = F.max_pool2d(x, 2, 2)
        while layer <= GROUP_END[l]:
            x = F.relu(F.conv2d(x, convs[layer], biases[layer], padding=1))
            layer += 1
        f = x / (torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)) + 1e-10)
        d = (f[:B] - f[B:]) ** 2
        m = (d * lins[l].view(1, -1, 1, 1)).sum(1, keepdim=True)
        means.append(m.mean((1, 2, 3)))
        maps.append(F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)[:, 0])
    layers = torch.stack(means, 1)
    plain = means[0]
    spatial = maps[0]
    for l in range(1, 5):
        plain = plain + means[l]
        spatial = spatial + maps[l]
    if m3 is None:
        masked = spatial.to(torch.float64).mean((1, 2))
    else:  # selected, not multiplied
        masked = torch.where(m3, spatial, spatial.new_zeros(())).to(torch.float64).sum((1, 2)) / m3.sum((1, 2)).to(torch.float64)
    out = {"plain": plain.to(out_dtype), "layers": layers.to(out_dtype), "masked": masked.to(out_dtype), "spatial": spatial.to(out_dtype)}
    if layer_maps:
        out["layer_maps"] = [m.to(out_dtype) for m in maps]
    return out


# ---- the call ----
def _workspace_bytes(B, H, W):
    return int(_native.load().gsr_lpips_workspace_bytes(B, H, W))


def _lpips_hip(model, in0, in1, m3, normalize, spatial):
    B, _, H, W = in0.shape
    dev = in0.device
    cw, cb, lw = model.packed(dev)
    if m3 is not None and (m3.stride(2) != 1 or m3.stride(1) != W or m3.stride(0) < 0):
        m3 = m3.contiguous()
    workspace = torch.empty(_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    plain = torch.empty((B,), dtype=torch.float32, device=dev)
    layers = torch.empty((B, 5), dtype=torch.float32, device=dev)
    masked = torch.empty((B,), dtype=torch.float32, device=dev)
    smap = torch.empty((B, H, W), dtype=torch.float32, device=dev) if spatial else None
    mp, sb = (None, 0) if m3 is None else (_native.ptr(m3), m3.stride(0))
    _native.run("gsr_lpips", dev, B, H, W, _native.ptr(in0), _native.ptr(in1), NORMALIZE if normalize else 0, _native.ptr(cw), _native.ptr(cb),
                _native.ptr(lw), mp, sb, _native.ptr(workspace), _native.ptr(plain), _native.ptr(layers), _native.ptr(masked),
                None if smap is None else _native.ptr(smap))
    return {"plain": plain, "layers": layers, "masked": masked, "spatial": smap}


def _run(model, in0, in1, mask, normalize, spatial=True, layer_maps=False, core=None):
    """-> the dict of _lpips_torch ("spatial" is None on the HIP path unless asked for)."""
    global last_path
    B, _, H, W = in0.shape
    m3 = _mask3(mask, B, H, W, in0.device)
    capable = _hip_tensor(in0) and _hip_tensor(in1) and 0 < B <= MAX_VIEWS
    if core == "hip" and not capable:
        raise ValueError("lpips: core='hip' takes fp32, contiguous tensors on a HIP device")
    if not (capable and (core == "hip" or (core is None and not force_torch))):
        last_path = "torch"
        return _lpips_torch(model, in0, in1, m3, normalize, torch.float64, layer_maps)
    if layer_maps:
        raise NotImplementedError("lpips: the HIP path returns the summed spatial map, not the five upsampled maps "
                                  "(retPerLayer with spatial=True: set gscream_amd.lpips.force_torch)")
    last_path = "hip"
    return _lpips_hip(model, in0, in1, m3, normalize, spatial)


#: lpips_views takes the HIP core by default for calls of at least this many views.  Measured at 567x1008 (tools/lpips_bench.py,
#: profiles/lpips_timing.json, INTEGRATION W): 8 views in one call 7.89 ms per view against 8.66 ms for the eager fp32 torch statement on
#: the same device -- the HIP path wins; ONE view 10.67 ms against 9.09 ms -- it loses (the 70x126 and 35x63 stages do not fill the
#: machine from two images).  Between the two points nothing is measured, so fewer than 8 views take the losing side's rule: core="torch".
HIP_MIN_VIEWS = 8


def _stack(images):
    return torch.cat([t[None] if t.dim() == 3 else t for t in images]) if isinstance(images, (list, tuple)) else images


def _stack_masks(masks):
    if not isinstance(masks, (list, tuple)):
        return masks
    planes = []
    for m in masks:
        while m.dim() > 2:
            m = m[0]
        planes.append(m[None])
    return torch.cat(planes)


def lpips_views(model, renders, gts, masks=None, normalize=True, max_workspace_bytes=DEFAULT_WORKSPACE_CAP, core=None):
    """train.py:948 and :952-953 for every view at once: lists (or [B,3,H,W] stacks) of equally sized images in [0, 1] and of bool
    masks ([H,W], or evaluate()'s [1,C,H,W] whose [0,0] plane speaks) -> ([B] LPIPS, [B] masked LPIPS) on the images' device, from one
    VGG pass per pair.  normalize=True is the 2*x-1 evaluate() writes.  The views go through in chunks whose workspace stays under
    `max_workspace_bytes` (at 567x1008 the first group's activations are 146 MB per image, 585 MB of workspace per view).  core:
    "hip" / "torch" force one; None = "hip" for fp32 HIP tensors of at least HIP_MIN_VIEWS = 8 views (where it measured faster than
    eager fp32 torch) and "torch", the fp64 statement, for fewer views (at one view it measured slower) and everywhere else.
    Without masks the masked value is the mean of the spatial map."""
    if core not in (None, "hip", "torch"):
        raise ValueError(f"lpips_views: core={core!r} (need None, 'hip' or 'torch')")
    in0, in1 = _images(_stack(renders), _stack(gts))
    B, _, H, W = in0.shape
    m3 = None if masks is None else _mask3(_stack_masks(masks), B, H, W, in0.device)
    if core is None:
        core = "hip" if (not force_torch and _hip_tensor(in0) and _hip_tensor(in1) and B >= HIP_MIN_VIEWS) else "torch"
    if core == "hip":
        per = _workspace_bytes(1, H, W)
        step = max(1, min(B, MAX_VIEWS, int(max_workspace_bytes) // max(per, 1)))
    else:  # the torch statement holds about 3.5 activation buffers of 2*64*H*W values of 8 bytes per view
        step = max(1, min(B, int(max_workspace_bytes) // (4 * 2 * 64 * H * W * 8)))
    plain, masked = [], []
    for b0 in range(0, B, step):
        b1 = min(b0 + step, B)
        r = _run(model, in0[b0:b1], in1[b0:b1], None if m3 is None else m3[b0:b1], normalize, spatial=False, core=core)
        plain.append(r["plain"])
        masked.append(r["masked"])
    return (plain[0], masked[0]) if len(plain) == 1 else (torch.cat(plain), torch.cat(masked))
