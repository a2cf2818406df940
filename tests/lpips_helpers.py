"""An fp64 oracle of the LPIPS rule of include/gsraster.h, written independently of gscream_amd/lpips.py: the convolution is
unfold + matmul (not conv2d), the pool a reshape and amax, the head explicit sums, torch's bilinear rule explicit index arithmetic and
gathers (not F.interpolate, against which it is checked once on the CPU by tests/test_lpips.py), the masked mean a selection.
Everything runs on the CPU in float64 on the fp32 inputs as they are.  Also the seeded generators of weights and images."""
import torch
import torch.nn.functional as F

WIDTHS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
          (512, 512), (512, 512), (512, 512))
PAIRS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512))  # the eight distinct layers
GROUPS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


# ---- generators ----
def make_weights(seed):
    """(13 conv weights, 13 biases, 5 lin vectors) in fp32: He-normal weights, biases of sigma 0.05, lin weights uniform in [0, 1/C)."""
    g = torch.Generator().manual_seed(1000 + int(seed))
    convs = [(torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float() for ci, co in WIDTHS]
    biases = [(0.05 * torch.randn((co,), generator=g, dtype=torch.float64)).float() for _, co in WIDTHS]
    lins = [(torch.rand((c,), generator=g, dtype=torch.float64) / c).float() for c in TAP_CHANNELS]
    return convs, biases, lins


def make_images(seed, B, H, W, lo=-1.0, hi=1.0):
    """Two [B,3,H,W] fp32 batches in [lo, hi): a smooth pattern plus noise, the second a perturbed copy of the first."""
    g = torch.Generator().manual_seed(2000 + int(seed))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    phase = torch.rand((B, 3, 1, 1), generator=g, dtype=torch.float64) * 6.28
    base = 0.5 + 0.3 * torch.sin(0.37 * xx + phase) * torch.cos(0.23 * yy - phase) + 0.2 * (torch.rand((B, 3, H, W), generator=g, dtype=torch.float64) - 0.5)
    other = base + 0.15 * (torch.rand((B, 3, H, W), generator=g, dtype=torch.float64) - 0.5)
    to = lambda t: (lo + (hi - lo) * t.clamp(0.0, 1.0 - 1e-7)).float()
    return to(base), to(other)


def make_masks(seed, B, H, W):
    """[B,H,W] bool, a different rectangle plus speckle per view."""
    g = torch.Generator().manual_seed(3000 + int(seed))
    m = torch.rand((B, H, W), generator=g) < 0.2
    for b in range(B):
        m[b, (b + 1) * H // (B + 2):, : W - b * W // (B + 1) // 2] |= True
    return m


# ---- the oracle ----
def conv_oracle(x, w, b, with_scale=False):
    """relu(conv3x3(x) + b), zero pad 1, in fp64 by unfold + matmul.  with_scale: also sum|w||x| + |b| per output element (the scale of
    the forward error bound of an fma chain)."""
    x, w, b = x.double(), w.double(), b.double()
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    cols = F.unfold(x, 3, padding=1)  # [N, Cin*9, H*W], rows ordered (ci, ky, kx) as w.reshape(Cout, Cin*9)
    y = (w.reshape(Cout, Cin * 9) @ cols + b.view(1, Cout, 1)).reshape(N, Cout, H, W)
    out = torch.where(y < 0, torch.zeros_like(y), y)
    if not with_scale:
        return out
    scale = (w.abs().reshape(Cout, Cin * 9) @ cols.abs() + b.abs().view(1, Cout, 1)).reshape(N, Cout, H, W)
    return out, scale


def pool_oracle(x):
    N, C, H, W = x.shape
    return x[:, :, : H // 2 * 2, : W // 2 * 2].reshape(N, C, H // 2, 2, W // 2, 2).amax((3, 5))


def scaling_oracle(x, normalize=False):
    x = x.double()
    if normalize:
        x = 2.0 * x - 1.0
    return (x - torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)


def head_oracle(f0, f1, lin):
    """[B,C,h,w] x 2, [C] -> m [B,h,w]."""
    B, C = f0.shape[:2]
    n0 = torch.zeros_like(f0[:, 0])
    n1 = torch.zeros_like(n0)
    for c in range(C):
        n0 = n0 + f0[:, c] * f0[:, c]
        n1 = n1 + f1[:, c] * f1[:, c]
    n0, n1 = n0.sqrt() + 1e-10, n1.sqrt() + 1e-10
    m = torch.zeros_like(n0)
    for c in range(C):
        d = f0[:, c] / n0 - f1[:, c] / n1
        m = m + float(lin[c]) * (d * d)
    return m


def _axis(out, size):
    scale = size / out
    src = ((torch.arange(out, dtype=torch.float64) + 0.5) * scale - 0.5).clamp(min=0.0)
    i0 = src.floor().long().clamp(max=size - 1)
    i1 = (i0 + 1).clamp(max=size - 1)
    t = src - i0.double()
    return i0, i1, t


def bilinear_oracle(m, H, W):
    """torch's Upsample(size=(H,W), mode='bilinear', align_corners=False) of m [B,h,w], in fp64."""
    y0, y1, ty = _axis(H, m.shape[1])
    x0, x1, tx = _axis(W, m.shape[2])
    ty, tx = ty.view(1, H, 1), tx.view(1, 1, W)
    top = (1 - tx) * m[:, y0][:, :, x0] + tx * m[:, y0][:, :, x1]
    bot = (1 - tx) * m[:, y1][:, :, x0] + tx * m[:, y1][:, :, x1]
    return (1 - ty) * top + ty * bot


def masked_mean_oracle(spatial, mask):
    """[B,H,W] fp64, bool [B,H,W] (or None = all) -> [B]; an empty selection gives NaN."""
    if mask is None:
        return spatial.reshape(spatial.shape[0], -1).mean(1)
    return torch.stack([spatial[b][mask[b]].sum() / float(mask[b].sum()) if mask[b].any() else spatial.new_tensor(float("nan"))
                        for b in range(spatial.shape[0])])


def lpips_oracle(weights, in0, in1, mask=None, normalize=False):
    """-> {"plain" [B], "layers" [B,5], "masked" [B], "spatial" [B,H,W], "maps": the five m_l} in fp64."""
    convs, biases, lins = weights
    B, _, H, W = in0.shape
    x = scaling_oracle(torch.cat([in0, in1]), normalize)
    means, maps, spatial = [], [], None
    for l, group in enumerate(GROUPS):
        if l:
            x = pool_oracle(x)
        for i in group:
            x = conv_oracle(x, convs[i], biases[i])
        m = head_oracle(x[:B], x[B:], lins[l].double())
        maps.append(m)
        means.append(m.reshape(B, -1).mean(1))
        up = bilinear_oracle(m, H, W)
        spatial = up if spatial is None else spatial + up
    layers = torch.stack(means, 1)
    if mask is not None and mask.dim() == 2:
        mask = mask[None].expand(B, H, W)
    return {"plain": layers.sum(1), "layers": layers, "masked": masked_mean_oracle(spatial, mask), "spatial": spatial, "maps": maps}


def deviation(got, want):
    """max |got - want| over a quantity, NaN where both are NaN counting as 0."""
    got, want = got.double().cpu(), want.double().cpu()
    both_nan = got.isnan() & want.isnan()
    d = torch.where(both_nan, torch.zeros_like(got), (got - want).abs())
    return float(d.max()) if d.numel() else 0.0
