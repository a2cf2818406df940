"""An independent per-anchor restatement of the cross-attention anchor sampler, for the anchor-sampler tests: one Python loop over
the anchors, written from the rules (valid / pixel / sampled / label / classes / ok / min_num / smallest (key, index)), not from
the reference's tensor expressions and not from the code under test.  Plus the scenes the tests share.

The reference's block (train.py:436-511) is inline in training() and cannot be executed offline, so no reference-run vector
exists: this loop is the yardstick for the semantics."""
import math

import numpy as np
import torch

M32 = 0xFFFFFFFF


def mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def key(seed, i):
    """The documented key function on Python integers."""
    s_lo, s_hi = seed & M32, (seed >> 32) & M32
    x = mix((((i & M32) ^ s_lo) + s_hi) & M32)
    return mix(((x + s_lo) & M32) ^ s_hi)


def classify_loop(visible, x, y, gt, rect):
    """-> (fg, bg, n_sampled): index lists in ascending order.  x, y, gt: float32 numpy arrays."""
    h, w = gt.shape
    min_y, max_y, min_x, max_x = rect
    fg, bg, n_sampled = [], [], 0
    for a in range(len(visible)):
        xa, ya = np.float32(x[a]), np.float32(y[a])
        if not visible[a]:
            continue
        if not (np.float32(0) < xa < np.float32(w) and np.float32(0) < ya < np.float32(h)):  # False for NaN
            continue
        px, py = int(math.trunc(float(xa))), int(math.trunc(float(ya)))
        if not (min_y <= py < max_y and min_x <= px < max_x):
            continue
        n_sampled += 1
        label = int(math.trunc(float(gt[py, px])))
        if label > 0:
            fg.append(a)
        elif label == 0:
            bg.append(a)
    return fg, bg, n_sampled


def sample_loop(visible, x, y, gt, rect, max_pairs, seed):
    """-> dict: fg, bg (all members), n_sampled, ok, min_num, src, dst (sorted index lists; empty when not ok)."""
    fg, bg, n_sampled = classify_loop(visible, x, y, gt, rect)
    ok = len(fg) > 11 and len(bg) > 11
    min_num = min(len(fg), len(bg), max_pairs)
    pick = lambda members: sorted(sorted(members, key=lambda i: (key(seed, i), i))[:min_num]) if ok else []  # noqa: E731
    return {"fg": fg, "bg": bg, "n_sampled": n_sampled, "ok": ok, "min_num": min_num, "src": pick(fg), "dst": pick(bg)}


def info_list(ref):
    return [ref["n_sampled"], len(ref["fg"]), len(ref["bg"]), ref["min_num"], int(ref["ok"]), 0, 0, 0]


def random_scene(N, h, w, seed, rect=None, frac_visible=0.9, mask_values=(0.0, 1.0)):
    """Random anchors around an h x w image (some outside, some invisible) and a mask of the given values."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.1 * w, 1.1 * w, N).astype(np.float32)
    y = rng.uniform(-0.1 * h, 1.1 * h, N).astype(np.float32)
    visible = rng.random(N) < frac_visible
    gt = rng.choice(np.asarray(mask_values, dtype=np.float32), size=(h, w))
    if rect is None:
        rect = (h // 4, h // 4 + h // 2, w // 4, w // 4 + w // 2)
    return visible, x, y, gt, rect


def counted_scene(N, n_fg, n_bg, seed, h=37, w=53):
    """Exactly n_fg foreground and n_bg background anchors scattered among N (N >= n_fg + n_bg); every other anchor is invisible,
    outside the image, outside the rectangle or on a negative label.  The left half of the mask is 1, the right half 0, the
    bottom row -1; the rectangle leaves out a one-pixel border."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((h, w), dtype=np.float32)
    gt[:, : w // 2] = 1.0
    gt[h - 2, :] = -1.0
    rect = (1, h - 1, 1, w - 1)
    x = np.empty(N, dtype=np.float32)
    y = np.empty(N, dtype=np.float32)
    visible = np.ones(N, dtype=bool)
    kind = np.full(N, 2)
    order = rng.permutation(N)
    kind[order[:n_fg]] = 0
    kind[order[n_fg:n_fg + n_bg]] = 1
    rest = order[n_fg + n_bg:]
    for a in range(N):
        yy = rng.uniform(1.0, h - 2.0)            # rows 1 .. h - 3: inside the rectangle, above the -1 row
        if kind[a] == 0:
            x[a], y[a] = rng.uniform(1.0, w // 2), yy
        elif kind[a] == 1:
            x[a], y[a] = rng.uniform(w // 2, w - 1.0), yy
    for n, a in enumerate(rest):
        how = n % 4
        x[a], y[a] = rng.uniform(1.0, w - 1.0), rng.uniform(1.0, h - 2.0)
        if how == 0:
            visible[a] = False
        elif how == 1:
            x[a] = -x[a]
        elif how == 2:
            y[a] = 0.5                              # row 0: valid, outside the rectangle
        else:
            y[a] = h - 1.5                          # row h - 2: sampled, label -1
    x = np.minimum(x, np.nextafter(np.float32(w - 1), np.float32(0)))  # float32 rounding must not push an anchor over a boundary
    return visible, x, y, gt, rect


def to_torch(visible, x, y, gt, device="cpu"):
    return (torch.from_numpy(np.ascontiguousarray(visible)).to(device), torch.from_numpy(x).to(device), torch.from_numpy(y).to(device),
            torch.from_numpy(gt).to(device))
