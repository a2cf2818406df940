"""The shared yardstick of test_normals.py / test_gpu_normals.py (and of tests/golden/make_reference_vectors7.py, which checks its inputs
with it): a per-pixel fp64 statement of the rules of gsr_depth_points / gsr_point_normals (include/gsraster.h), their tolerances, and
seeded synthetic frames.

Tolerances, with u32 = 2^-24 and u64 = 2^-53 the unit roundoffs.

Normals, per component: |got - oracle| <= 2 u32 + NORMAL_C(size) * cond * 2^-52.
  2 u32: the result is rounded to fp32 once (u32 for a component of magnitude <= 1), and the torch fallback, which normalises in
  fp64 and rounds, or a second rounding of the oracle's value when it is compared in fp32, may add another.
  The rest is the perturbation bound |dv| / |v| <= cond(A) (|dA| / |A| + |ds| / |s|) of the 3x3 system, counted in u64 = 2^-53:
  each of A's entries is a sum of size^2 exact products (fp32 x fp32 is exact in fp64) and carries at most size^2 roundings relative to
  sum |q_i q_j| <= |A|_F <= sqrt(3) |A|_2; s carries size^2 likewise (the camera's points lie on one side of the origin: no
  cancellation in s); the kernel's elimination with partial pivoting puts at most 14 roundings on the way to any one component
  (backward stable: they count against cond(A) once), the oracle's own LU solve about 3 n^2 = 27, norm and division 5.  (sqrt(3) size^2 + size^2 + 46) u64 < (1.4 size^2 + 23) 2^-52;
  NORMAL_C takes twice that for the second-order terms: 2.8 size^2 + 46, that is 273 at size 9.
  cond is that of the system solved: cond_2(A), or 1 where the identity replaces A (det < eps: v = s, no solve) and where a sum is
  not finite (IEEE semantics decide the result exactly).

Points, per component: |got - fp64| <= POINTS_K u32 (|c2w[r][0] xc| + |c2w[r][1] yc| + |c2w[r][2] zc| + |c2w[r][3]|).
  xn carries 2 roundings (subtraction, division), xc 3, the product c2w[r][0] xc 4, and it passes through 3 additions: 7 on the first
  term, fewer on the others.  POINTS_K = 8 covers the second-order terms.  Two fp32 evaluations in different orders (ours against
  the stored torch.matmul result, which may use FMAs) are each within that of fp64, so they differ by at most 2 POINTS_K u32 of that magnitude.
"""
import numpy as np

U32 = 2.0 ** -24
POINTS_K = 8


def NORMAL_C(size):
    return 2.8 * size * size + 46.0


def normal_tol(cond, size):
    """[h*w] cond -> [h*w, 1] bound per component."""
    return (2.0 * U32 + NORMAL_C(size) * np.asarray(cond, np.float64) * 2.0 ** -52)[:, None]


def points_oracle(depth, K, c2w):
    """depth [h,w], K [3,3], c2w [3,4] (fp32 values) -> (P [3,h,w] fp64, magnitude [3,h,w] fp64 of the bound above)."""
    d = np.asarray(depth, np.float64)
    K = np.asarray(K, np.float64)
    c = np.asarray(c2w, np.float64)
    h, w = d.shape
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xc = (j - K[0, 2]) / K[0, 0] * d
    yc = (i - K[1, 2]) / K[1, 1] * d
    P = np.stack([c[r, 0] * xc + c[r, 1] * yc + c[r, 2] * d + c[r, 3] for r in range(3)])
    mag = np.stack([np.abs(c[r, 0] * xc) + np.abs(c[r, 1] * yc) + np.abs(c[r, 2] * d) + np.abs(c[r, 3]) for r in range(3)])
    return P, mag


def _adjugate_rules(A, s, eps):
    """det and solve by cofactors in fp64, for sums that are not finite: only IEEE semantics matter there (inf - inf, 0 * inf and NaN
    operands give NaN under any evaluation order, and NaN ends as 0)."""
    a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    det = a00 * c00 + a01 * c01 + a02 * c02
    if det < eps:
        return s.copy(), det
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    adj = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
    return adj @ s / det, det


def normals_oracle(points, size=9, gamma=0.15, eps=1e-5):
    """points [3,h,w] fp32 -> dict: normals [h*w,3] fp64 (not rounded), cond [h*w] (of the system solved, see above), det [h*w],
    margin [h*w] (min over the window of ||dz/zc| - gamma|, in fp64), dropped [h*w] (window points the mask zeroed)."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    _, h, w = p.shape
    r = size // 2
    g32 = np.float32(gamma)
    off = np.arange(-r, r + 1)
    out = np.zeros((h * w, 3))
    cond, det_out, margin, dropped = np.ones(h * w), np.zeros(h * w), np.full(h * w, np.inf), np.zeros(h * w, np.int64)
    with np.errstate(all="ignore"):
        for i in range(h):
            iy = np.clip(i + off, 0, h - 1)
            for j in range(w):
                ix = np.clip(j + off, 0, w - 1)
                q = p[:, iy[:, None], ix[None, :]].reshape(3, -1)  # rows, then columns
                cz = p[2, i, j]
                t = np.abs((q[2] - cz) / cz)                        # fp32, one rounding per operation
                drop = t > g32                                       # False for NaN
                t64 = np.abs((q[2].astype(np.float64) - np.float64(cz)) / np.float64(cz))
                m = np.abs(t64 - float(g32))
                m = m[np.isfinite(m)]
                k = i * w + j
                margin[k] = m.min() if m.size else np.inf
                dropped[k] = int(drop.sum())
                ql = np.where(drop[None, :], np.float32(0), q).astype(np.longdouble)
                A = (ql[:, None, :] * ql[None, :, :]).sum(-1)
                s = ql.sum(-1)
                if np.isfinite(A).all() and np.isfinite(s).all():
                    det = (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[1, 2]) + A[0, 1] * (A[0, 2] * A[1, 2] - A[0, 1] * A[2, 2])
                           + A[0, 2] * (A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]))
                    A, s, det = A.astype(np.float64), s.astype(np.float64), float(det)
                    if det < eps:
                        v = s
                    else:
                        v = np.linalg.solve(A, s)
                        cond[k] = np.linalg.cond(A)
                else:
                    v, det = _adjugate_rules(A.astype(np.float64), s.astype(np.float64), eps)
                det_out[k] = det
                length = np.sqrt(v @ v)
                v = v / (1e-12 if length < 1e-12 else length)        # max(length, 1e-12) that keeps a NaN length
                v[np.isnan(v)] = 0.0
                out[k] = -v
    return dict(normals=out, cond=cond, det=det_out, margin=margin, dropped=dropped)


def reference_layout(n, h, w):
    """[h*w, 3] by pixel -> what the reference returns: [1, 3, w, h] with r[0, c, a, b] = n[a*h + b, c]."""
    return np.asarray(n).reshape(1, w, h, 3).transpose(0, 3, 1, 2)


def from_reference_layout(r):
    """The inverse: [1, 3, w, h] -> [h*w, 3] by pixel."""
    r = np.asarray(r)
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)).reshape(-1, 3)


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def synthetic_frame(h, w, seed):
    """A seeded frame for the shapes that have no stored case: depth [h,w] around 2 (smooth, slanted, with a x1.4 step along a
    diagonal so that the mask fires), focal 0.8 max(h, w), a camera turned by a few tenths of a radian -> (depth, K, c2w) fp32."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    f = 0.8 * max(h, w, 8)
    a, b, c = rng.uniform(0.5, 1.5, 3)
    depth = 2.0 + 0.15 * np.sin(a * 6.0 * i / max(h, 8) + 1.0) + 0.1 * np.cos(b * 5.0 * j / max(w, 8)) + 0.002 * c * (i + j) * 16.0 / max(h, w, 16)
    depth = np.where(i * w + 0.7 * j * h > 1.1 * h * w, depth * 1.4, depth)
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float32)
    c2w = np.concatenate([rotation(0.15, -0.2, 0.1), np.array([[0.3], [-0.2], [0.25]])], 1).astype(np.float32)
    return depth.astype(np.float32), K, c2w
