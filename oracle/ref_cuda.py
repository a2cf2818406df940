"""ctypes front-end of oracle/_ref/libgsref.so: the reference's own rasterizer kernels, compiled for gfx950 by
`make -C oracle ref` (recipe: oracle/Makefile, oracle/ref_cuda/) and run on the GPU.

TEST INFRASTRUCTURE ONLY, like oracle.py.  It loads the built library and nothing else: no file of the reference is read
here, so it works wherever the library travelled.  tests/test_gpu_reference_kernels.py holds the CPU oracle
(gs_oracle.c) and the HIP library against what these kernels compute.

forward() / backward() take the scene dictionaries of gscream_amd.synthetic / tests/golden and return the keys of
tests/helpers.oracle_forward / oracle.backward, so either side can stand in for the other in tests/helpers.py.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libgsref.so")
_LIB = None

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_int, _flt, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def available():
    """True when `make -C oracle ref` has produced the library (it needs the reference checkout at build time)."""
    return os.path.exists(LIB_PATH)


def lib():
    global _LIB
    if _LIB is None:
        L = ctypes.CDLL(LIB_PATH)
        L.gsref_last_error.restype = ctypes.c_char_p
        L.gsref_release.argtypes = [_vp]
        L.gsref_release.restype = None
        L.gsref_forward.restype = _int
        L.gsref_forward.argtypes = ([_int] * 3 + [_f32p, _int, _int] + [_f32p] * 6 + [_flt] + [_f32p] * 5 + [_flt, _flt]
                                    + [_f32p] * 3 + [_i32p, ctypes.POINTER(_vp)])
        L.gsref_state.restype = _int
        L.gsref_state.argtypes = [_vp, _u32p, _u8p] + [_f32p] * 6 + [_u32p] * 3 + [_u64p, _u32p, _f32p]
        L.gsref_backward.restype = _int
        L.gsref_backward.argtypes = ([_vp, _int, _int] + [_f32p] * 5 + [_flt] + [_f32p] * 5 + [_flt, _flt, _i32p]
                                     + [_f32p] * 3 + [_f32p] * 11)
        L.gsref_mark_visible.restype = _int
        L.gsref_mark_visible.argtypes = [_int] + [_f32p] * 3 + [_u8p]
        L.gsref_filter.restype = _int
        L.gsref_filter.argtypes = [_int] * 4 + [_f32p] * 2 + [_flt] + [_f32p] * 4 + [_flt, _flt, _i32p, _f32p, _f32p]
        _LIB = L
    return _LIB


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a, t=_f32p):
    return None if a is None else a.ctypes.data_as(t)


def _ok(rc, what):
    if rc < 0:
        raise RuntimeError(f"{what}: {lib().gsref_last_error().decode()}")
    return rc


class _Frame:
    """The three opaque buffers one forward left on the device; released with the state dictionary that holds it."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        if self.handle and _LIB is not None:
            _LIB.gsref_release(self.handle)
            self.handle = None


def _inputs(s):
    """The optional inputs as the reference's Python wrapper passes them: SH or precomputed colours, scales + rotations or a
    precomputed covariance; the absent one of each pair is an empty tensor there, a null pointer here."""
    shs = _f(s["shs"]) if "shs" in s else None
    colors = None if shs is not None else _f(s["colors"])
    cov = _f(s["cov3D_precomp"]) if "cov3D_precomp" in s else None
    scales = None if cov is not None else _f(s["scales"])
    rots = None if cov is not None else _f(s["rotations"])
    D = int(s.get("sh_degree", 0)) if shs is not None else 0
    M = 0 if shs is None else int(shs.shape[1])
    return shs, colors, cov, scales, rots, D, M


def forward(s):
    """Rasterizer::forward on scene `s` -> the keys of tests/helpers.oracle_forward (plus `rgb`, `point_keys`, `point_offsets`)."""
    L = lib()
    means3D = _f(s["means3D"])
    P, W, H = int(means3D.shape[0]), int(s["W"]), int(s["H"])
    shs, colors, cov, scales, rots, D, M = _inputs(s)
    opac, unc_in = _f(s["opacities"]), _f(s["uncertainties"])
    view, proj, campos, bg = _f(s["viewmatrix"]), _f(s["projmatrix"]), _f(s["campos"]), _f(np.asarray(s["bg"], np.float32))
    st = dict(out_color=np.zeros((3, H, W), np.float32), out_depth=np.zeros((1, H, W), np.float32),
              out_unc=np.zeros((1, H, W), np.float32), radii=np.zeros(P, np.int32))
    handle = _vp()
    R = _ok(L.gsref_forward(P, D, M, _p(bg), W, H, _p(means3D), _p(shs), _p(colors), _p(opac), _p(unc_in), _p(scales),
                            float(s["scale_modifier"]), _p(rots), _p(cov), _p(view), _p(proj), _p(campos), float(s["tanfovx"]),
                            float(s["tanfovy"]), _p(st["out_color"]), _p(st["out_depth"]), _p(st["out_unc"]),
                            _p(st["radii"], _i32p), ctypes.byref(handle)), "gsref_forward")
    frame = _Frame(handle.value)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    st.update(tiles_touched=np.zeros(P, np.uint32), clamped=np.zeros((P, 3), np.uint8), means2D=np.zeros((P, 2), np.float32),
              depths=np.zeros(P, np.float32), cov3D=np.zeros((P, 6), np.float32), conic_opacity=np.zeros((P, 4), np.float32),
              rgb=np.zeros((P, 3), np.float32), unc=np.zeros(P, np.float32), point_offsets=np.zeros(P, np.uint32),
              ranges=np.zeros((tiles, 2), np.uint32), point_list=np.zeros(R, np.uint32), point_keys=np.zeros(R, np.uint64),
              n_contrib=np.zeros((H, W), np.uint32), final_T=np.zeros((H, W), np.float32))
    _ok(L.gsref_state(frame.handle, _p(st["tiles_touched"], _u32p), _p(st["clamped"], _u8p), _p(st["means2D"]), _p(st["depths"]),
                      _p(st["cov3D"]), _p(st["conic_opacity"]), _p(st["rgb"]), _p(st["unc"]), _p(st["point_offsets"], _u32p),
                      _p(st["ranges"], _u32p), _p(st["point_list"], _u32p), _p(st["point_keys"], _u64p),
                      _p(st["n_contrib"], _u32p), _p(st["final_T"])), "gsref_state")
    if cov is not None:
        st["cov3D"] = cov  # (as oracle.forward: the covariance the backward reads)
    st.update(num_rendered=R, colors=colors if colors is not None else st["rgb"], bg=bg, W=W, H=H, _frame=frame)
    return st


def backward(s, state, grads):
    """Rasterizer::backward on the buffers `state` (a forward() result) holds -> the keys of oracle.backward."""
    L = lib()
    means3D = _f(s["means3D"])
    P, W, H = int(means3D.shape[0]), state["W"], state["H"]
    shs, colors, cov, scales, rots, D, M = _inputs(s)
    gc, gd, gu = (_f(g) for g in grads)
    assert gc.size == 3 * H * W and gd.size == H * W and gu.size == H * W
    o = dict(mean2D=np.zeros((P, 3), np.float32), conic=np.zeros((P, 4), np.float32), opacity=np.zeros((P, 1), np.float32),
             color=np.zeros((P, 3), np.float32), depth=np.zeros(P, np.float32), unc=np.zeros((P, 1), np.float32),
             mean3D=np.zeros((P, 3), np.float32), cov3D=np.zeros((P, 6), np.float32), sh=np.zeros((P, M, 3), np.float32),
             scale=np.zeros((P, 3), np.float32), rot=np.zeros((P, 4), np.float32))
    _ok(L.gsref_backward(state["_frame"].handle, D, M, _p(state["bg"]), _p(means3D), _p(shs), _p(colors), _p(scales),
                         float(s["scale_modifier"]), _p(rots), _p(cov), _p(_f(s["viewmatrix"])), _p(_f(s["projmatrix"])),
                         _p(_f(s["campos"])), float(s["tanfovx"]), float(s["tanfovy"]), _p(state["radii"], _i32p), _p(gc), _p(gd),
                         _p(gu), *[_p(o[k]) for k in ("mean2D", "conic", "opacity", "color", "depth", "unc", "mean3D", "cov3D", "sh",
                                                      "scale", "rot")]), "gsref_backward")
    return dict(dL_dmeans3D=o["mean3D"], dL_dcov3D=o["cov3D"], dL_dsh=o["sh"], dL_dscales=o["scale"], dL_drotations=o["rot"],
                dL_dmeans2D=o["mean2D"], dL_dcolors=o["color"], dL_dopacity=o["opacity"], dL_duncertainty=o["unc"],
                dL_ddepths=o["depth"], dL_dconic=np.ascontiguousarray(o["conic"][:, [0, 1, 3]]))  # (float4 {x, y, -, w}: backward.cu:596-598)


def mark_visible(means3D, viewmatrix, projmatrix):
    """Rasterizer::markVisible -> bool[P]."""
    means3D = _f(means3D)
    P = int(means3D.shape[0])
    out = np.zeros(P, np.uint8)
    _ok(lib().gsref_mark_visible(P, _p(means3D), _p(_f(viewmatrix)), _p(_f(projmatrix)), _p(out, _u8p)), "gsref_mark_visible")
    return out.astype(bool)


def _filter(positions, means3D, scales, rotations, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, scale_modifier, cov3D_precomp):
    means3D = _f(means3D)
    P = int(means3D.shape[0])
    radii = np.zeros(P, np.int32)
    x, y = (np.zeros(P, np.float32), np.zeros(P, np.float32)) if positions else (None, None)
    cov = _f(cov3D_precomp)
    _ok(lib().gsref_filter(P, 0, int(W), int(H), _p(means3D), _p(None if cov is not None else _f(scales)), float(scale_modifier),
                           _p(None if cov is not None else _f(rotations)), _p(cov), _p(_f(viewmatrix)), _p(_f(projmatrix)),
                           float(tanfovx), float(tanfovy), _p(radii, _i32p), _p(x), _p(y)), "gsref_filter")
    return radii, x, y


def visible_filter(means3D, scales, rotations, *, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, scale_modifier=1.0,
                   cov3D_precomp=None):
    """Rasterizer::visible_filter -> radii."""
    return _filter(False, means3D, scales, rotations, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, scale_modifier, cov3D_precomp)[0]


def position2D_filter(means3D, scales, rotations, *, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, scale_modifier=1.0,
                      cov3D_precomp=None):
    """Rasterizer::position2D_filter -> (radii, x, y)."""
    return _filter(True, means3D, scales, rotations, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, scale_modifier, cov3D_precomp)
