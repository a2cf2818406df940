"""The rasterizer's workspace layout as the built library reports it (debugging / tests only): decodes the opaque geom / image /
binning byte tensors the forward returns.  Where a piece lies, how many elements of what size it holds, the constants and the
position formulas are the library's answers (gsr_workspace_layout, gsr_layout_*: the walk that carves the caller's pointer);
written here is only the presentation: the dtype and shape under which each piece is seen."""
import ctypes

import torch

from . import _native

def __getattr__(name):  # the constants, asked of the library when first wanted: the module imports without it
    if name in ("SEG1", "SEG2", "SEG_MAX", "XCD_CHUNK"):
        return _native.load().gsr_layout_constant(_native._ABI.constants["GSR_CONSTANT_" + name])
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _ask(symbol):
    return lambda *args: getattr(_native.load(), symbol)(*args)


ckpt_pos = _ask("gsr_layout_ckpt_pos")      # (k, L): list position of checkpoint k = 0 .. SEG_MAX-2 at the launch's segment length L (64 up
                                            # to 4096 tiles, 128 beyond).  Fixed positions: they do not depend on the list
num_chunks = _ask("gsr_layout_num_chunks")  # (P): binning chunks = rows of `table`
xcd_tiles = _ask("gsr_layout_xcd_tiles")    # (T): tile slots per XCD
xcd_tile = _ask("gsr_layout_xcd_tile")      # (xcd, i, T): the i-th tile of XCD `xcd`, -1 = none


def _pieces(which, P=0, W=0, H=0, R=0):
    """{name: gsr_layout_piece} of workspace GSR_LAYOUT_<which>"""
    lib, which = _native.load(), _native._ABI.constants["GSR_LAYOUT_" + which]
    n = lib.gsr_workspace_layout(which, P, W, H, R, None, 0)
    _native.check(min(n, 0), "gsr_workspace_layout")
    out = (_native.LayoutPiece * n)()
    lib.gsr_workspace_layout(which, P, W, H, R, out, n)
    return {ctypes.string_at(p.name).decode(): p for p in out}


def _i32(*names):
    return {k: (k, torch.int32, 1) for k in names}


# view -> (piece, dtype, `dtype`s per element)
_GEOM = {"rec_f32": ("rec", torch.float32, 16), "rec_i32": ("rec", torch.int32, 16), "rect": ("rect", torch.int32, 2),
         **_i32("depthkey", "tiles", "offsets"), "tmask": ("tmask", torch.int64, 1)}
_IMAGE = {"ranges": ("ranges", torch.int32, 2), "final_T": ("final_T", torch.float32, 1),
          **_i32("n_contrib", "table", "tile_count", "tile_work", "sorted_len", "need_full"), "ckpt": ("ckpt", torch.float32, 1),
          **_i32("occ_mass", "info", "qresume", "qorder", "occ_cut", "occ_drop", "tile_group")}
_BINNING = {"seg_keys": ("seg_keys", torch.int64, 1), "point_list_raw": ("point_list", torch.int32, 1),
            "slot_written": ("slot_written", torch.uint8, 1)}


def _views(buf, table, pieces):
    out = {}
    for key, (name, dtype, width) in table.items():
        p = pieces[name]
        if torch.empty((), dtype=dtype).element_size() * width != p.elem_size:
            raise TypeError(f"_layout: {key} is seen as {width} x {dtype}, but the library's {name} has elements of {p.elem_size} bytes")
        v = buf.narrow(0, p.offset, p.count * p.elem_size).view(dtype)
        out[key] = v.reshape(p.count, width) if width > 1 else v
    return out


def geom_views(buf, P):
    return {k: v[:P] for k, v in _views(buf, _GEOM, _pieces("GEOM", P=P)).items()}


def image_views(buf, P, W, H):
    out = _views(buf, _IMAGE, _pieces("IMAGE", P=P, W=W, H=H))
    for k in ("final_T", "n_contrib"):
        out[k] = out[k].reshape(H, W)
    out["table"] = out["table"].reshape(-1, out["ranges"].shape[0])   # a row of tile counts per binning chunk
    out["ckpt"] = out["ckpt"].reshape(__getattr__("SEG_MAX"), -1)
    out["qorder"] = out["qorder"].reshape(8, -1)   # dispatch order of the forward's quadrant tasks, per XCD (gsr_tuning.walk_depths)
    return out


def binning_views(buf, R, capacity=None):
    """`capacity` = what the workspace was sized for (>= R after a speculative forward)."""
    out = {k: v[:R] for k, v in _views(buf, _BINNING, _pieces("BINNING", R=R if capacity is None else capacity)).items()}
    raw = out["point_list_raw"]
    out["point_list"] = raw & 0x7fffffff   # Gaussian ids; bit 31 of an entry = the forward met it inside the alpha = 1/255 guard band
    out["band_flag"] = raw < 0
    return out
