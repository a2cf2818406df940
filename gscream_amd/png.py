"""render_set's PNG files on the HIP path: the finished uint8 pictures of gscream_amd.frames -> the bytes of their .png files, on the
device, ready for one D2H copy and a plain file write.  This is the stage behind torchvision.utils.save_image, cv2.imwrite and
plt.imsave in train.py:776-834, which on the host costs a hundred times the render it stores.

Integration is a handful of rebindings in render_set (INTEGRATION U):

    save_image(x, path) per file                      ->  png.save(frames.to_uint8(x), path)
    the five files of a train / test view             ->  png.save_view_frames(frames.view_frames(...), paths): two encodes, two copies
    the rgbd picture and its four panels              ->  png.save_rgbd_frame(frames.rgbd_frame(..., panels=True), paths)

The rules (include/gsraster.h has them in full): signature, IHDR, one IDAT per deflate chunk, IEND; zlib header 78 01 and the Adler-32
of the filtered stream; the stream is filtered per row (a fixed type 0 .. 4, or "adaptive": the type with the smallest sum of |signed
residual|, ties to the lowest) and cut every 32 KiB; each chunk is a deflate sequence of its own -- literals and distance-1 matches of
3 .. 258 by the greedy run rule, one dynamic-Huffman block or a stored block, whichever is shorter, an empty stored block behind every
chunk but the last.  No LZ77 matching beyond distance 1: rendered photographs gain nothing from it, flat pictures are runs, smooth
colour maps come out about 2.5 times the size of PIL's default (a stated loss).

The HIP path (gscream_amd/csrc/png.hip; `last_path = "hip"`) takes uint8 tensors on a HIP device, [H, W, C] or [B, H, W, C] with C = 1, 3
or 4, the inner two dimensions dense and the row stride free -- a panel of a wider sheet is read in place -- launches three kernels on
torch's current stream, allocates its output and a workspace, reads nothing back and never synchronises.  CPU tensors and
`force_torch = True` take a host statement of the same container, filter and cuts with zlib's Z_RLE strategy per chunk
(`last_path = "torch"`): a valid file with the same filter bytes, whose size may differ from the device's.  A missing library raises;
nothing falls back quietly."""
import struct
import zlib
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _native

__all__ = ["PngBatch", "capacity", "encode", "filter_stream", "save", "save_rgbd_frame", "save_view_frames", "to_bytes"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last encode took

CHUNK = _native.PNG_CHUNK           # GSR_PNG_CHUNK
HEADER = _native.PNG_HEADER_BYTES   # GSR_PNG_HEADER_BYTES: four uint32 words {file bytes, IDAT chunks, 0, 0} in front of every file
MAX_PICTURES = 65535
_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": _native.PNG_FILTER_ADAPTIVE}
_COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
_SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngBatch(NamedTuple):
    """data: uint8 [B, >= HEADER + capacity] on the pictures' device, row b = the header words, then picture b's file; shape = (H, W, C);
    batched: whether `encode` was given [B, H, W, C]."""
    data: torch.Tensor
    shape: Tuple[int, int, int]
    batched: bool


def capacity(H, W, C):
    """gsr_png_capacity: the most bytes a file of an [H, W, C] picture takes (every chunk stored)."""
    stream = H * (1 + W * C)
    return 8 + 25 + -(-stream // CHUNK) * (12 + 5 + 5) + stream + 2 + 4 + 12


def _filter_code(filter):
    if isinstance(filter, str):
        if filter not in _FILTERS:
            raise ValueError(f"png: filter {filter!r} (have {tuple(_FILTERS)} or 0 .. 4)")
        return _FILTERS[filter]
    if filter not in range(5):
        raise ValueError(f"png: filter {filter!r} (have {tuple(_FILTERS)} or 0 .. 4)")
    return int(filter)


# ---- the host statement ----
def filter_stream(image, filter="adaptive"):
    """uint8 numpy [H, W, C] -> the filtered stream, uint8 [H, 1 + W*C], by the filter rule."""
    code = filter if filter == _native.PNG_FILTER_ADAPTIVE else _filter_code(filter)
    H, W, C = image.shape
    cur = image.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, C:] = cur[:, :-C]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, C:] = cur[:-1, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([(cur - q) & 255 for q in (np.zeros_like(cur), a, b, (a + b) >> 1, paeth)])  # [5, H, W*C]
    if code == _native.PNG_FILTER_ADAPTIVE:
        types = np.where(res < 128, res, 256 - res).sum(2).argmin(0)  # (argmin: the first = the lowest type of a tie)
    else:
        types = np.full(H, code)
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = types
    out[:, 1:] = res[types, np.arange(H)]
    return out


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def _encode_host(image, filter):
    """uint8 numpy [H, W, C] -> the file's bytes: the same container, filter and cuts, zlib's Z_RLE per chunk."""
    H, W, C = image.shape
    stream = filter_stream(image, filter).tobytes()
    parts = [_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _COLOUR_TYPE[C], 0, 0, 0))]
    cuts = range(0, len(stream), CHUNK)
    for k, at in enumerate(cuts):
        last = k == len(cuts) - 1
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        piece = stream[at:at + CHUNK]
        data = co.compress(piece) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)
        stored = (bytes([1 if last else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece
                  + (b"" if last else b"\x00\x00\x00\xff\xff"))
        if len(stored) < len(data):  # (zlib may split a chunk into blocks and pass the stored form: the capacity is derived from it)
            data = stored
        if k == 0:
            data = b"\x78\x01" + data
        if last:
            data += struct.pack(">I", zlib.adler32(stream))
        parts.append(_chunk(b"IDAT", data))
    parts.append(_chunk(b"IEND", b""))
    return b"".join(parts), len(cuts)


# ---- the calls ----
def _check_images(images):
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise TypeError("png: a uint8 tensor")
    batched = images.dim() == 4
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or images.shape[3] not in _COLOUR_TYPE or 0 in images.shape:
        raise ValueError(f"png: images are {tuple(images.shape)} (need [H, W, C] or [B, H, W, C] with C = 1, 3 or 4, none empty)")
    B, H, W, C = images.shape
    if B > MAX_PICTURES or W * C >= 1 << 24 or H * (1 + W * C) >= 0x70000000:
        raise ValueError(f"png: images of {tuple(images.shape)} are beyond B <= {MAX_PICTURES}, W*C < 2^24, H*(1 + W*C) < 0x70000000")
    return images, batched


def encode(images, filter="adaptive", out=None):
    """uint8 [H, W, C] or [B, H, W, C] (C = 1, 3, 4: grey, RGB, RGBA) -> PngBatch.  The inner two dimensions are dense, the row stride and
    the picture stride are free (anything else is copied first).  out: a uint8 [B, >= HEADER + capacity(H, W, C)] buffer on the pictures'
    device with dense rows whose stride is a multiple of 4; only the header words and the files' own bytes are written.  No
    synchronisation on the HIP path."""
    global last_path
    images, batched = _check_images(images)
    code = _filter_code(filter)
    B, H, W, C = images.shape
    need = HEADER + capacity(H, W, C)
    if out is None:
        out = torch.empty((B, (need + 15) & ~15), dtype=torch.uint8, device=images.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < need
          or out.device != images.device or out.stride(1) != 1 or out.stride(0) % 4 or out.stride(0) < need or out.data_ptr() % 4):
        raise ValueError(f"png: out is a uint8 [{B}, >= {need}] buffer on {images.device}, dense rows, row stride and address multiples of 4")
    if force_torch or not images.is_cuda:
        last_path = "torch"
        host = images.cpu().numpy()
        for b in range(B):
            data, chunks = _encode_host(host[b], code)
            row = np.frombuffer(struct.pack("<IIII", len(data), chunks, 0, 0) + data, np.uint8)
            out[b, :row.size] = torch.from_numpy(row.copy()).to(out.device)
        return PngBatch(out, (H, W, C), batched)
    last_path = "hip"
    sb, sy, sx, sc = images.stride()
    if sc != 1 or sx != C or sy < W * C or (B > 1 and sb < 0):
        images = images.contiguous()
        sb, sy, sx, sc = images.stride()
    lib = _native.load()
    workspace = torch.empty(int(lib.gsr_png_workspace_bytes(B, H, W, C)), dtype=torch.uint8, device=images.device)
    _native.run("gsr_png_encode", images.device, _native.ptr(images), sy, sb, B, H, W, C, code, _native.ptr(out), out.stride(0), _native.ptr(workspace))
    return PngBatch(out, (H, W, C), batched)


def to_bytes(batch):
    """PngBatch -> the files as a list of bytes: ONE copy of the buffer to the host (which waits for the encode), then slices of it."""
    host = batch.data.cpu().numpy()
    files = []
    for row in host:
        n = int(row[:4].view("<u4")[0])
        if not 0 < n <= row.size - HEADER:
            raise RuntimeError(f"png: a header says {n} bytes in a buffer of {row.size - HEADER}")
        files.append(row[HEADER:HEADER + n].tobytes())
    return files


def _write(files, paths):
    if len(files) != len(paths):
        raise ValueError(f"png: {len(files)} pictures and {len(paths)} paths")
    for data, path in zip(files, paths):
        with open(path, "wb") as f:
            f.write(data)


def save(images, paths, filter="adaptive"):
    """encode, one copy, and the files: `paths` is one path for [H, W, C], a sequence of B paths for [B, H, W, C]."""
    batch = encode(images, filter)
    _write(to_bytes(batch), list(paths) if batch.batched else [paths])


def _panels(sheet, count):
    """[H, count*W, C] -> [count, H, W, C]: the panels as a batch, a view of the sheet (picture stride W*C, row stride count*W*C)."""
    H, WW, C = sheet.shape
    return sheet.view(H, count, WW // count, C).permute(1, 0, 2, 3)


def save_view_frames(vf, paths, filter="adaptive"):
    """frames.ViewFrames -> its five files; paths = (render, uncertainty, error, gt, depth).  The four RGB panels are encoded in one
    call as views of the sheet, the RGBA depth picture in a second: two encodes, two copies."""
    paths = list(paths)
    if len(paths) != 5:
        raise ValueError(f"save_view_frames: {len(paths)} paths (need render, uncertainty, error, gt, depth)")
    four, depth = encode(_panels(vf.sheet, 4), filter), encode(vf.depth, filter)
    _write(to_bytes(four) + to_bytes(depth), paths)


def save_rgbd_frame(fr, paths, filter="adaptive"):
    """frames.RgbdFrame (rgbd_frame(..., panels=True)) -> its five files; paths = (rgbd, render, depth, normal, uncertainty)."""
    paths = list(paths)
    if len(paths) != 5:
        raise ValueError(f"save_rgbd_frame: {len(paths)} paths (need rgbd, render, depth, normal, uncertainty)")
    whole, four = encode(fr.rgbd, filter), encode(_panels(fr.rgbd, 4), filter)
    _write(to_bytes(whole) + to_bytes(four), paths)
