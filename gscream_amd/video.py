"""The spiral video of render_set on the HIP path: Motion-JPEG in a plain AVI 1.0 (RIFF) file, made from the uint8 sheets of
gscream_amd.frames.rgbd_frame with gscream_amd.jpeg -- one encode and one read-back per batch of frames, no outside program.

    os.system("ffmpeg -y -i rgbd/%05d.png -q:v 0 ... .mp4")      ->  video.save_rgbd_video(sheets, path)      (train.py:844-846)

This is a DIFFERENT codec and container from the reference's .mp4 (MPEG-4 from ffmpeg): every frame is a baseline JPEG file, a key
frame of its own.  The container is pinned as written only: no player, ffmpeg or cv2 is on this stack; tests parse it by the statement
below and decode every frame with PIL (INTEGRATION Y).

    RIFF 'AVI ' { LIST 'hdrl' { 'avih' (56 bytes), LIST 'strl' { 'strh' (56: vids / MJPG, scale 1, rate fps), 'strf' (40: BITMAPINFOHEADER,
    24 bits, MJPG) } }, LIST 'movi' { '00dc' chunk per frame: one JPEG file, padded to even length with a zero }, 'idx1' { 16 bytes
    per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its size } }

All numbers little-endian.  A file stays below 2^31 - 1 bytes (no OpenDML): `add` refuses the frame that would pass it.

Reading it back: MjpegReader walks the 'movi' list of such a file chunk by chunk (the index is not needed) and decodes the frames with
gscream_amd.jpeg_decode, a batch per call, on the device; read_rgbd_video returns all of them (INTEGRATION Z)."""
import struct

import torch

from . import jpeg

__all__ = ["MjpegReader", "MjpegWriter", "read_rgbd_video", "save_rgbd_video"]

AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
MAX_BYTES = (1 << 31) - 1
_HEAD = 12 + 12 + (8 + 56) + 12 + (8 + 56) + (8 + 40) + 12  # everything in front of the first chunk


class MjpegWriter:
    """MjpegWriter(path, W, H).add(frames) ... .close(); also a context manager.  frames: uint8 [H, W, 3] or [B, H, W, 3], on the
    device (encoded there, one read-back per call) or on the host (jpeg's host path, the same bytes)."""

    def __init__(self, path, W, H, fps=25, quality=95, subsampling="4:2:0"):
        if not (isinstance(W, int) and isinstance(H, int) and 0 < W <= 65535 and 0 < H <= 65535):
            raise ValueError(f"MjpegWriter: W={W!r} H={H!r} (need integers 1 .. 65535)")
        if not isinstance(fps, int) or fps < 1:
            raise ValueError(f"MjpegWriter: fps={fps!r} (need an integer >= 1: the stream's rate over a scale of 1)")
        if not isinstance(quality, int) or not 1 <= quality <= 100:
            raise ValueError(f"MjpegWriter: quality={quality!r} (need an integer 1 .. 100)")
        sub = jpeg._check_subsampling(subsampling, 3)
        if sub == 420 and (W % 2 or H % 2):
            raise ValueError(f"MjpegWriter: {W}x{H} is odd and the frames are 4:2:0 (players expect whole chroma samples; pass '4:4:4')")
        self.W, self.H, self.fps, self.quality, self.subsampling = W, H, fps, quality, subsampling
        self.index = []   # (offset from the 'movi' fourcc, size) per frame
        self.largest = 0
        self.f = open(path, "wb")
        self.f.write(b"\0" * _HEAD)
        self.at = _HEAD

    def __enter__(self):
        return self

    def __exit__(self, kind, *rest):
        self.close()
        return False

    def add(self, frames):
        if self.f is None:
            raise RuntimeError("MjpegWriter: the file is closed")
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or tuple(frames.shape[-3:]) != (self.H, self.W, 3):
            raise ValueError(f"MjpegWriter: frames are uint8 [{self.H}, {self.W}, 3] or [B, {self.H}, {self.W}, 3]")
        for data in jpeg.to_bytes(jpeg.encode(frames, self.quality, self.subsampling)):
            n = len(data)
            if self.at + 8 + n + (n & 1) + 8 + 16 * (len(self.index) + 1) > MAX_BYTES:
                raise RuntimeError(f"MjpegWriter: frame {len(self.index)} would take the file past 2^31 - 1 bytes (AVI 1.0 has no larger files)")
            self.f.write(b"00dc" + struct.pack("<I", n) + data + (b"\0" if n & 1 else b""))
            self.index.append((self.at - (_HEAD - 4), n))
            self.largest = max(self.largest, n)
            self.at += 8 + n + (n & 1)

    def close(self):
        if self.f is None:
            return
        f, n = self.f, len(self.index)
        f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size) for off, size in self.index))
        total = self.at + 8 + 16 * n
        avih = struct.pack("<14I", 1000000 // self.fps, min(self.largest * self.fps, 0xFFFFFFFF), 0, AVIF_HASINDEX, n, 0, 1, self.largest, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, n, self.largest, 0xFFFFFFFF, 0, 0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = (b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", self.at - _HEAD + 4) + b"movi")
        assert len(head) == _HEAD and len(avih) == 56 and len(strh) == 56 and len(strf) == 40
        f.seek(0)
        f.write(head)
        f.close()
        self.f = None


def save_rgbd_video(sheets, path, fps=25, quality=95, batch=8):
    """The line behind render_set's spiral loop: `sheets` yields the uint8 [H, 4W, 3] pictures of frames.rgbd_frame (or its RgbdFrame
    tuples), in order; they are encoded `batch` at a time.  25 frames a second is ffmpeg's default for an image sequence.  4:2:0 where
    the sheet's sizes are even, else 4:4:4 (the 567-row sheet of the reference's renders).  Returns the number of frames."""
    writer, held = None, []

    def flush():
        if held:
            writer.add(torch.stack(held) if len(held) > 1 else held[0])
            held.clear()

    try:
        for sheet in sheets:
            sheet = getattr(sheet, "rgbd", sheet)
            if writer is None:
                H, W = int(sheet.shape[0]), int(sheet.shape[1])
                writer = MjpegWriter(path, W, H, fps, quality, "4:2:0" if (W % 2 == 0 and H % 2 == 0) else "4:4:4")
            held.append(sheet)
            if len(held) >= batch:
                flush()
        if writer is None:
            raise ValueError("save_rgbd_video: no frames")
        flush()
        return len(writer.index)
    finally:
        if writer is not None:
            writer.close()


class MjpegReader:
    """MjpegReader(path): the frames of a file MjpegWriter wrote.  W, H, fps from the headers; len() frames; frames(device, batch)
    yields uint8 [H, W, 3] pictures in order, `batch` files per jpeg_decode.decode + check, the pictures staying on `device`.  The
    'movi' list is walked by its chunk sizes; 'idx1' is not read.  ValueError for a file that is not RIFF 'AVI ' with an MJPG stream
    first, or whose chunks run past the list."""

    def __init__(self, path):
        with open(path, "rb") as f:
            data = f.read()
        self.path = path

        def bad(reason):
            return ValueError(f"MjpegReader: {path}: {reason}")
        if len(data) < _HEAD or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise bad("not a RIFF 'AVI ' file")
        at, end = 12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0])
        self.W = self.H = self.fps = None
        self.chunks = []  # (offset of the JPEG file, size)
        movi = False
        while at + 8 <= end and not movi:
            kind, size = struct.unpack_from("<4sI", data, at)
            if kind == b"LIST" and data[at + 8:at + 12] == b"hdrl":
                avih = at + 12
                if data[avih:avih + 4] != b"avih" or struct.unpack_from("<I", data, avih + 4)[0] < 40:
                    raise bad("'hdrl' does not start with an 'avih' chunk")
                self.W, self.H = struct.unpack_from("<II", data, avih + 8 + 32)
                strl = avih + 8 + struct.unpack_from("<I", data, avih + 4)[0]
                if data[strl:strl + 4] != b"LIST" or data[strl + 8:strl + 16] != b"strlstrh" or data[strl + 20:strl + 28] != b"vidsMJPG":
                    raise bad("the first stream is not Motion-JPEG video")
                scale, rate = struct.unpack_from("<II", data, strl + 20 + 20)
                self.fps = rate / scale if scale else float(rate)
            elif kind == b"LIST" and data[at + 8:at + 12] == b"movi":
                movi = True
                stop, q = min(end, at + 8 + size), at + 12
                while q + 8 <= stop:
                    tag, n = struct.unpack_from("<4sI", data, q)
                    if q + 8 + n > stop:
                        raise bad("a chunk runs past the 'movi' list")
                    if tag == b"00dc" and n:
                        self.chunks.append((q + 8, n))
                    q += 8 + n + (n & 1)
            at += 8 + size + (size & 1)
        if not movi or self.W is None:
            raise bad("no 'hdrl' or no 'movi' list")
        self.data = data

    def __len__(self):
        return len(self.chunks)

    def frame_bytes(self, i):
        off, n = self.chunks[i]
        return self.data[off:off + n]

    def frames(self, device, batch=8, split=None):
        from . import jpeg_decode
        split = jpeg_decode.DEFAULT_SPLIT if split is None else split  # (jpeg_decode.decode's `split`, passed through)
        if batch < 1:
            raise ValueError(f"MjpegReader: batch={batch!r} (need >= 1)")
        for at in range(0, len(self.chunks), batch):
            ids = range(at, min(at + batch, len(self.chunks)))
            pictures = jpeg_decode.check(jpeg_decode.decode([self.frame_bytes(i) for i in ids], device, [f"{self.path} frame {i}" for i in ids], split=split))
            for image in pictures.images:
                if tuple(image.shape) != (self.H, self.W, 3):
                    raise ValueError(f"MjpegReader: {self.path}: a frame of {tuple(image.shape)} in a {self.H} x {self.W} stream")
                yield image


def read_rgbd_video(path, device, batch=8):
    """All frames of a save_rgbd_video / MjpegWriter file -> the list of uint8 [H, W, 3] pictures on `device`."""
    return list(MjpegReader(path).frames(device, batch))
