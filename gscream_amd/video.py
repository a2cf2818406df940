"""The spiral video of render_set on the HIP path: Motion-JPEG in a plain AVI 1.0 (RIFF) file, made from the uint8 sheets of
gscream_amd.frames.rgbd_frame with gscream_amd.jpeg -- one encode and one read-back per batch of frames, no outside program.

    os.system("ffmpeg -y -i rgbd/%05d.png -q:v 0 ... .mp4")      ->  video.save_rgbd_video(sheets, path)      (train.py:844-846)

This is a DIFFERENT codec and container from the reference's .mp4 (MPEG-4 from ffmpeg): every frame is a baseline JPEG file, a key
frame of its own.  The container is pinned as written only: no player, ffmpeg or cv2 is on this stack; tests parse it by the statement
below and decode every frame with PIL (INTEGRATION Y).

    RIFF 'AVI ' { LIST 'hdrl' { 'avih' (56 bytes), LIST 'strl' { 'strh' (56: vids / MJPG, scale 1, rate fps), 'strf' (40: BITMAPINFOHEADER,
    24 bits, MJPG) } }, LIST 'movi' { '00dc' chunk per frame: one JPEG file, padded to even length with a zero }, 'idx1' { 16 bytes
    per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its size } }

All numbers little-endian.  A file stays below 2^31 - 1 bytes (no OpenDML): `add` refuses the frame that would pass it."""
import struct

import torch

from . import jpeg

__all__ = ["MjpegWriter", "save_rgbd_video"]

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
