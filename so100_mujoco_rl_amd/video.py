"""Streaming Motion-JPEG AVI writer: what `main.py record` writes its video with.

The reference records with SB3's VecVideoRecorder (moviepy / ffmpeg); neither is a dependency here.  This writer needs only
PIL's JPEG encoder: each frame is encoded and appended to the file at once (a RIFF 'AVI ' file: hdrl/avih/strl header,
a 'movi' list of '00dc' chunks, an 'idx1' index), and nothing but the 16-byte index entries is kept in memory, so a
3000-frame recording costs no more memory than one frame.  Every common player (VLC, mpv, ffplay, browsers via ffmpeg)
plays Motion-JPEG AVI.
"""
import io
import struct

import numpy as np

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


class MjpegAviWriter:
    def __init__(self, path, width, height, fps, quality=90):
        from PIL import Image  # noqa: F401  (fail at construction, not at the first frame, when PIL is missing)
        self.path, self.width, self.height, self.fps, self.quality = path, int(width), int(height), int(fps), int(quality)
        if self.width < 1 or self.height < 1 or self.fps < 1:
            raise ValueError(f"bad video geometry {width} x {height} @ {fps} fps")
        self._f = open(path, "wb")
        self._index = []                      # (offset from the 'movi' fourcc, size) of every frame
        self._max_chunk = 0
        self._write_headers()

    # ---- header layout: RIFF(AVI ) > LIST(hdrl) > avih, LIST(strl) > strh, strf ; LIST(movi) ; idx1
    def _avih(self, frames):
        return struct.pack("<4sI10I4I", b"avih", 56, round(1e6 / self.fps), 0, 0, AVIF_HASINDEX, frames, 0, 1,
                           self._max_chunk, self.width, self.height, 0, 0, 0, 0)

    def _strh(self, frames):
        return struct.pack("<4sI4s4sIHHIIIIIIIIhhhh", b"strh", 56, b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, frames,
                           self._max_chunk, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)

    def _strf(self):
        return struct.pack("<4sIIiiHH4sIiiII", b"strf", 40, 40, self.width, self.height, 1, 24, b"MJPG",
                           self.width * self.height * 3, 0, 0, 0, 0)

    def _write_headers(self):
        strl = b"strl" + self._strh(0) + self._strf()
        hdrl = b"hdrl" + self._avih(0) + struct.pack("<4sI", b"LIST", len(strl)) + strl
        f = self._f
        f.write(struct.pack("<4sI4s", b"RIFF", 0, b"AVI "))
        f.write(struct.pack("<4sI", b"LIST", len(hdrl)))
        self._hdrl_pos = f.tell()
        f.write(hdrl)
        f.write(struct.pack("<4sI", b"LIST", 0))
        self._movi_size_pos = f.tell() - 4
        self._movi_pos = f.tell()             # position of the 'movi' fourcc: idx1 offsets count from here
        f.write(b"movi")

    def write(self, frame):
        """frame: uint8 [height, width, 3] (RGB, row 0 at the top)."""
        from PIL import Image
        a = np.asarray(frame)
        if a.dtype != np.uint8 or a.shape != (self.height, self.width, 3):
            raise ValueError(f"frame must be uint8 [{self.height}, {self.width}, 3], got {a.dtype} {a.shape}")
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a), "RGB").save(buf, format="JPEG", quality=self.quality)
        data = buf.getvalue()
        f = self._f
        self._index.append((f.tell() - self._movi_pos, len(data)))
        f.write(struct.pack("<4sI", b"00dc", len(data)))
        f.write(data)
        if len(data) & 1:
            f.write(b"\0")
        self._max_chunk = max(self._max_chunk, len(data))

    @property
    def frames(self):
        return len(self._index)

    def close(self):
        f = self._f
        if f is None:
            return
        movi_end = f.tell()
        f.write(struct.pack("<4sI", b"idx1", 16 * len(self._index)))
        for off, size in self._index:
            f.write(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size))
        end = f.tell()
        n = len(self._index)
        f.seek(4); f.write(struct.pack("<I", end - 8))
        f.seek(self._movi_size_pos); f.write(struct.pack("<I", movi_end - self._movi_size_pos - 4))
        f.seek(self._hdrl_pos + 4); f.write(self._avih(n))
        f.seek(self._hdrl_pos + 4 + 64 + 8 + 4); f.write(self._strh(n))
        f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
