"""Baseline JPEG files encoded on the device (include/gp_jpeg.h, csrc/jpeg_kernels.hip) -- colour transform, chroma subsampling, the
8 x 8 DCT, quantisation, Huffman coding with a restart interval per workgroup, byte stuffing and every marker: the bytes that come
back are the file -- and Motion-JPEG video in an AVI container, whose frames are those files and whose bookkeeping is the host's.

  [REF eval.py:113-115]             the interpolated-pose frames muxed into <scene>.mp4
  [REF train_GCN.py:45-53,147]      renders/video.mp4 of the predicted keypoint motion
  [REF metrics.py:148]              deltas/%05d.jpg

The reference's videos are mp4 through cv2 / imageio; neither exists where this runs, and Motion-JPEG needs nothing but the encoder
here.  Quality 90 for video is this project's choice (the reference's mp4 encoders expose no setting to be at parity with).

`encode` reads nothing from the device; `encode_to_bytes` reads once; `JpegWriter` and `VideoWriter` copy the files into pinned
buffers behind the encode and leave the waiting and the disk to a worker thread (png_ops.PngWriter's ring).  HIP only: CPU tensors
raise."""
from __future__ import annotations

import ctypes as C
import os
import struct
from fractions import Fraction

import torch

from . import _lib
from . import png_ops
from .png_ops import SRC_F32, SRC_U8

GP_JPEG_ABI_VERSION = 1             # include/gp_jpeg.h
RESTART_MCUS = 8
BLOCK_BITS = 1660
HEAD_BYTES = 629
MAX_BATCH = 65535
MAX_SIDE = 65535
SUB_420, SUB_444 = 0, 1
SUBSAMPLING = {"420": SUB_420, "444": SUB_444, "4:2:0": SUB_420, "4:4:4": SUB_444}
VIDEO_QUALITY = 90                  # this project's choice
AVI_MAX_BYTES = 2 ** 31 - 1         # (no OpenDML: one RIFF chunk, 32-bit offsets that players read as signed)


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_jpeg.h declares them (tests/test_jpeg_host.py compares the two)
        "gp_jpeg_abi_version": (i32, []),
        "gp_jpeg_quant_tables": (i32, [i32, P, P]),
        "gp_jpeg_bound": (i64, [i32, i32, i32]),
        "gp_jpeg_scratch_bytes": (i64, [i32, i32, i32, i32]),
        "gp_jpeg_encode": (i32, [i32, i32, i32, P, i32, P, P, i32, P, i64, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_jpeg.h", "gp_jpeg_abi_version", GP_JPEG_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _sub(subsampling) -> int:
    try:
        return SUBSAMPLING[str(subsampling)]
    except KeyError:
        raise ValueError(f"jpeg_ops: subsampling must be '420' or '444' (got {subsampling!r})") from None


def quant_tables(quality):
    """(luminance, chrominance): two lists of 64 entries in natural (row-major) order, the Annex K tables scaled by the IJG rule."""
    lum, chr_ = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    if lib().gp_jpeg_quant_tables(int(quality), lum, chr_):
        raise ValueError(f"jpeg_ops.quant_tables: {_lib.last_error()}")
    return list(lum), list(chr_)


def bound(H, W, subsampling="420") -> int:
    """The largest file an H x W image can become, in bytes (a multiple of 8); ValueError outside the limits of gp_jpeg.h."""
    n = int(lib().gp_jpeg_bound(int(H), int(W), _sub(subsampling)))
    if n < 0:
        raise ValueError(f"jpeg_ops.bound: {_lib.last_error()}")
    return n


def _tables(quality, qtables):
    """Two ctypes arrays of 64 bytes from `qtables` (two sequences of 64 integers in 1 .. 255, natural order) or from `quality`."""
    if qtables is None:
        qtables = quant_tables(quality)
    if len(qtables) != 2 or any(len(t) != 64 for t in qtables) or any(not 1 <= int(v) <= 255 for t in qtables for v in t):
        raise ValueError("jpeg_ops: qtables must be two tables of 64 entries in 1 .. 255 (natural order)")
    return tuple((C.c_uint8 * 64)(*[int(v) for v in t]) for t in qtables)


def encode(images, *, quality=90, subsampling="420", qtables=None, out=None):
    """(buffer [B, stride] uint8, sizes [B] int32), both on the device: buffer[b, :sizes[b]] is the complete JPEG file of image b
    (baseline, Y Cb Cr, JFIF; float input quantised as floor(x * 255 + 0.5) clamped, NaN -> 0), stride = bound(H, W, subsampling).
    The rest of a row is not written.  images: as png_ops.encode takes them, with the same refusals.  qtables: (luminance,
    chrominance) in natural order instead of `quality`.  out: a contiguous [B, stride >= bound] uint8 device tensor to receive the
    files.  Nothing is read from the device."""
    sub = _sub(subsampling)
    lum, chr_ = _tables(quality, qtables)
    x = png_ops._batch(images)
    B, _, H, W = x.shape
    dev = x.device
    stride = bound(H, W, subsampling)
    scratch = _lib.scratch(lib().gp_jpeg_scratch_bytes, B, H, W, sub, device=dev)
    if out is None:
        out = torch.empty(B, stride, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != dev or out.dim() != 2 or out.shape[0] != B
          or out.shape[1] < stride or not out.is_contiguous()):
        raise RuntimeError(f"jpeg_ops.encode: out must be a contiguous [{B}, >= {stride}] uint8 tensor on {dev}")
    sizes = torch.empty(B, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_jpeg_encode(B, H, W, x, SRC_U8 if x.dtype == torch.uint8 else SRC_F32, lum, chr_, sub,
                                        out, out.shape[1], sizes, scratch, _lib.stream_ptr(dev)), "gp_jpeg_encode")
    return out, sizes


def encode_to_bytes(images, *, quality=90, subsampling="420", qtables=None):
    """The files as a list of bytes: one read of the device (the sizes ride behind the buffer in one tensor)."""
    return png_ops.files_to_bytes(*encode(images, quality=quality, subsampling=subsampling, qtables=qtables))


class JpegWriter(png_ops.PngWriter):
    """png_ops.PngWriter with the JPEG encoder behind the same ring: `submit(images, paths)` enqueues the encode and the copies into
    pinned buffers and returns; worker threads wait for the event and write the files; `close()` re-raises the first worker error."""

    def __init__(self, slots=32, threads=2, quality=90, subsampling="420", qtables=None):
        super().__init__(slots=slots, threads=threads)
        self.subsampling = subsampling
        _sub(subsampling)
        self.qtables = tuple(list(t) for t in _tables(quality, qtables))       # (also the refusal of a bad quality, at construction)

    def _encode(self, x):
        return encode(x, subsampling=self.subsampling, qtables=self.qtables)


# ---- Motion-JPEG in AVI: host bookkeeping ------------------------------------------------------------------------------------------
def _rate_scale(fps):
    f = Fraction(fps).limit_denominator(100000)
    if f <= 0:
        raise ValueError(f"fps must be positive (got {fps!r})")
    return f.numerator, f.denominator


class AviFile:
    """A RIFF 'AVI ' file of complete JPEG files: LIST hdrl (avih, LIST strl (strh vids/MJPG, strf BITMAPINFOHEADER 24 bit 'MJPG')),
    LIST movi (one '00dc' chunk per frame, padded to an even length), idx1 (one keyframe entry per frame, offsets from the 'movi'
    tag).  dwTotalFrames, dwLength, dwSuggestedBufferSize, dwMaxBytesPerSec and the RIFF / LIST sizes are patched by close().
    `add` refuses a frame after which the finished file would pass AVI_MAX_BYTES: there is no OpenDML index here."""
    HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))       # 'hdrl' avih LIST strl(strh strf)
    MOVI_AT = 12 + 8 + HDRL_BYTES                                    # the 'LIST' of movi

    def __init__(self, path, width, height, fps):
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width <= MAX_SIDE and 1 <= self.height <= MAX_SIDE):
            raise ValueError(f"AviFile: {self.width} x {self.height} outside [1, {MAX_SIDE}]")
        self.rate, self.scale = _rate_scale(fps)
        self.path = os.fspath(path)
        self.frames = 0
        self._index = []                 # (offset from the 'movi' tag, length)
        self._movi = 4                   # bytes of the movi list's data so far: its tag
        self._largest = 0
        self._fp = open(self.path, "wb")
        self._fp.write(self._headers())

    @staticmethod
    def final_bytes(movi_bytes, frames):
        """The finished file's length for a movi list of `movi_bytes` (tag and padded chunks) and `frames` index entries."""
        return AviFile.MOVI_AT + 8 + movi_bytes + 8 + 16 * frames

    def _headers(self):
        n, big = self.frames, self._largest
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        persec = min(0xffffffff, (self._movi * self.rate) // (self.scale * n)) if n else 0
        avih = struct.pack("<14I", usec, persec, 0, 0x10, n, 0, 1, big, self.width, self.height, 0, 0, 0, 0)       # AVIF_HASINDEX
        strh = struct.pack("<4s4sIHHIIIIIIIIHHHH", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, big, 0xffffffff, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        assert len(hdrl) == self.HDRL_BYTES
        total = self.final_bytes(self._movi, n)
        return (b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", self._movi) + b"movi")

    def add(self, data):
        """Append one frame: the bytes of a complete JPEG file."""
        if self._fp is None:
            raise RuntimeError("AviFile.add: the file is closed")
        n = len(data)
        padded = n + (n & 1)
        if self.final_bytes(self._movi + 8 + padded, self.frames + 1) > AVI_MAX_BYTES:
            raise RuntimeError(f"AviFile.add: frame {self.frames} would take {self.path} past {AVI_MAX_BYTES} bytes (AVI without OpenDML)")
        self._fp.write(b"00dc" + struct.pack("<I", n))
        self._fp.write(data)
        if n & 1:
            self._fp.write(b"\0")
        self._index.append((self._movi, n))
        self._movi += 8 + padded
        self._largest = max(self._largest, n)
        self.frames += 1

    def close(self):
        if self._fp is None:
            return
        fp, self._fp = self._fp, None
        try:
            fp.write(b"idx1" + struct.pack("<I", 16 * self.frames))
            fp.write(b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, n) for off, n in self._index))       # AVIIF_KEYFRAME
            fp.seek(0)
            fp.write(self._headers())
        finally:
            fp.close()


class VideoWriter(png_ops.PngWriter):
    """Motion-JPEG video written behind the render loop: `submit(images)` encodes on the device and appends the frames in submission
    order (one worker thread, a FIFO queue); `close()` drains, finalises the container and re-raises the first worker error.  The
    H x W of the first frame fixes the video: another size raises at submit.  `frames`: the frames submitted so far."""

    def __init__(self, path, fps, quality=VIDEO_QUALITY, subsampling="420", slots=32):
        super().__init__(slots=slots, threads=1)
        _rate_scale(fps)
        _sub(subsampling)
        self.path, self.fps, self.subsampling = os.fspath(path), fps, subsampling
        self.qtables = tuple(list(t) for t in _tables(quality, None))
        self.size = None
        self._avi = None

    @property
    def frames(self):
        return self.files

    def _encode(self, x):
        return encode(x, subsampling=self.subsampling, qtables=self.qtables)

    def _store(self, path, data):
        self._avi.add(data)

    def submit(self, images, paths=None):
        x = png_ops._batch(images)
        H, W = int(x.shape[2]), int(x.shape[3])
        if self.size is None:
            if self._closed:
                raise RuntimeError("VideoWriter.submit: the writer is closed")
            self._avi = AviFile(self.path, W, H, self.fps)
            self.size = (H, W)
        elif self.size != (H, W):
            raise RuntimeError(f"VideoWriter.submit: a frame of {H} x {W} in a video of {self.size[0]} x {self.size[1]}")
        super().submit(x, [None] * x.shape[0])

    def close(self):
        try:
            super().close()
        finally:
            if self._avi is not None:
                self._avi.close()
