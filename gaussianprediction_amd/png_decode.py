"""PNG files decoded on the device (include/gp_png_decode.h, csrc/png_decode_kernels.hip): inflate, the Adler-32, the five row filters,
the planar conversion with its division by 255 and, for RGBA ground truth, the composite over a background -- what the loaders did per
file with a host library.

  [REF scene/dataset_readers.py:210-218]   Image.open, convert("RGBA"), the composite in numpy
  [REF utils/general_utils.py:21-27]       PILtoTorch: resize, / 255.0, permute (the resize: `resize=`, through resize_ops)

The host walks the chunks (`parse`: signature, lengths, every CRC-32, IHDR) and copies the IDAT data of all files, with their segment
tables, into ONE pinned buffer that goes up in one copy.  A file with exactly ceil(S / 16384) IDAT chunks (S = H (1 + C W)) -- every
file png_ops writes -- is tried BANDED, one workgroup per chunk; the device proves or refutes that every chunk stands alone, and an
image that comes back NOT_BANDED is decoded again SERIALLY, as one stream.  `decode` reads the status and mode words once per pass.
16-bit, sub-byte, palette and interlaced files are refused on the host with a ValueError: the package has no other decoder to fall
back to.  HIP only: CPU devices raise."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from types import SimpleNamespace

import torch

from . import _lib, decode_stage
from .decode_stage import DST_F32, DST_U8, MAX_BATCH, READER_THREADS  # noqa: F401  (what include/gp_png_decode.h calls GP_PNG_DECODE_*)

GP_PNG_DECODE_ABI_VERSION = 1       # include/gp_png_decode.h
BAND_BYTES = 16384                  # GP_PNG_BAND_BYTES of include/gp_png.h: where png_ops cuts its IDAT chunks
MODE_SERIAL, MODE_BANDED = 1, 2
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}  # colour type -> C

STATUS = {0: "OK", 1: "TRUNCATED", 2: "BLOCK_TYPE", 3: "STORED_LEN", 4: "TOO_MANY_CODES", 5: "CLEN_CODE", 6: "REPEAT_FIRST",
          7: "REPEAT_OVERRUN", 8: "LIT_OVERSUBSCRIBED", 9: "LIT_INCOMPLETE", 10: "NO_END_OF_BLOCK", 11: "LIT_SYMBOL", 12: "DIST_SYMBOL",
          13: "DIST_TOO_FAR", 14: "OUTPUT_LONG", 15: "OUTPUT_SHORT", 16: "ADLER", 17: "FILTER", 18: "ZLIB_METHOD", 19: "ZLIB_FDICT",
          20: "ZLIB_FCHECK", 21: "ZLIB_WINDOW", 22: "DIST_CODE", 23: "NOT_BANDED", 24: "TRAILING", 25: "TABLE", 26: "BUDGET",
          27: "LIT_CODE", 28: "FINAL_INSIDE"}       # GP_PNG_DECODE_* (tests/test_png_decode_host.py compares the two)
NOT_BANDED = 23


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_png_decode.h declares them (tests/test_png_decode_host.py compares the two)
        "gp_png_decode_abi_version": (i32, []),
        "gp_png_decode_scratch_bytes": (i64, [i32, i32, i32, i32, i32]),
        "gp_png_decode": (i32, [i32, i32, i32, i32, i32, i32, P, i64, P, i32, P, P, P, i64, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_png_decode.h", "gp_png_decode_abi_version", GP_PNG_DECODE_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def parse(data, name="<bytes>"):
    """Walk the chunks of a PNG file held in `data` (bytes): the signature, every chunk's length and CRC-32, the IHDR, the IDAT chunks
    in one run.  Returns a namespace: name, H, W, C, S = H (1 + C W), pieces (the IDAT chunks' data, views of `data`), banded (whether
    the chunk count is the one png_ops writes, so that a banded decode is worth trying).  ValueError, naming the file and the reason,
    for a file that is not a PNG, is damaged, or is of a kind the device decoder does not take (16-bit and sub-byte depths, palette,
    interlace).  Nothing here touches the device."""
    def bad(why):
        return ValueError(f"png_decode: {name}: {why}")
    view = memoryview(data)
    if bytes(view[:8]) != SIGNATURE:
        raise bad("not a PNG file (signature)")
    pos, n, ihdr, pieces, closed, ended = 8, len(view), None, [], False, False
    while pos < n:
        if ended:
            raise bad("data after IEND")
        if pos + 12 > n:
            raise bad("a chunk header runs past the end of the file")
        (length,) = struct.unpack(">I", view[pos:pos + 4])
        kind = bytes(view[pos + 4:pos + 8])
        if length > n - pos - 12:
            raise bad(f"chunk {kind!r} of {length} bytes runs past the end of the file")
        body = view[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", view[pos + 8 + length:pos + 12 + length])
        if crc != zlib.crc32(view[pos + 4:pos + 8 + length]):
            raise bad(f"CRC-32 of chunk {kind!r} at byte {pos}")
        if ihdr is None and kind != b"IHDR":
            raise bad("the first chunk is not IHDR")
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise bad("IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            if closed:
                raise bad("IDAT chunks are not consecutive")
            pieces.append(body)
        else:
            closed = closed or bool(pieces)
            ended = kind == b"IEND"
        pos += 12 + length
    if ihdr is None:
        raise bad("no IHDR")
    if not ended:
        raise bad("no IEND")
    W, H, depth, colour, comp, filt, lace = ihdr
    if W < 1 or H < 1 or comp != 0 or filt != 0 or lace not in (0, 1):
        raise bad(f"IHDR: {W} x {H}, compression {comp}, filter {filt}, interlace {lace}")
    if colour == 3:
        raise bad("palette images are not decoded on the device")
    if colour not in CHANNELS or depth not in (1, 2, 4, 8, 16):
        raise bad(f"IHDR: colour type {colour}, bit depth {depth}")
    if depth != 8:
        raise bad(f"bit depth {depth}: only 8-bit samples are decoded on the device")
    if lace:
        raise bad("interlaced images are not decoded on the device")
    if not pieces:
        raise bad("no IDAT chunk")
    Cn = CHANNELS[colour]
    S = H * (1 + Cn * W)
    if S >= 1 << 31 or H > 65535:
        raise bad(f"{W} x {H} x {Cn}: beyond the limits of include/gp_png_decode.h")
    return SimpleNamespace(name=name, H=H, W=W, C=Cn, S=S, pieces=pieces, banded=len(pieces) > 1 and len(pieces) == -(-S // BAND_BYTES))


def _arguments(device, dtype, background):
    device = decode_stage.arguments("png_decode", device, dtype)
    if background is not None:
        if not torch.is_tensor(background) or background.numel() != 3 or not background.dtype.is_floating_point:
            raise RuntimeError("png_decode: background must be a tensor of three floats")
        if not background.is_cuda:
            raise RuntimeError(f"png_decode: background is on {background.device} -- HIP kernels only (no CPU fallback)")
        background = background.detach().to(device=device, dtype=torch.float32).reshape(3).contiguous()
    return device, background


def groups(items, channels=None, background=None):
    """The images by shape, in order of first appearance: [((H, W, C), C_out, [index])].  Checked before the device."""
    out = []
    for (H, W, Cn), idx in decode_stage.groups(items, lambda it: (it.H, it.W, it.C)):
        if background is not None and Cn != 4:
            raise ValueError(f"png_decode: {items[idx[0]].name}: a background composites RGBA images, this one has {Cn} channel(s)")
        c_out = 3 if background is not None and channels is None else Cn if channels is None else min(int(channels), Cn)
        if c_out < 1 or (background is not None and c_out != 3):
            raise ValueError(f"png_decode: {items[idx[0]].name}: channels = {c_out} of an image with {Cn}" + (" and a background" if background is not None else ""))
        out.append(((H, W, Cn), c_out, idx))
    return out


def tables(items, banded, idx):
    """The tables of one shape group (the images idx of items) as include/gp_png_decode.h states them: (segments [(image, first payload
    byte, the byte after the last, out_first, out_len)], image_seg [B + 1], copies [(payload offset, piece)], payload bytes).  A banded
    image has one segment per IDAT chunk, writing GP_PNG_BAND_BYTES of the filtered stream each; a serial one is one segment."""
    seg, image_seg, at, copies = [], [0], 0, []
    for b, i in enumerate(idx):
        it = items[i]
        first = at
        for k, piece in enumerate(it.pieces):
            if banded[i]:
                seg.append((b, at, at + len(piece), k * BAND_BYTES, min(BAND_BYTES, it.S - k * BAND_BYTES)))
            copies.append((at, piece))
            at += len(piece)
        if not banded[i]:
            seg.append((b, first, at, 0, it.S))
        image_seg.append(len(seg))
    return seg, image_seg, copies, at


def plans(items, banded, shapes):
    """decode_stage's plan of every shape group: its `tables`."""
    return [decode_stage.plan(idx, (c_out, H, W), *tables(items, banded, idx)) for (H, W, _), c_out, idx in shapes]


def stage(items, banded, shapes, pool=None):
    """The pinned staging buffer of one pass (decode_stage.stage): the segment and image tables, then every group's joined IDAT data with
    the chunk framing gone.  Returns a namespace: buffer, plans (per group: seg, image_seg, bytes and where its parts lie)."""
    return decode_stage.stage(plans(items, banded, shapes), pool)


def launch(staged, up, shapes, words, *, device, dtype, background, guard=0):
    """One gp_png_decode call per shape group on `up`, the staging buffer's copy on the device; words: int32 [2, images] on the device
    for the status and mode words, in group order.  Nothing is read.  Returns (per group the [B, C_out H W + guard] output buffer)."""
    l = lib()

    def call(group, pl, dst, stride, done):
        (H, W, Cn), c_out, idx = group
        scratch = _lib.scratch(l.gp_png_decode_scratch_bytes, len(idx), H, W, Cn, len(pl.seg), device=device)
        _lib.check(l.gp_png_decode(len(idx), H, W, Cn, c_out, DST_U8 if dtype == torch.uint8 else DST_F32, up[pl.pay_at:], pl.bytes,
                                   up[pl.seg_at:], len(pl.seg), up[pl.img_at:], background, dst, stride, words[0, done:], words[1, done:],
                                   scratch, _lib.stream_ptr(device)), "gp_png_decode")

    return decode_stage.launch(shapes, staged.plans, call, device=device, dtype=dtype, guard=guard)


def decode_once(items, banded, *, device, dtype=torch.uint8, channels=None, background=None, guard=0, pool=None):
    """One pass over parsed files (`parse`), image i banded where banded[i]: one pinned staging buffer, one copy up, one gp_png_decode
    call per shape group, ONE read of the status and mode words.  Returns (images: a list of [C_out, H, W] device tensors, views of
    their group's batch; status and modes: lists of ints; slots: per group the whole [B, C_out H W + guard] buffer, whose `guard`
    trailing elements per image were filled with 0xA5 bytes before the call -- the tests look at them)."""
    device, background = _arguments(device, dtype, background)
    if not items:
        return [], [], [], []
    shapes = groups(items, channels, background)
    images, where, read, slots = decode_stage.once(
        plans(items, banded, shapes), (2, len(items)), device=device, pool=pool,
        launch=lambda staged, up, words: launch(staged, up, shapes, words, device=device, dtype=dtype, background=background, guard=guard))
    status, modes = ([row[k] for k in where] for row in read.tolist())
    return images, status, modes, slots


def decode(files, *, device, dtype=torch.uint8, channels=None, background=None, names=None, return_modes=False, resize=None, resample="bicubic",
           _pool=None):
    """PNG files held in memory (a list of bytes) -> a list of [C_out, H, W] tensors on `device`, one per file, in order.
    dtype: torch.uint8, or torch.float32 = byte / 255 (bit-equal to uint8.to(float32) / 255.0).  channels: keep the first `channels`
    channels, as the slice [:channels] would (default: all).  background: three floats on the device -- RGBA files are composited over it to three channels as the
    D-NeRF reader does [REF scene/dataset_readers.py:212-218].  The files are grouped by shape; a group is one launch sequence.  The
    device is read once, and once more only if a file that looked banded was not (those are decoded again as one stream).  A
    damaged file raises GpHipError naming the file and the status word.  return_modes: also the final mode per file
    (MODE_BANDED / MODE_SERIAL).
    resize: (width, height), or a callable (w, h) -> (width, height) -- every image is resized as Image.resize does it, byte for byte
    (resize_ops.resize, filter `resample`): a shape group is decoded as uint8 with all of the file's channels, an RGBA file's alpha
    plane among them, and resized in one batched call; `channels` and `background` apply to the resized image, as [:3] follows
    .resize in the reference [REF metrics.py readImages], and `dtype` last."""
    _arguments(device, dtype, background)                                       # (the device is checked before any file is looked at)
    if resize is not None:
        from . import resize_ops
        resize_ops.filter_id(resample)
    items = decode_stage.parsed("png_decode", files, names, parse)
    kw = dict(device=device, dtype=dtype, channels=channels, background=background, pool=_pool)
    if resize is not None:
        groups(items, channels, background)                                     # (what channels and background ask of the files, before the device)
        for it in items:
            if it.C == 2:
                raise ValueError(f"png_decode: {it.name}: grey + alpha images are not resized on the device")
            resize_ops.target_size(resize, it.W, it.H, it.name)
        kw.update(dtype=torch.uint8, channels=None, background=None)
    banded = [it.banded for it in items]
    images, status, modes, _ = decode_once(items, banded, **kw)
    again = [i for i, s in enumerate(status) if s == NOT_BANDED and banded[i]]
    if again:
        im2, st2, mo2, _ = decode_once([items[i] for i in again], [False] * len(again), **kw)
        for k, i in enumerate(again):
            images[i], status[i], modes[i] = im2[k], st2[k], mo2[k]
    for it, s in zip(items, status):
        if s:
            raise _lib.GpHipError(f"png_decode: {it.name}: the device decoder reports status {s} (GP_PNG_DECODE_{STATUS.get(s, '?')})")
    if resize is not None:
        images = _resized(images, items, resize, resample, dtype, channels, _arguments(device, dtype, background)[1])
    return (images, modes) if return_modes else images


def _resized(images, items, size, resample, dtype, channels, background):
    """decode's resize=: the decoded uint8 images, all channels, through resize_ops.resize_each; then the channel slice, or the
    composite over `background` -- the D-NeRF reader's formula in float64, as gp_png_decode computes it on full-size images -- and
    the conversion to `dtype`."""
    from . import resize_ops
    names = [it.name for it in items]
    if background is None:
        out = resize_ops.resize_each(images, size, resample, dtype=dtype, names=names)
        return out if channels is None else [im[:int(channels)] for im in out]
    bg = background.to(torch.float64).view(3, 1, 1)
    full = torch.full((), 255.0, dtype=torch.float64, device=bg.device)       # (a tensor: torch divides by a Python scalar with a reciprocal)
    out = []
    for im in resize_ops.resize_each(images, size, resample, names=names):
        norm = im.to(torch.float64) / full
        arr = norm[:3] * norm[3:4] + bg * (1.0 - norm[3:4])
        byte = ((arr * full).trunc().to(torch.int64) & 255).to(torch.uint8)
        # (float32 = byte / 255 by the copy path of gp_resize_u8: one correctly rounded division)
        out.append(byte if dtype == torch.uint8 else resize_ops.resize(byte, (byte.shape[2], byte.shape[1]), dtype=torch.float32))
    return out


def decode_files(paths, *, device, dtype=torch.uint8, channels=None, background=None, return_modes=False, resize=None, resample="bicubic"):
    """`decode` of files on disk: at most READER_THREADS threads read and parse them and fill the staging buffer."""
    _arguments(device, dtype, background)
    return decode_stage.decode_files(paths, parse, decode, device=device, dtype=dtype, channels=channels, background=background,
                                     return_modes=return_modes, resize=resize, resample=resample)
