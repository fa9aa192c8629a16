"""Baseline JPEG files decoded on the device (include/gp_jpeg_decode.h, csrc/jpeg_decode_kernels.hip): Huffman decoding with a lane per
restart interval, dequantisation, the integer inverse DCT, chroma upsampling, the colour transform and the planar conversion with its
division by 255 -- what the loaders did per file with a host library -- and the frames of a Motion-JPEG AVI file.

  [REF scene/dataset_readers.py:210-218]   Image.open whatever the dataset holds
  [REF utils/general_utils.py:21-27]       PILtoTorch: resize, / 255.0, permute (the resize: `resize=`, through resize_ops)
  [REF metrics.py:148]                     deltas/%05d.jpg

The host walks the markers (`parse`), finds the restart intervals by their RST markers and copies the scans of all files, with
their segment tables and their quantisation and Huffman tables, into ONE pinned buffer that goes up in one copy.  Every
file jpeg_ops writes carries a restart marker every 8 MCUs; a file without restart markers is one interval, one lane, and slow --
unless `sync` sends it through jpeg_sync, which decodes it on many lanes.
`decode` reads the status words once.  Progressive, extended, arithmetic-coded, 12-bit, greyscale, CMYK, 4:2:2 / 4:4:0 / 4:1:1 and
multi-scan files are refused on the host with a ValueError: the package has no other decoder to fall back to.  HIP only: CPU
devices raise."""
from __future__ import annotations

import ctypes as C
import os
import struct
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, decode_stage
from .decode_stage import DST_F32, DST_U8, MAX_BATCH, READER_THREADS  # noqa: F401  (what include/gp_jpeg_decode.h calls GP_JPEG_DECODE_*)

GP_JPEG_DECODE_ABI_VERSION = 1      # include/gp_jpeg_decode.h
TABLE_BYTES = 1232
SUB_420, SUB_444 = 0, 1             # GP_JPEG_420, GP_JPEG_444 of include/gp_jpeg.h
AVI_BATCH = 32                      # frames per decode call of decode_avi

STATUS = {0: "OK", 1: "TRUNCATED", 2: "NO_CODE", 3: "CATEGORY", 4: "RUN", 5: "TRAILING", 6: "MARKER", 7: "HUFFMAN_TABLE", 8: "TABLE",
          9: "BUDGET"}              # GP_JPEG_DECODE_* (tests/test_jpeg_decode_host.py compares the two)

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_jpeg_decode.h declares them (tests/test_jpeg_decode_host.py compares the two)
        "gp_jpeg_decode_abi_version": (i32, []),
        "gp_jpeg_decode_scratch_bytes": (i64, [i32, i32, i32, i32, i32]),
        "gp_jpeg_decode": (i32, [i32, i32, i32, i32, i32, P, i64, P, i32, P, i32, P, P, i64, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_jpeg_decode.h", "gp_jpeg_decode_abi_version", GP_JPEG_DECODE_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


_SOF_NAMES = {0xc1: "extended sequential (SOF1)", 0xc2: "progressive (SOF2)", 0xc3: "lossless (SOF3)", 0xc5: "differential sequential (SOF5)",
              0xc6: "differential progressive (SOF6)", 0xc7: "differential lossless (SOF7)"}


def parse(data, name="<bytes>"):
    """Walk the markers of a JPEG file held in `data` (bytes): SOI, the tables, SOF0, the one scan and its restart intervals, EOI.
    Returns a namespace: name, H, W, sub (SUB_420 / SUB_444), nmcu, interval (MCUs per restart interval), scan (the entropy-coded
    bytes SOS .. EOI as the file holds them, a view of `data`), seg_at and seg_len (where each of the nseg restart intervals lies
    in it), tables (the TABLE_BYTES of include/gp_jpeg_decode.h).  ValueError, naming
    the file and the reason, for a file that is not a JPEG, is damaged in its markers, or is of a kind the device decoder does not
    take.  Nothing here touches the device."""
    def bad(why):
        return ValueError(f"jpeg_decode: {name}: {why}")
    view = memoryview(data)
    n = len(view)
    if n < 4 or bytes(view[:2]) != b"\xff\xd8":
        raise bad("not a JPEG file (no SOI)")
    qt, huff, sof, dri, adobe, pos = {}, {}, None, 0, None, 2
    while True:
        if pos + 4 > n:
            raise bad("the file ends before a scan")
        if view[pos] != 0xff:
            raise bad(f"byte {pos}: a marker was expected")
        m = view[pos + 1]
        if m == 0xff:                                   # a fill byte
            pos += 1
            continue
        (length,) = struct.unpack(">H", view[pos + 2:pos + 4])
        if length < 2 or pos + 2 + length > n:
            raise bad(f"segment {m:#04x} at byte {pos} runs past the end of the file")
        body = view[pos + 4:pos + 2 + length]
        if m == 0xc0:
            if sof is not None:
                raise bad("two SOF segments")
            if len(body) < 6:
                raise bad("SOF0")
            P, H, W, nc = struct.unpack(">BHHB", body[:6])
            if P != 8:
                raise bad(f"{P}-bit samples: only 8-bit samples are decoded on the device")
            if nc == 1:
                raise bad("one component (greyscale) is not decoded on the device")
            if nc == 4:
                raise bad("four components (CMYK / YCCK) are not decoded on the device")
            if nc != 3 or len(body) != 6 + 3 * nc:
                raise bad(f"SOF0: {nc} components")
            if H == 0:
                raise bad("height 0: the number of lines comes in a DNL segment, which is not decoded on the device")
            if W == 0:
                raise bad("SOF0: width 0")
            sof = (H, W, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)])
        elif m in _SOF_NAMES:
            raise bad(f"{_SOF_NAMES[m]} is not decoded on the device: baseline sequential (SOF0) only")
        elif m in (0xc9, 0xca, 0xcb, 0xcc, 0xcd, 0xce, 0xcf):
            raise bad("arithmetic coding is not decoded on the device")
        elif m == 0xc4:
            at = 0
            while at < len(body):
                if at + 17 > len(body):
                    raise bad("DHT")
                tc, th = body[at] >> 4, body[at] & 15
                bits = bytes(body[at + 1:at + 17])
                cnt = sum(bits)
                if tc > 1 or th > 1:
                    raise bad(f"DHT: table class {tc}, id {th} (baseline has ids 0 and 1)")
                if cnt > 256 or at + 17 + cnt > len(body):
                    raise bad("DHT")
                huff[(tc, th)] = bits + bytes(body[at + 17:at + 17 + cnt]) + bytes(256 - cnt)
                at += 17 + cnt
        elif m == 0xdb:
            at = 0
            while at < len(body):
                pq, tq = body[at] >> 4, body[at] & 15
                if pq == 1:
                    raise bad("16-bit quantisation table (DQT): only 8-bit tables are decoded on the device")
                if pq or tq > 3 or at + 65 > len(body):
                    raise bad("DQT")
                nat = bytearray(64)
                for k in range(64):
                    nat[ZIGZAG[k]] = body[at + 1 + k]
                qt[tq] = bytes(nat)
                at += 65
        elif m == 0xdd:
            if len(body) != 2:
                raise bad("DRI")
            (dri,) = struct.unpack(">H", body)
        elif m == 0xdc:
            raise bad("DNL is not decoded on the device")
        elif m == 0xee and len(body) >= 12 and bytes(body[:5]) == b"Adobe":
            adobe = body[11]
        elif m == 0xda:
            break
        elif m == 0xd9:
            raise bad("EOI before a scan")
        elif not (0xe0 <= m <= 0xef or m == 0xfe):     # APPn and COM are skipped
            raise bad(f"marker {m:#04x} at byte {pos}")
        pos += 2 + length
    if sof is None:
        raise bad("SOS before SOF0")
    H, W, comps = sof
    if adobe is not None and adobe != 1:
        raise bad(f"Adobe APP14 with colour transform {adobe}: only Y Cb Cr (transform 1) is decoded on the device")
    if adobe is None and bytes(c[0] for c in comps) == b"RGB":
        raise bad("components named R, G, B without a colour transform are not decoded on the device")
    samp = [(c[1], c[2]) for c in comps]
    if samp == [(2, 2), (1, 1), (1, 1)]:
        sub, ms = SUB_420, 16
    elif samp == [(1, 1), (1, 1), (1, 1)]:
        sub, ms = SUB_444, 8
    else:
        raise bad("sampling factors " + " ".join(f"{h}x{v}" for h, v in samp) + ": only 4:4:4 (1x1 1x1 1x1) and 4:2:0 (2x2 1x1 1x1) are decoded on the device")
    ns = body[0] if len(body) else 0
    if ns != 3:
        raise bad(f"a scan of {ns} component(s): more than one scan is not decoded on the device")
    if len(body) != 1 + 2 * ns + 3:
        raise bad("SOS")
    if bytes(body[-3:]) != b"\x00\x3f\x00":
        raise bad(f"SOS: Ss = {body[-3]}, Se = {body[-2]}, Ah/Al = {body[-1]:#04x} (baseline has 0, 63, 0)")
    sel = bytearray(16)
    tqs = []
    for i in range(3):
        cs, t = body[1 + 2 * i], body[2 + 2 * i]
        if cs != comps[i][0]:
            raise bad("SOS: the scan's components are not the frame's, in order")
        td, ta = t >> 4, t & 15
        if td > 1 or ta > 1 or (0, td) not in huff or (1, ta) not in huff:
            raise bad(f"SOS: component {i} uses Huffman tables DC {td}, AC {ta}, which the file does not define (ids 0 and 1)")
        if comps[i][3] not in qt:
            raise bad(f"component {i} uses quantisation table {comps[i][3]}, which the file does not define")
        if comps[i][3] not in tqs:
            tqs.append(comps[i][3])
        sel[i], sel[3 + i], sel[6 + i] = tqs.index(comps[i][3]), td, ta
    if len(tqs) > 2:
        raise bad("three different quantisation tables: the device decoder takes two")
    empty = bytes(272)
    tables = bytes(sel) + qt[tqs[0]] + qt[tqs[-1]] + b"".join(huff.get(k, empty) for k in ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert len(tables) == TABLE_BYTES
    # the scan: every 0xFF that is followed by neither 0x00 nor 0xFF; it ends at the first marker that is not RSTn.  Bytes 0x01 .. 0xBF
    # behind a 0xFF are no segment markers: they stay in their interval, where the device reports them
    start = pos + 2 + length
    arr = np.frombuffer(view, dtype=np.uint8)
    ff = np.flatnonzero(arr[start:n - 1] == 0xff) + start
    nxt = arr[ff + 1]
    keep = nxt >= 0xc0
    keep &= nxt != 0xff
    ff, nxt = ff[keep], nxt[keep]
    rst = (nxt >= 0xd0) & (nxt <= 0xd7)
    ends = np.flatnonzero(~rst)
    if not len(ends):
        raise bad("no EOI: the scan runs to the end of the file")
    k = int(ends[0])
    end, after = int(ff[k]), int(nxt[k])
    if after == 0xda or after == 0xc4 or after == 0xdb:
        raise bad("more than one scan is not decoded on the device")
    if after == 0xdc:
        raise bad("DNL is not decoded on the device")
    if after != 0xd9:
        raise bad(f"marker {after:#04x} at byte {end} behind the scan")
    marks = ff[:k]
    if len(marks) and not np.array_equal(nxt[:k] - 0xd0, np.arange(len(marks)) % 8):
        raise bad("the RST markers do not count 0 .. 7 in turn")
    mw, mh = -(-W // ms), -(-H // ms)
    nmcu = mw * mh
    interval = dri if dri else nmcu
    if len(marks) + 1 != -(-nmcu // interval):
        raise bad(f"{len(marks) + 1} restart interval(s) where {nmcu} MCUs at DRI = {dri} make {-(-nmcu // interval)}")
    seg_at = np.concatenate([[0], marks - start + 2]).astype(np.int64)          # the intervals inside the scan, their RST markers left out
    seg_len = np.concatenate([marks, [end]]).astype(np.int64) - start - seg_at
    return SimpleNamespace(name=name, H=H, W=W, sub=sub, nmcu=nmcu, interval=interval, scan=view[start:end], seg_at=seg_at, seg_len=seg_len,
                           nseg=len(seg_at), tables=tables)


def pieces(item):
    """The restart intervals of a parsed file, as bytes."""
    return [bytes(item.scan[a:a + n]) for a, n in zip(item.seg_at.tolist(), item.seg_len.tolist())]


def groups(items):
    """The images by shape and subsampling, in order of first appearance: [((H, W, sub), [index])]."""
    return decode_stage.groups(items, lambda it: (it.H, it.W, it.sub))


def tables(items, idx):
    """The tables of one shape group (the images idx of items) as include/gp_jpeg_decode.h states them: (segments: int64 [nseg, 5] of
    (image, first payload byte, byte count, first MCU, MCU count), image_seg [B + 1], copies [(payload offset, scan)], payload bytes,
    the largest segment count of an image).  A file's scan goes into the payload whole, in one copy; its RST markers lie between
    the segments' ranges."""
    seg, image_seg, at, copies, most = [], [0], 0, [], 1
    for b, i in enumerate(idx):
        it = items[i]
        first = np.arange(it.nseg, dtype=np.int64) * it.interval
        seg.append(np.stack([np.full(it.nseg, b, dtype=np.int64), it.seg_at + at, it.seg_len, first, np.minimum(it.interval, it.nmcu - first)], axis=1))
        copies.append((at, it.scan))
        at += len(it.scan)
        image_seg.append(image_seg[-1] + it.nseg)
        most = max(most, it.nseg)
    return np.concatenate(seg), image_seg, copies, at, most


def plans(items, shapes):
    """decode_stage's plan of every shape group: its `tables` and the images' quantisation and Huffman tables."""
    return [decode_stage.plan(idx, (3, H, W), *tables(items, idx), tables=b"".join(items[i].tables for i in idx)) for (H, W, _), idx in shapes]


def stage(items, shapes, pool=None):
    """The pinned staging buffer of one pass (decode_stage.stage): the segment and image tables, every image's quantisation and Huffman
    tables, then every group's scans.  Returns a namespace: buffer, plans (per group: seg, image_seg, bytes, most and where its parts lie)."""
    return decode_stage.stage(plans(items, shapes), pool)


def launch(staged, up, shapes, words, *, device, dtype, guard=0):
    """One gp_jpeg_decode call per shape group on `up`, the staging buffer's copy on the device; words: int32 [images] on the device
    for the status words, in group order.  Nothing is read.  Returns (per group the [B, 3 H W + guard] output buffer)."""
    l = lib()

    def call(group, pl, dst, stride, done):
        (H, W, sub), idx = group
        scratch = _lib.scratch(l.gp_jpeg_decode_scratch_bytes, len(idx), H, W, sub, len(pl.seg), device=device)
        _lib.check(l.gp_jpeg_decode(len(idx), H, W, sub, DST_U8 if dtype == torch.uint8 else DST_F32, up[pl.pay_at:], pl.bytes, up[pl.seg_at:],
                                    len(pl.seg), up[pl.img_at:], pl.most, up[pl.tab_at:], dst, stride, words[done:], scratch,
                                    _lib.stream_ptr(device)), "gp_jpeg_decode")

    return decode_stage.launch(shapes, staged.plans, call, device=device, dtype=dtype, guard=guard)


def decode_once(items, *, device, dtype=torch.uint8, guard=0, pool=None):
    """One pass over parsed files (`parse`): one pinned staging buffer, one copy up, one gp_jpeg_decode call per shape group, ONE read
    of the status words.  Returns (images: a list of [3, H, W] device tensors, views of their group's batch; status: a list of ints;
    slots: per group the whole [B, 3 H W + guard] buffer, whose `guard` trailing elements per image were filled with 0xA5 bytes
    before the call -- the tests look at them)."""
    device = decode_stage.arguments("jpeg_decode", device, dtype)
    if not items:
        return [], [], []
    shapes = groups(items)
    images, where, read, slots = decode_stage.once(
        plans(items, shapes), (len(items),), device=device, pool=pool,
        launch=lambda staged, up, words: launch(staged, up, shapes, words, device=device, dtype=dtype, guard=guard))
    read = read.tolist()
    return images, [read[k] for k in where], slots


def _sync_flag(sync):
    if sync is not False and sync is not True and sync != "auto":
        raise RuntimeError(f"jpeg_decode: sync must be False, True or \"auto\" (got {sync!r})")
    return bool(sync)


def decode(files, *, device, dtype=torch.uint8, names=None, sync=False, resize=None, resample="bicubic", _pool=None):
    """JPEG files held in memory (a list of bytes) -> a list of [3, H, W] R G B tensors on `device`, one per file, in order.
    dtype: torch.uint8, or torch.float32 = byte / 255 (bit-equal to uint8.to(float32) / 255.0).  The files are grouped by shape and
    subsampling; a group is one launch sequence.  The device is read once.  A damaged file raises GpHipError naming the file and the
    status word.
    sync: True or "auto" sends the files without restart markers that jpeg_sync.eligible takes through jpeg_sync.decode_once (many
    lanes per file instead of one); what comes back SERIAL there, and every other file, goes through the one-lane call in a second
    pass, so the pixels and every error are those of sync=False.  Off by default.
    resize: (width, height), or a callable (w, h) -> (width, height) -- every image is decoded as uint8 and resized as Image.resize
    does it, byte for byte (resize_ops.resize, filter `resample`), one batched call per shape group; `dtype` applies to the result."""
    decode_stage.arguments("jpeg_decode", device, dtype)                        # (the device is checked before any file is looked at)
    sync = _sync_flag(sync)
    out_dtype = dtype
    if resize is not None:
        from . import resize_ops
        resize_ops.filter_id(resample)
        dtype = torch.uint8
    items = decode_stage.parsed("jpeg_decode", files, names, parse)
    if resize is not None:
        for it in items:
            resize_ops.target_size(resize, it.W, it.H, it.name)                 # (a target size of 0 names its file, before the device)
    images, rest = [None] * len(items), list(range(len(items)))
    if sync:
        from . import jpeg_sync
        fast = [i for i in rest if jpeg_sync.eligible(items[i])]
        got, words, _ = jpeg_sync.decode_once([items[i] for i in fast], device=device, dtype=dtype, pool=_pool)
        for i, im, s in zip(fast, got, words):
            if s == jpeg_sync.OK:
                images[i] = im
        rest = [i for i in rest if images[i] is None]
    got, status, _ = decode_once([items[i] for i in rest], device=device, dtype=dtype, pool=_pool)
    for i, im, s in zip(rest, got, status):
        if s:
            raise _lib.GpHipError(f"jpeg_decode: {items[i].name}: the device decoder reports status {s} (GP_JPEG_DECODE_{STATUS.get(s, '?')})")
        images[i] = im
    if resize is not None:
        images = resize_ops.resize_each(images, resize, resample, dtype=out_dtype, names=[it.name for it in items])
    return images


def decode_files(paths, *, device, dtype=torch.uint8, sync=False, resize=None, resample="bicubic"):
    """`decode` of files on disk: at most READER_THREADS threads read and parse them and fill the staging buffer."""
    decode_stage.arguments("jpeg_decode", device, dtype)
    _sync_flag(sync)
    return decode_stage.decode_files(paths, parse, decode, device=device, dtype=dtype, sync=sync, resize=resize, resample=resample)


# ---- Motion-JPEG in AVI ----------------------------------------------------------------------------------------------------------------
def avi_frames(data, name="<bytes>"):
    """Walk a RIFF 'AVI ' file as jpeg_ops.AviFile writes it -- LIST hdrl (avih, LIST strl (strh, strf)), LIST movi ('00dc' chunks),
    idx1 -- and return (width, height, [the frames' bytes, views of `data`]).  ValueError for anything that is not one MJPG video
    stream, or whose sizes or index do not add up."""
    def bad(why):
        return ValueError(f"jpeg_decode: {name}: {why}")
    view = memoryview(data)
    n = len(view)
    if n < 12 or bytes(view[:4]) != b"RIFF" or bytes(view[8:12]) != b"AVI ":
        raise bad("not a RIFF 'AVI ' file")
    if struct.unpack("<I", view[4:8])[0] + 8 > n:
        raise bad("the RIFF chunk runs past the end of the file")
    found = {"frames": [], "offsets": [], "index": None, "streams": [], "movi": None}

    def chunks(lo, hi):
        pos = lo
        while pos + 8 <= hi:
            cid, size = bytes(view[pos:pos + 4]), struct.unpack("<I", view[pos + 4:pos + 8])[0]
            end = pos + 8 + size
            if end > hi:
                raise bad(f"chunk {cid!r} at byte {pos} runs past its list")
            if cid == b"LIST":
                if size < 4:
                    raise bad("LIST")
                if bytes(view[pos + 8:pos + 12]) == b"movi":
                    found["movi"] = pos + 8
                chunks(pos + 12, end)
            elif cid == b"avih":
                found["avih"] = view[pos + 8:end]
            elif cid == b"strh":
                found["streams"].append(view[pos + 8:end])
            elif cid == b"strf":
                found["strf"] = view[pos + 8:end]
            elif cid == b"idx1":
                found["index"] = [struct.unpack("<4sIII", view[pos + 8 + 16 * i:pos + 24 + 16 * i]) for i in range(size // 16)]
            elif cid[2:] in (b"dc", b"db", b"wb", b"pc"):
                if cid != b"00dc":
                    raise bad(f"chunk {cid!r}: not one compressed video stream")
                found["frames"].append(view[pos + 8:end])
                found["offsets"].append(pos)
            pos = end + (size & 1)                      # chunks are padded to an even length

    chunks(12, n)
    if len(found["streams"]) != 1 or "avih" not in found or "strf" not in found or found["movi"] is None:
        raise bad(f"{len(found['streams'])} stream(s): exactly one video stream is read")
    strh, strf = found["streams"][0], found["strf"]
    if len(strh) < 8 or len(strf) < 40 or bytes(strh[:4]) != b"vids" or bytes(strf[16:20]).upper() != b"MJPG":
        raise bad("the stream is not MJPG video")
    width, height = struct.unpack("<ii", strf[4:12])
    if found["index"] is not None:
        want = [(b"00dc", off - found["movi"], len(f)) for off, f in zip(found["offsets"], found["frames"])]
        if [(c, o, s) for c, _, o, s in found["index"]] != want:
            raise bad("idx1 does not list the frames of movi")
    return width, abs(height), found["frames"]


def decode_avi(path, *, device, dtype=torch.uint8, frames=None, sync=False, resize=None, resample="bicubic"):
    """The frames of a Motion-JPEG AVI file (one MJPG video stream, as jpeg_ops.VideoWriter writes it) as one [F, 3, H, W] tensor on
    `device`.  frames: the frame numbers to decode, in the order wanted (default: all).  AVI_BATCH frames per decode call.  sync: as
    `decode` -- the frames other encoders write carry no restart markers.  resize, resample: as `decode`; the result is then
    [F, 3, height, width]."""
    device = decode_stage.arguments("jpeg_decode", device, dtype)
    _sync_flag(sync)
    if resize is not None:
        from . import resize_ops
        resize_ops.filter_id(resample)
    path = os.fspath(path)
    with open(path, "rb") as fp:
        data = fp.read()
    width, height, all_frames = avi_frames(data, path)
    pick = list(range(len(all_frames))) if frames is None else [int(f) for f in frames]
    for f in pick:
        if not 0 <= f < len(all_frames):
            raise ValueError(f"jpeg_decode: {path}: frame {f} of {len(all_frames)}")
    items = [parse(all_frames[f], f"{path}#{f}") for f in pick]
    for it in items:
        if (it.W, it.H) != (width, height):
            raise ValueError(f"jpeg_decode: {it.name}: a frame of {it.H} x {it.W} in a video of {height} x {width}")
    if resize is not None:
        width, height = resize_ops.target_size(resize, width, height, path)
    out = torch.empty(len(items), 3, height, width, dtype=dtype, device=device)
    for lo in range(0, len(items), AVI_BATCH):
        imgs = decode(items[lo:lo + AVI_BATCH], device=device, dtype=dtype, sync=sync, resize=resize, resample=resample)
        out[lo:lo + len(imgs)] = torch.stack(imgs)
    return out
