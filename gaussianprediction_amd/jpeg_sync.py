"""Baseline JPEG files WITHOUT restart markers decoded on many lanes (include/gp_jpeg_sync.h, csrc/jpeg_sync_kernels.hip): the
self-synchronising entropy stage in front of jpeg_decode's transform and pixel stage.  Such a file is one restart interval, which
jpeg_decode gives to ONE lane; here its scan is cut into subsequences of S bytes, a lane starts at every cut with a guessed state, and
the lanes are corrected from their left neighbours until nothing changes -- a fixpoint that proves the result, whatever the file
(Weissenberger and Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).

`decode_once` is the whole interface; jpeg_decode.decode(..., sync=True) routes the files that are `eligible` through it and sends what
comes back SERIAL (a stream that is not well formed) through the one-lane path, which names the GP_JPEG_DECODE_* word.  HIP only."""
from __future__ import annotations

import ctypes as ct

import torch

from . import _lib, decode_stage, jpeg_decode

GP_JPEG_SYNC_ABI_VERSION = 1        # include/gp_jpeg_sync.h
S = 128                             # GP_JPEG_SYNC_SUBSEQ_BYTES: bytes of the stuffed scan per lane
C = 256                            # GP_JPEG_SYNC_CHUNK: subsequences per workgroup
STATUS = {0: "OK", 1: "SERIAL"}     # GP_JPEG_SYNC_* (tests/test_jpeg_sync_host.py compares the two)
OK, SERIAL = 0, 1
# A scan below 8 S = 1024 bytes has at most eight lanes' worth of work and is a few hundred symbols on one lane; the stage's six further
# launches (ten against four) cost about what that one lane does.  From there on more lanes win.  (Reasoned from the launch counts;
# DESIGN §17 has what was measured.)
MIN_BYTES = 8 * S


def _prototypes():
    i32, i64, P = ct.c_int32, ct.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_jpeg_sync.h declares them (tests/test_jpeg_sync_host.py compares the two)
        "gp_jpeg_sync_abi_version": (i32, []),
        "gp_jpeg_sync_scratch_bytes": (i64, [i32, i32, i32, i32, i64]),
        "gp_jpeg_sync_decode": (i32, [i32, i32, i32, i32, i32, P, i64, P, i32, P, i32, P, P, i64, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_jpeg_sync.h", "gp_jpeg_sync_abi_version", GP_JPEG_SYNC_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def eligible(item) -> bool:
    """A parsed file (jpeg_decode.parse) this stage is for: one segment -- no restart markers -- and a scan of at least MIN_BYTES."""
    return item.nseg == 1 and len(item.scan) >= MIN_BYTES


def launch(staged, up, shapes, words, *, device, dtype, guard=0):
    """One gp_jpeg_sync_decode call per shape group on `up`, the staging buffer's copy on the device; words: int32 [images, 5] on the
    device: per group its status words, then its info words.  Nothing is read.  Returns (per group the [B, 3 H W + guard] output
    buffer; per group (scratch, pad, bytes) where guard bytes were laid round the scratch)."""
    l, fences = lib(), []
    pad = -(-int(guard) // 256) * 256                                          # (the scratch itself stays 256-byte aligned)

    def call(group, pl, dst, stride, done):
        (H, W, sub), idx = group
        B = len(idx)
        scratch = _lib.scratch(l.gp_jpeg_sync_scratch_bytes, B, H, W, sub, pl.bytes, device=device, extra=2 * pad)
        n = scratch.numel() - 2 * pad
        if guard:
            scratch[:pad].fill_(0xA5)
            scratch[pad + n:].fill_(0xA5)
            fences.append((scratch, pad, n))
        mine = words[done:done + B].view(-1)
        _lib.check(l.gp_jpeg_sync_decode(B, H, W, sub, jpeg_decode.DST_U8 if dtype == torch.uint8 else jpeg_decode.DST_F32, up[pl.pay_at:], pl.bytes,
                                         up[pl.seg_at:], len(pl.seg), up[pl.img_at:], pl.most, up[pl.tab_at:], dst, stride, mine[:B], mine[B:],
                                         scratch[pad:], _lib.stream_ptr(device)), "gp_jpeg_sync_decode")

    return decode_stage.launch(shapes, staged.plans, call, device=device, dtype=dtype, guard=guard), fences


def decode_once(items, *, device, dtype=torch.uint8, guard=0, pool=None):
    """One pass over parsed files of one segment each (jpeg_decode.parse): staged as jpeg_decode.decode_once stages them (one pinned
    buffer, one copy up), one gp_jpeg_sync_decode call per shape group, ONE read of the status and info words.  Returns (images: a list
    of [3, H, W] device tensors; status: a list of OK / SERIAL; info: a list of (subsequences, chunks, most rounds inside a chunk,
    rounds across chunks)).  guard: that many elements behind every output slot, and that many bytes on both sides of the scratch
    buffer, are filled with 0xA5 before the call and checked after it (RuntimeError) -- the tests ask for it."""
    device = decode_stage.arguments("jpeg_sync", device, dtype)
    if not items:
        return [], [], []
    for it in items:
        if it.nseg != 1:
            raise RuntimeError(f"jpeg_sync: {it.name}: {it.nseg} restart intervals -- this stage takes files without restart markers (jpeg_decode.decode takes the rest)")
    shapes, guard, fences = jpeg_decode.groups(items), int(guard), []

    def go(staged, up, words):
        slots, fenced = launch(staged, up, shapes, words, device=device, dtype=dtype, guard=guard)
        fences.extend(fenced)
        return slots

    images, _, read, slots = decode_stage.once(jpeg_decode.plans(items, shapes), (len(items), 5), go, device=device, pool=pool)
    with _lib.on_device(device):
        for scratch, pad, n in fences:
            if not (bool((scratch[:pad] == 0xA5).all()) and bool((scratch[pad + n:] == 0xA5).all())):
                raise RuntimeError("jpeg_sync: a kernel wrote outside its scratch buffer")
        if guard:
            for dst in slots:
                if not bool((dst[:, -guard:].contiguous().view(torch.uint8) == 0xA5).all()):
                    raise RuntimeError("jpeg_sync: a kernel wrote behind an output slot")
    status, info, k = [0] * len(items), [None] * len(items), 0
    for _, idx in shapes:
        B = len(idx)
        flat = read[k:k + B].reshape(-1).tolist()
        for b, i in enumerate(idx):
            status[i] = flat[b]
            info[i] = tuple(v & 0xffffffff for v in flat[B + 4 * b:B + 4 * b + 4])
        k += B
    return images, status, info
