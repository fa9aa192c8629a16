"""What png_decode, jpeg_decode and jpeg_sync do around their one library call, written once: the argument checks, the shape groups,
the byte layout of the staging buffer, its fill, the launch loop over the groups, the one-copy one-read pass and the reader pool.
Nothing here knows a file format: a decoder describes each shape group by a `plan` and makes its library call in a closure."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

MAX_BATCH = 65535
READER_THREADS = 4
DST_U8, DST_F32 = 0, 1


def arguments(who, device, dtype):
    """The device a decoder runs on (a `cuda` one, with its index) and the check of its output dtype."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: device {device} -- HIP kernels only (no CPU fallback)")
    if dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"{who}: dtype must be torch.uint8 or torch.float32 (got {dtype})")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def parsed(who, files, names, parse):
    """decode's files (bytes, or what `parse` returned already) -> the parsed items, named `names` or <file i>."""
    files = list(files)
    names = [f"<file {i}>" for i in range(len(files))] if names is None else [os.fspath(n) for n in names]
    if len(names) != len(files):
        raise RuntimeError(f"{who}: {len(files)} files but {len(names)} names")
    return [f if isinstance(f, SimpleNamespace) else parse(f, n) for f, n in zip(files, names)]


def groups(items, key):
    """The items by key(item), in order of first appearance and cut at MAX_BATCH: [(key, [index])]."""
    by_key = {}
    for i, it in enumerate(items):
        by_key.setdefault(key(it), []).append(i)
    return [(k, idx[lo:lo + MAX_BATCH]) for k, idx in by_key.items() for lo in range(0, len(idx), MAX_BATCH)]


def plan(idx, shape, seg, image_seg, copies, nbytes, most=1, tables=b""):
    """One shape group: idx (its files), shape (C, H, W of an output image), seg (rows of five: a list of tuples or an int64 array),
    image_seg [B + 1], copies [(payload offset, piece)], bytes (of payload), most (the largest segment count of an image, where the
    decoder's tables() counts it), tables (the images' table bytes, joined; none for PNG)."""
    return SimpleNamespace(idx=idx, shape=shape, seg=seg, image_seg=image_seg, copies=copies, bytes=nbytes, most=most, tables=tables)


def layout(plans):
    """Where every plan's parts lie in the ONE buffer the library calls read (seg_at, img_at, tab_at, pay_at); returns the buffer's
    size.  All segment tables from offset 0 (int64, 40 bytes a row), all image tables behind them (int32), the table bytes at the
    next multiple of 16, the payload at the next multiple of 256 with every group's share rounded up to 16 bytes, 16 spare bytes."""
    seg_at, img_at = 0, 40 * sum(len(pl.seg) for pl in plans)
    tab_at = -(-(img_at + 4 * sum(len(pl.image_seg) for pl in plans)) // 16) * 16
    pay_at = -(-(tab_at + sum(len(pl.tables) for pl in plans)) // 256) * 256
    for pl in plans:
        pl.seg_at, pl.img_at, pl.tab_at, pl.pay_at = seg_at, img_at, tab_at, pay_at
        seg_at, img_at, tab_at = seg_at + 40 * len(pl.seg), img_at + 4 * len(pl.image_seg), tab_at + len(pl.tables)
        pay_at += -(-pl.bytes // 16) * 16
    return pay_at + 16


def fill(host, plans, pool=None):
    """Write laid-out plans into `host`, a writable uint8 numpy array of layout's size; the payload pieces through `pool` if given."""
    for pl in plans:
        host[pl.seg_at:pl.seg_at + 40 * len(pl.seg)].view(np.int64)[:] = np.asarray(pl.seg, dtype=np.int64).reshape(-1)
        host[pl.img_at:pl.img_at + 4 * len(pl.image_seg)].view(np.int32)[:] = np.asarray(pl.image_seg, dtype=np.int32)
        host[pl.tab_at:pl.tab_at + len(pl.tables)] = np.frombuffer(pl.tables, dtype=np.uint8)

    def copy(job):
        at, piece = job
        host[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)

    jobs = [(pl.pay_at + at, piece) for pl in plans for at, piece in pl.copies]
    if pool is not None and len(jobs) > 1:
        list(pool.map(copy, jobs, chunksize=max(1, len(jobs) // (4 * READER_THREADS))))
    else:
        for job in jobs:
            copy(job)


def stage(plans, pool=None):
    """The pinned staging buffer of one pass.  Returns a namespace: buffer, plans (laid out)."""
    staging = torch.empty(layout(plans), dtype=torch.uint8, pin_memory=True)
    fill(staging.numpy(), plans, pool)
    return SimpleNamespace(buffer=staging, plans=plans)


def launch(shapes, plans, call, *, device, dtype, guard=0):
    """Per shape group: the [B, C H W + guard] output buffer, its guard elements filled with 0xA5 bytes, then the decoder's library
    call, call(group, plan, dst, stride, done); done: the images of the groups before.  Returns the buffers."""
    slots, done, guard = [], 0, int(guard)
    with _lib.on_device(device):
        for group, pl in zip(shapes, plans):
            B, stride = len(pl.idx), pl.shape[0] * pl.shape[1] * pl.shape[2] + guard
            dst = torch.empty(B, stride, dtype=dtype, device=device)
            if guard:
                dst.view(torch.uint8).fill_(0xA5)
            call(group, pl, dst, stride, done)
            slots.append(dst)
            done += B
    return slots


def once(plans, words_shape, launch, *, device, pool=None):
    """One pass: `stage`, ONE copy of the buffer up, launch(staged, up, words) -> the groups' output buffers, ONE read of words (int32
    of words_shape on the device).  Returns (images: per file its [C, H, W] view of its group's buffer; where: per file the number of
    its image in group order, as the words count them; the words on the host; the buffers)."""
    staged = stage(plans, pool)
    with _lib.on_device(device):
        up = staged.buffer.to(device, non_blocking=True)                        # the one copy
        words = torch.empty(*words_shape, dtype=torch.int32, device=device)
        slots = launch(staged, up, words)
        read = words.cpu()                                                      # the one read (it also ends the staging buffer's use)
    order = [i for pl in plans for i in pl.idx]
    images = [None] * len(order)
    for pl, dst in zip(plans, slots):
        for b, i in enumerate(pl.idx):
            images[i] = dst[b, :pl.shape[0] * pl.shape[1] * pl.shape[2]].view(pl.shape)
    return images, sorted(range(len(order)), key=order.__getitem__), read, slots


def decode_files(paths, parse, decode, **kw):
    """decode(..., **kw) of files on disk: at most READER_THREADS threads read and parse them and fill the staging buffer."""
    paths = [os.fspath(p) for p in paths]

    def load(path):
        with open(path, "rb") as fp:
            return parse(fp.read(), path)

    with ThreadPoolExecutor(max_workers=max(1, min(READER_THREADS, len(paths)))) as pool:
        return decode(list(pool.map(load, paths)), names=paths, _pool=pool, **kw)
