"""PNG files encoded on the device (include/gp_png.h, csrc/png_kernels.hip): quantisation, the row filters, a run-length + dynamic-Huffman
deflate per band of the filtered stream, Adler-32, every chunk with its CRC-32 -- the bytes that come back are the file.

  [REF eval.py:110,146,155,182,185,217,220]    torchvision.utils.save_image after every rendered frame

`encode` reads nothing from the device; `encode_to_bytes` reads once; `PngWriter` copies the files into pinned buffers behind the
encode and leaves the waiting and the disk to worker threads.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import queue
import threading

import torch

from . import _lib

GP_PNG_ABI_VERSION = 1              # include/gp_png.h
BAND_BYTES = 16384
MAX_BATCH = 65535
SRC_F32, SRC_U8 = 0, 1
FILTER_NONE = 1


def _prototypes():
    i32, i64, u32, P = C.c_int32, C.c_int64, C.c_uint32, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_png.h declares them (tests/test_png_host.py compares the two)
        "gp_png_abi_version": (i32, []),
        "gp_png_bound": (i64, [i32, i32]),
        "gp_png_scratch_bytes": (i64, [i32, i32, i32]),
        "gp_png_encode": (i32, [i32, i32, i32, P, i32, u32, P, i64, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_png.h", "gp_png_abi_version", GP_PNG_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def bound(H, W) -> int:
    """The largest file an H x W image can become, in bytes (a multiple of 8); ValueError outside the limits of gp_png.h."""
    n = int(lib().gp_png_bound(int(H), int(W)))
    if n < 0:
        raise ValueError(f"png_ops.bound: {_lib.last_error()}")
    return n


def _batch(images):
    """A contiguous [B, 3, H, W] float32 or uint8 device tensor from a tensor ([B,3,H,W] / [3,H,W]) or a list of [3,H,W] tensors.
    Shape and dtype are checked before the device, and all of it before anything is launched."""
    if isinstance(images, (list, tuple)):
        if not images:
            raise RuntimeError("png_ops: no images")
        for im in images:
            if not torch.is_tensor(im) or im.dim() != 3 or im.shape != images[0].shape or im.dtype != images[0].dtype:
                raise RuntimeError("png_ops: images must be tensors of one shape [3,H,W] and one dtype")
        for im in images:
            if not im.is_cuda:
                raise RuntimeError(f"png_ops: images are on {im.device} -- HIP kernels only (no CPU fallback)")
        images = torch.stack([im.detach() for im in images])
    if not torch.is_tensor(images):
        raise TypeError(f"png_ops: images must be a tensor or a list of tensors (got {type(images).__name__})")
    x = images.detach()
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"png_ops: images must be [B,3,H,W] or [3,H,W] (got {tuple(images.shape)})")
    if x.dtype != torch.uint8 and not x.dtype.is_floating_point:
        raise RuntimeError(f"png_ops: images must be uint8 or a float dtype (got {x.dtype})")
    if not 1 <= x.shape[0] <= MAX_BATCH:
        raise RuntimeError(f"png_ops: B = {x.shape[0]} outside [1, {MAX_BATCH}]")
    if not x.is_cuda:
        raise RuntimeError(f"png_ops: images are on {x.device} -- HIP kernels only (no CPU fallback)")
    if x.dtype != torch.uint8:
        x = x.to(torch.float32)
    return x.contiguous()


def encode(images, *, filter_none=False, out=None):
    """(buffer [B, stride] uint8, sizes [B] int32), both on the device: buffer[b, :sizes[b]] is the complete PNG file of image b (8-bit
    RGB; float input quantised as floor(x * 255 + 0.5) clamped, NaN -> 0), stride = bound(H, W).  The rest of a row is not written.
    filter_none: every row filter type 0.  out: a contiguous [B, stride >= bound(H, W)] uint8 device tensor to receive the files.
    Nothing is read from the device."""
    x = _batch(images)
    B, _, H, W = x.shape
    dev = x.device
    stride = bound(H, W)
    scratch = _lib.scratch(lib().gp_png_scratch_bytes, B, H, W, device=dev)
    if out is None:
        out = torch.empty(B, stride, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != dev or out.dim() != 2 or out.shape[0] != B
          or out.shape[1] < stride or not out.is_contiguous()):
        raise RuntimeError(f"png_ops.encode: out must be a contiguous [{B}, >= {stride}] uint8 tensor on {dev}")
    sizes = torch.empty(B, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_png_encode(B, H, W, x, SRC_U8 if x.dtype == torch.uint8 else SRC_F32, FILTER_NONE if filter_none else 0,
                                       out, out.shape[1], sizes, scratch, _lib.stream_ptr(dev)), "gp_png_encode")
    return out, sizes


def encode_to_bytes(images, *, filter_none=False):
    """The files as a list of bytes: one read of the device (the sizes ride behind the buffer in one tensor)."""
    return files_to_bytes(*encode(images, filter_none=filter_none))


def files_to_bytes(out, sizes):
    """What `encode` (here or in jpeg_ops) returned, as a list of bytes, with one read of the device."""
    both = torch.cat([out.reshape(-1), sizes.view(torch.uint8)]).cpu()
    B, stride = out.shape
    n = both[B * stride:].view(torch.int32).tolist()
    flat = both.numpy()
    return [flat[b * stride:b * stride + n[b]].tobytes() for b in range(B)]


class PngWriter:
    """Files written behind the render loop.  `submit(images, paths)` enqueues the encode, then the device-to-host copies of the files
    and of their sizes into pinned buffers, records an event and returns; a worker thread waits for the event and writes the files.
    The submitting thread waits for nothing on the device; it blocks only while all `slots` pinned buffers (one image each) are in
    flight.  `close()` drains the queue, joins the workers and re-raises the first error one of them met (also on leaving a `with`
    block).  `threads` is a small constant: the workers wait for events and for the disk, they do not compute.  `files`: the number
    of files submitted so far."""

    def __init__(self, slots=32, threads=2):
        self.slots, self.threads = int(slots), int(threads)
        if self.slots < 1 or self.threads < 1:
            raise ValueError("PngWriter: slots and threads must be >= 1")
        self._pinned = None                     # [slots, stride] uint8, pinned
        self._free = list(range(self.slots))
        self._cond = threading.Condition()
        self._queue = queue.Queue()
        self._error = None
        self._workers = []
        self._closed = False
        self.files = 0

    def _start(self):
        if not self._workers:
            for k in range(self.threads):
                w = threading.Thread(target=self._work, name=f"{type(self).__name__}-{k}", daemon=True)
                w.start()
                self._workers.append(w)

    def _work(self):
        while True:
            item = self._queue.get()
            if item is None:
                return
            event, slot, sizes, index, path = item
            try:
                if self._error is None:
                    event.synchronize()
                    self._store(path, memoryview(self._pinned[slot].numpy())[:int(sizes[index])])
            except BaseException as e:          # noqa: BLE001  (kept for close())
                with self._cond:
                    if self._error is None:
                        self._error = e
            finally:
                with self._cond:
                    self._free.append(slot)
                    self._cond.notify_all()

    def _encode(self, x):
        """(buffer, sizes) of the batch x; jpeg_ops' writers put their own encoder behind the same ring."""
        return encode(x)

    def _store(self, path, data):
        with open(path, "wb") as fp:
            fp.write(data)

    def _take(self, n):
        with self._cond:
            while len(self._free) < n:
                self._cond.wait()
            taken, self._free = self._free[:n], self._free[n:]
        return taken

    def _drain(self):
        with self._cond:
            while len(self._free) < self.slots:
                self._cond.wait()

    def submit(self, images, paths):
        """images: [B,3,H,W] / [3,H,W] / a list of [3,H,W] device tensors; paths: one file name per image."""
        if self._closed:
            raise RuntimeError("PngWriter.submit: the writer is closed")
        x = _batch(images)
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        if len(paths) != x.shape[0]:
            raise RuntimeError(f"PngWriter.submit: {x.shape[0]} images but {len(paths)} paths")
        out, sizes = self._encode(x)
        B, stride = out.shape
        if self._pinned is None or self._pinned.shape[1] < stride:
            self._drain()                       # (a larger image than any before: the buffers are replaced once nothing is in flight)
            self._pinned = torch.empty(self.slots, stride, dtype=torch.uint8, pin_memory=True)
        self._start()
        for lo in range(0, B, self.slots):
            hi = min(B, lo + self.slots)
            taken = self._take(hi - lo)
            host_sizes = torch.empty(hi - lo, dtype=torch.int32, pin_memory=True)
            host_sizes.copy_(sizes[lo:hi], non_blocking=True)
            for k, slot in enumerate(taken):
                self._pinned[slot, :stride].copy_(out[lo + k], non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(x.device))
            for k, slot in enumerate(taken):
                self._queue.put((event, slot, host_sizes, k, paths[lo + k]))
            self.files += hi - lo

    def close(self):
        if not self._closed:
            self._closed = True
            for _ in self._workers:
                self._queue.put(None)
            for w in self._workers:
                w.join()
            self._workers = []
        error, self._error = self._error, None
        if error is not None:
            raise error

    def __enter__(self):
        return self

    def __exit__(self, etype, exc, tb):
        if etype is None:
            self.close()
        else:
            try:
                self.close()
            except BaseException:               # noqa: BLE001  (the block's own exception wins)
                pass
        return False
