"""PNG encoding on the device (include/gp_png.h, png_ops) with the decoders as the oracle: for every case of tests/png_cases.py Pillow
opens the file to exactly the quantised input; the test's own chunk walk finds IHDR, the IDAT chunks and IEND with every CRC-32
equal to zlib's, zlib inflates the joined IDAT data (which checks the Adler-32) to H rows of 1 + 3 W bytes with legal filter types;
the file stays inside bound(H, W) and the slot behind it untouched; two calls are bit-identical and a batched row is the single
call's file.  Sizes: a constant image under 1/20 of its raw bytes; the disc and the ramp within 1.10 of zlib's own run-length
strategy over the very same filtered bytes cut at the same bands (measured on the MI355X: 0.9999 and 0.9992)."""
import numpy as np
import pytest
import torch

import png_cases as P

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def PNG():
    from gaussianprediction_amd import png_ops
    return png_ops


def _cases():
    from gaussianprediction_amd.png_ops import BAND_BYTES
    return {name: (imgs, fnone) for name, imgs, fnone in P.cases(BAND_BYTES)}


CASES = _cases()


def _encode(PNG, imgs, fnone):
    """(files as bytes, the whole slots as numpy, sizes) of one call into canary-filled slots."""
    x = torch.from_numpy(imgs).cuda()
    B, _, H, W = x.shape
    stride = PNG.bound(H, W)
    out = torch.full((B, stride + 64), CANARY, dtype=torch.uint8, device="cuda")
    buf, sizes = PNG.encode(x, filter_none=fnone, out=out)
    assert buf.data_ptr() == out.data_ptr() and sizes.dtype == torch.int32 and sizes.shape == (B,)
    slots, n = out.cpu().numpy(), sizes.cpu().tolist()
    return [slots[b, :n[b]].tobytes() for b in range(B)], slots, n


@pytest.mark.parametrize("name", list(CASES))
def test_files_decode_to_the_quantised_input(PNG, name):
    imgs, fnone = CASES[name]
    B, _, H, W = imgs.shape
    files, slots, sizes = _encode(PNG, imgs, fnone)
    again, slots2, sizes2 = _encode(PNG, imgs, fnone)
    assert sizes == sizes2 and np.array_equal(slots, slots2)                     # two calls: the same bits
    for b in range(B):
        want = P.quantise(imgs[b])
        assert 0 < sizes[b] <= PNG.bound(H, W)
        assert (slots[b, sizes[b]:] == CANARY).all()                             # nothing at or beyond the file's length
        stream, payload, nidat = P.check_file(files[b], want, fnone)
        assert nidat == -(-len(stream) // PNG.BAND_BYTES)                        # one IDAT chunk per band
        if not fnone:
            types = np.frombuffer(stream, dtype=np.uint8).reshape(H, 3 * W + 1)[:, 0]
            assert np.array_equal(types, P.best_filters(want))                   # the smallest sum of |residual|, ties to the lower type
        ratio = payload / P.rle_reference_bytes(stream, PNG.BAND_BYTES)
        print(f"{name}[{b}]: {H}x{W} file {sizes[b]} B, IDAT payload {payload} B, {ratio:.4f} of zlib's Z_RLE over the same bands")
        if name.startswith(("disc", "ramp-300")):
            assert ratio <= 1.10
        if name.startswith("constant"):
            assert sizes[b] < H * 3 * W / 20
        if B > 1:                                                                # row b of the batch is the B = 1 call on image b
            alone, _, _ = _encode(PNG, imgs[b:b + 1], fnone)
            assert alone[0] == files[b]


def test_uint8_input_float_input_and_the_read_forms_agree(PNG):
    """The 8-bit render that gp_image_metrics hands out (`quantized`) encodes to the file of the float image it came from; a list of
    [3, H, W] tensors is the batch; encode_to_bytes is encode read once."""
    from gaussianprediction_amd import metrics as M
    x = torch.from_numpy(np.stack([P.disc(163, 178, 7), P.edge_floats((3, 163, 178), 8)])).cuda()
    gt = torch.from_numpy(P.disc(163, 178, 9)[None]).cuda().expand(2, -1, -1, -1).contiguous()
    q = M.image_metrics(torch.nan_to_num(x, nan=0.0, posinf=2.0), gt, quantize8=True, quantized=True).quantized
    assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), P.quantise(x.cpu().numpy()))
    from_float = PNG.encode_to_bytes(x)
    assert PNG.encode_to_bytes(q) == from_float == PNG.encode_to_bytes([x[0], x[1]])
    assert PNG.encode_to_bytes(x[1]) == from_float[1:]
    assert PNG.encode_to_bytes(x.double()) == PNG.encode_to_bytes(x) and PNG.encode_to_bytes(x, filter_none=True) != from_float
    with pytest.raises(RuntimeError, match="out must be"):
        PNG.encode(x, out=torch.empty(2, PNG.bound(163, 178) - 8, dtype=torch.uint8, device="cuda"))


def test_writer_writes_behind_the_stream_and_reports_a_worker_error(PNG, tmp_path):
    import threading
    from PIL import Image
    x = torch.from_numpy(np.stack([P.disc(37, 45, s) for s in range(5)])).cuda()
    want = P.quantise(x.cpu().numpy()).transpose(0, 2, 3, 1)
    with PNG.PngWriter(slots=2, threads=2) as w:                                 # more images than buffers: the submit waits for free ones
        w.submit(x, [tmp_path / f"{i:05d}.png" for i in range(5)])
        w.submit(x[0], tmp_path / "single.png")
        big = torch.from_numpy(P.disc(90, 120, 1)).cuda()                        # a larger image: the pinned buffers are replaced
        w.submit([big], [str(tmp_path / "big.png")])
    assert w.files == 7
    for i in range(5):
        assert np.array_equal(np.array(Image.open(tmp_path / f"{i:05d}.png")), want[i])
    assert np.array_equal(np.array(Image.open(tmp_path / "single.png")), want[0])
    assert np.array_equal(np.array(Image.open(tmp_path / "big.png")), P.quantise(big.cpu().numpy()).transpose(1, 2, 0))
    bad = PNG.PngWriter()
    bad.submit(x[:2], [tmp_path / "missing" / "a.png", tmp_path / "missing" / "b.png"])
    with pytest.raises(FileNotFoundError):
        bad.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("PngWriter")]
    bad.close()                                                                  # (a second close is quiet)
