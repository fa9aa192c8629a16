"""The decoders' pinned staging buffer (png_decode.stage, jpeg_decode.stage: decode_stage.stage) holds, over every defined section, the
bytes decode_stage.fill writes into a plain numpy array of the same size -- what tests/test_decode_stage_host.py and the emulator tests
check without a device.  No kernel runs; the padding between the sections is written by neither and is not compared."""
import numpy as np
import pytest

import decode_stage_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["png", "jpeg"])
def test_the_pinned_buffer_equals_the_plain_fill(kind):
    from gaussianprediction_amd import jpeg_decode as JD, png_decode as PD
    *args, plans = SC.png_set() if kind == "png" else SC.jpeg_set()
    staged = (PD if kind == "png" else JD).stage(*args)
    host = SC.filled(plans)
    assert staged.buffer.is_pinned() and staged.buffer.dtype.itemsize == 1 and len(staged.buffer) == len(host)
    pinned, compared = staged.buffer.numpy(), 0
    assert len(staged.plans) == len(plans) == 2
    for got, want in zip(staged.plans, plans):
        assert SC.spans(got) == SC.spans(want) and got.idx == want.idx
        assert SC.sections(pinned, got) == SC.sections(host, want)
        compared += sum(n for _, n in SC.spans(want))
    assert compared > 1000 and (kind == "png") == (not any(len(pl.tables) for pl in plans))
