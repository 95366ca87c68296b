"""tests/guard_bands.py on CPU tensors: the proof that the detector the GPU extent tests rely on does detect (no device needed,
and no device buffer is ever overrun on purpose to show it)."""
import pytest
import torch

import guard_bands as GB


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, (153, 64)), (torch.float16, (2, 13, 21, 192)), (torch.float32, (3, 640, 2)),
                                         (torch.uint8, (546, 8)), (torch.uint8, 1000)])
@pytest.mark.parametrize("band", [1, 256, 300, 256 * 64 * 2])
def test_carve_gives_the_claimed_layout(dtype, shape, band):
    p, h = GB.carve(shape, dtype, "cpu", band)
    item = torch.empty((), dtype=dtype).element_size()
    want_shape = (shape // item,) if isinstance(shape, int) else shape
    n = item
    for s in want_shape:
        n *= s
    assert tuple(p.shape) == want_shape and p.dtype == dtype and p.is_contiguous()
    assert h.band % 256 == 0 and h.band >= band and h.band >= 256
    assert h.nbytes == n and h.raw.dtype == torch.uint8 and h.raw.numel() == h.band + n + h.band
    off = p.data_ptr() - h.raw.data_ptr()
    assert off == h.band and off % 256 == 0 and p.data_ptr() % 16 == 0
    assert h.leading.numel() == h.band and h.trailing.numel() == h.band
    assert h.trailing.data_ptr() == p.data_ptr() + n                   # the trailing band starts at the first byte behind the payload
    assert bool((h.raw == 0xFF).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(p.float()).all()) and not GB.finite(p)   # the fill is a NaN in every float format used
    else:
        assert bool((p == 255).all())
    GB.check(h, "fresh")
    GB.check_untouched(h, "fresh")


def test_fill_writes_the_payload_only():
    v = torch.arange(153 * 64, dtype=torch.float32).reshape(153, 64).bfloat16()
    p, h = GB.carve((153, 64), torch.bfloat16, "cpu", 512)
    GB.fill(p, v)
    assert torch.equal(p, v) and GB.finite(p)
    GB.check(h, "after fill")
    with pytest.raises(AssertionError):
        GB.check_untouched(h, "after fill")             # (the payload is no longer 0xFF)
    with pytest.raises(AssertionError):
        GB.fill(p, v.float())                           # another dtype
    with pytest.raises(AssertionError):
        GB.fill(p, v[:100])                             # another size


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_check_fails_on_one_changed_byte_of_the_leading_band(where):
    p, h = GB.carve((7, 24), torch.float16, "cpu", 1000)
    i = {"first": 0, "last": h.band - 1, "middle": h.band // 2}[where]
    h.raw[i] = 0xFE                                      # one bit of one byte, through the handle's own tensor
    with pytest.raises(AssertionError) as e:
        GB.check(h, "out")
    msg = str(e.value)
    assert "out: 1 guard byte(s) changed (1 leading, 0 trailing)" in msg
    assert "first at payload offset %d, last at %d;" % (i - h.band, i - h.band) in msg


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_check_fails_on_one_changed_byte_of_the_trailing_band(where):
    p, h = GB.carve((7, 24), torch.float16, "cpu", 1000)
    j = {"first": 0, "last": h.band - 1, "middle": h.band // 2}[where]
    h.raw[h.band + h.nbytes + j] = 0                     # the byte right behind the payload for "first"
    with pytest.raises(AssertionError) as e:
        GB.check(h, "out")
    msg = str(e.value)
    assert "out: 1 guard byte(s) changed (0 leading, 1 trailing)" in msg
    assert "first at payload offset %d, last at %d;" % (h.nbytes + j, h.nbytes + j) in msg


def test_check_reports_count_and_span_over_both_bands():
    p, h = GB.carve(4096, torch.uint8, "cpu", 256)
    h.raw[h.band - 3:h.band] = 1                         # 3 bytes in front of the payload
    h.raw[h.band + 4096:h.band + 4096 + 16] = 0          # 16 bytes behind it
    with pytest.raises(AssertionError) as e:
        GB.check(h, "ws")
    msg = str(e.value)
    assert "19 guard byte(s) changed (3 leading, 16 trailing)" in msg and "first at payload offset -3, last at 4111;" in msg
    # writing the payload itself — all of it, up to its last byte — is what a kernel is supposed to do
    q, g = GB.carve(4096, torch.uint8, "cpu", 256)
    q.zero_()
    GB.check(g, "payload")
