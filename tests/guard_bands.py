"""Guard bands around the buffers a kernel is handed (a plain helper module, no fixtures).

A carved buffer is ONE uint8 allocation, [leading band | payload | trailing band], filled with 0xFF throughout.  0xFFFF is a NaN
in bf16 and fp16, 0xFFFFFFFF one in fp32, 0xFF is 255 in uint8 — so the same fill is the guard pattern of the bands, the
"never written" marker of an output payload and the "must never be read" poison around an input payload.  A store that
leaves the tensor it was given lands in memory the test owns: it is detected afterwards, it never faults.

    y, hy = carve((M, N), torch.bfloat16, "cuda", band)     # an output: left at 0xFF
    x, hx = carve(tuple(x0.shape), x0.dtype, "cuda", band)  # an input ...
    fill(x, x0)                                             # ... with real data inside poison
    launch(x.data_ptr(), y.data_ptr(), ...)
    torch.cuda.synchronize()
    check(hx, "x"); check(hy, "y")                          # both bands of each still 0xFF
    assert finite(y)                                        # every element written, no poison read into it
"""
import math

import torch

FILL = 0xFF
ALIGN = 256


def round_band(nbytes):
    """a band of at least nbytes, in whole 256-byte units (never empty)"""
    return max(ALIGN, (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN)


class Handle:
    """the whole allocation of one carved buffer: raw uint8 [band + nbytes + band]; the payload is raw[band : band + nbytes]"""

    def __init__(self, raw, band, nbytes):
        self.raw, self.band, self.nbytes = raw, band, nbytes

    @property
    def leading(self):
        return self.raw[:self.band]

    @property
    def trailing(self):
        return self.raw[self.band + self.nbytes:]


def carve(nbytes_or_shape, dtype, device, band):
    """-> (payload_view, handle).  nbytes_or_shape: a shape, or a byte count (the payload is then 1-d, nbytes / itemsize long).
    The payload starts at offset `band` (rounded up to a multiple of 256) of a fresh allocation, is contiguous and has the
    requested dtype and shape; the trailing band starts at the first byte behind it."""
    item = torch.empty((), dtype=dtype).element_size()
    if isinstance(nbytes_or_shape, int):
        assert nbytes_or_shape % item == 0, "byte count is no multiple of the element size"
        shape = (nbytes_or_shape // item,)
    else:
        shape = tuple(int(s) for s in nbytes_or_shape)
    nbytes = math.prod(shape) * item
    assert nbytes > 0
    band = round_band(band)
    raw = torch.full((band + nbytes + band,), FILL, dtype=torch.uint8, device=device)
    payload = raw[band:band + nbytes].view(dtype).view(shape)
    assert payload.is_contiguous() and payload.data_ptr() == raw.data_ptr() + band
    assert payload.data_ptr() % 16 == 0, "the allocator returned a block that is not 16-byte aligned"
    return payload, Handle(raw, band, nbytes)


def fill(payload_view, values):
    """copy real data (same dtype and element count, any device) into a payload"""
    assert values.dtype == payload_view.dtype and values.numel() == payload_view.numel(), (values.dtype, tuple(values.shape))
    payload_view.copy_(values.reshape(payload_view.shape))
    return payload_view


def _changed(t):
    return torch.nonzero(t != FILL).flatten()


def check(handle, what):
    """both bands are still entirely 0xFF (call after the device has finished); otherwise an AssertionError that says how
    many bytes changed and the first / last changed offset relative to the payload's first byte (negative: leading band;
    >= payload bytes: trailing band)"""
    lead, trail = _changed(handle.leading), _changed(handle.trailing)
    n = int(lead.numel() + trail.numel())
    if n == 0:
        return
    offs = torch.cat([lead.cpu() - handle.band, trail.cpu() + handle.nbytes])
    raise AssertionError("%s: %d guard byte(s) changed (%d leading, %d trailing); first at payload offset %d, last at %d; "
                         "payload = %d bytes, band = %d bytes" % (what, n, lead.numel(), trail.numel(), int(offs.min()),
                                                                  int(offs.max()), handle.nbytes, handle.band))


def check_untouched(handle, what):
    """bands AND payload are still 0xFF: a call that was refused wrote nothing at all"""
    check(handle, what)
    pay = _changed(handle.raw[handle.band:handle.band + handle.nbytes])
    assert pay.numel() == 0, "%s: %d payload byte(s) written by a call that was refused (first at %d)" % (
        what, pay.numel(), int(pay.min()))


def finite(payload_view):
    """no element of a floating-point payload is NaN / inf: everything was written and no poison was read into it"""
    return bool(torch.isfinite(payload_view.float() if payload_view.dtype != torch.float64 else payload_view).all())
