"""The two comparisons of the level-3 FDA tests (a plain helper module, no fixtures), and their synthetic frames.

A: device_aug.fda_u8 against the host FFT (augmentations.fourier_domain_adaptation).  B: the device against
device_aug.fda_u8.  Both bands are conditions on f = device_aug.fda_f64 of the same inputs; the cap on the share of
bytes inside the band is asserted BEFORE the bytes are compared, so an input that sits on the knife edges fails loudly."""
import numpy as np

BAND_A, CAP_A = 1e-3, 0.005


def smooth_noise(seed, h, w, mean):
    """a smooth field plus noise around `mean`, uint8 [h, w, 3]"""
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = g.uniform(0, 6.28, (3, 2))
    f = np.stack([mean + 40.0 * np.sin(x / (7.0 + 3 * c) + ph[c, 0]) * np.cos(y / (11.0 - 2 * c) + ph[c, 1]) for c in range(3)], -1)
    return np.clip(np.rint(f + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8)


def comparison_a(got, host, f, what):
    """got: fda_u8 (or what is pinned to it); host: the FFT form; f: fda_f64 of the same inputs"""
    assert got.shape == host.shape == f.shape and got.dtype == host.dtype == np.uint8, what
    band = np.abs(f - np.rint(f)) < BAND_A
    share = float(band.mean())
    assert share <= CAP_A, ("%s: %.3f %% of the bytes within %g of an integer (cap %.1f %%)"
                            % (what, 100 * share, BAND_A, 100 * CAP_A))
    d = got.astype(np.int32) - host.astype(np.int32)
    diff = d != 0
    print("%s: %d of %d bytes differ, %.3f %% in the band" % (what, int(diff.sum()), d.size, 100 * share))
    assert int(np.abs(d).max(initial=0)) <= 1, "%s: a byte differs by %d" % (what, int(np.abs(d).max()))
    assert not (diff & ~band).any(), "%s: %d differing bytes outside the band" % (what, int((diff & ~band).sum()))


BAND_B, CAP_B = 1e-6, 1e-4


def band_b(f, what):
    band = np.abs(f - np.rint(f)) < BAND_B
    share = float(band.mean())
    assert share <= CAP_B, "%s: %.2e of the bytes within %g of an integer (cap %g)" % (what, share, BAND_B, CAP_B)
    return band


def comparison_b(got, want, band, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d bytes differ, %d in the band" % (what, int((d != 0).sum()), d.size, int(band.sum())))
    assert int(d.max(initial=0)) <= 1, "%s: a byte differs by %d" % (what, int(d.max()))
    assert not ((d != 0) & ~band).any(), "%s: %d differing bytes outside the band" % (what, int(((d != 0) & ~band).sum()))
