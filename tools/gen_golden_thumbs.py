#!/usr/bin/env python3
"""Golden vectors of the thumbnail display planes: tests/golden/thumbs.npz.

Runs in the build container under the Python that has astropy (the one oracle/_refload.py is written for);
never on the GPU machine.  For every stamp it stores what the reference's OWN functions make of
np.flipud(stamp), exactly as save_thumbs_row (blackbox.py:2786-2808) chains them:

    vmin, vmax = zscale().get_limits(data)        # astropy ZScaleInterval, as imported by the reference
    data = scale_data(data, vmin, vmax)           # blackbox.py:2814-2826

The inputs travel with the results (nothing depends on a random stream being reproducible): int16 counts
and one float32 scale per stamp, stamp = float32(counts) * scale, count -32768 = NaN.  No constant stamp:
the reference divides by zero there.

    python tools/gen_golden_thumbs.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
SIZE = 100
NAN_COUNT = -32768


def moffat(yy, xx, y0, x0, fwhm, beta=2.5):
    alpha = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / beta) - 1.0))
    return (1.0 + ((yy - y0) ** 2 + (xx - x0) ** 2) / alpha ** 2) ** (-beta)


def decode(counts, scale):
    """the float32 stamps of the stored counts (the tests use the same two lines)"""
    stamps = counts.astype(np.float32) * scale.astype(np.float32)[:, None, None]
    stamps[counts == NAN_COUNT] = np.nan
    return stamps


def build_stamps():
    rng = np.random.default_rng(20240607)
    yy, xx = np.mgrid[0:SIZE, 0:SIZE].astype(np.float64)
    stamps, kinds = [], []

    def sky(sigma, sources):
        img = rng.normal(0.0, sigma, (SIZE, SIZE))
        for amp, y0, x0, fwhm in sources:
            img += amp * sigma * moffat(yy, xx, y0, x0, fwhm)
        return img

    # sky noise (counts, sigma 4-12) with one to four Moffat sources at several contrasts
    cases = [(4.0, [(8, 50, 50, 3.0)]),
             (6.0, [(40, 50, 50, 3.5)]),
             (8.0, [(400, 50, 50, 4.0)]),
             (5.0, [(2500, 50, 50, 3.0)]),
             (7.0, [(15, 50, 50, 3.0), (150, 20, 71, 3.0)]),
             (9.0, [(60, 50, 50, 4.5), (6, 80, 12, 4.5)]),
             (12.0, [(25, 50, 50, 2.5), (900, 33, 30, 2.5), (12, 70, 85, 2.5)]),
             (6.0, [(10, 50, 50, 5.0), (80, 10, 10, 5.0), (300, 90, 40, 5.0), (30, 44, 93, 5.0)]),
             (10.0, [(-30, 50, 50, 3.0), (45, 56, 50, 3.0)])]          # a D-like dipole
    for sigma, sources in cases:
        stamps.append((sky(sigma, sources), 1.0)); kinds.append(0)
    # Scorr-like: unit noise, a +-6 ... +-100 peak; stored in steps of 1/256
    for peak in (6.0, -6.0, 14.0, -35.0, 100.0):
        img = rng.normal(0.0, 1.0, (SIZE, SIZE)) + peak * moffat(yy, xx, 50, 50, 4.0)
        stamps.append((img, 1.0 / 256)); kinds.append(1)
    # a zero-padded band of 1-60 columns or rows (a candidate near the frame edge)
    for width, side in ((1, 'l'), (7, 'r'), (25, 't'), (40, 'b'), (60, 'l'), (60, 't')):
        img = sky(8.0, [(50, 50, 50, 3.5)]) + 3.0
        if side == 'l':
            img[:, :width] = 0
        elif side == 'r':
            img[:, SIZE - width:] = 0
        elif side == 't':
            img[:width] = 0
        else:
            img[SIZE - width:] = 0
        stamps.append((img, 1.0)); kinds.append(2)
    # a few dozen NaNs: scattered, a clump, a row segment
    for n_nan, how in ((24, 's'), (36, 'c'), (60, 'r'), (48, 's')):
        img = sky(6.0, [(120, 50, 50, 3.0)])
        if how == 's':
            idx = rng.choice(SIZE * SIZE, n_nan, replace=False)
            img.reshape(-1)[idx] = np.nan
        elif how == 'c':
            img[30:36, 60:66] = np.nan
        else:
            img[47, 20:80] = np.nan
        stamps.append((img, 1.0)); kinds.append(3)

    counts = np.zeros((len(stamps), SIZE, SIZE), np.int16)
    scale = np.zeros(len(stamps), np.float32)
    for k, (img, sc) in enumerate(stamps):
        q = np.rint(np.where(np.isfinite(img), img, 0) / sc)
        assert np.abs(q).max() < 32767
        counts[k] = q.astype(np.int16)
        counts[k][~np.isfinite(img)] = NAN_COUNT
        scale[k] = sc
    return counts, scale, np.asarray(kinds, np.int8)


def main(out):
    from oracle import _refload
    bb, _ = _refload.load()
    counts, scale, kinds = build_stamps()
    stamps = decode(counts, scale)
    limits = np.zeros((len(stamps), 2), np.float64)
    planes = np.zeros(stamps.shape, np.uint8)
    for k, stamp in enumerate(stamps):
        assert np.nanmax(stamp) > np.nanmin(stamp)
        data = np.flipud(stamp.copy())
        vmin, vmax = bb.zscale().get_limits(data)
        with np.errstate(invalid='ignore'):
            planes[k] = bb.scale_data(data, vmin, vmax)
        limits[k] = vmin, vmax
    np.savez_compressed(out, counts=counts, scale=scale, kinds=kinds, limits=limits, planes=planes,
                        nan_count=np.int16(NAN_COUNT))
    print('{}: {} stamps, {} bytes'.format(out, len(stamps), os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, '..', 'tests', 'golden', 'thumbs.npz'))
