"""The peak search (bbx_find_peaks) behind the catalogue and the transient candidates, and the windowed centroids of the
peaks (bbx_win_centroid)."""
import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, fetch, ptr as _p


def find_transients(ctx, Scorr, nsigma=None, max_out=100000):
    """connected regions of |Scorr| >= T-NSIGMA -> sorted list of (y, x, Scorr peak)"""
    ys, xs, val = find_peaks_arrays(ctx, Scorr, nsigma, max_out)
    return list(zip(ys.tolist(), xs.tolist(), val.tolist()))


def find_peaks_enqueue(ctx, Scorr, nsigma=None, max_out=100000):
    """queue bbx_find_peaks -> the device tensors find_peaks_collect reads (host work in between overlaps the search)"""
    nsigma = settings.transient_nsigma if nsigma is None else nsigma
    ny, nx = Scorr.shape
    dev = ctx.device
    yx = torch.empty((max_out, 2), dtype=torch.int32, device=dev)
    val = torch.empty(max_out, dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.bbx_find_peaks(ctx.h, ny, nx, _p(Scorr), float(nsigma), max_out, _p(yx), _p(val), _p(cnt), ctx.stream()),
          'bbx_find_peaks', ctx.h)
    return yx, val, cnt, max_out


def find_peaks_collect(ctx, pending):
    """-> arrays (y int32, x int32, peak float32), sorted by (y, x)"""
    yx, val, cnt, max_out = pending
    if max_out * 12 <= (2 << 20):
        # the count and the whole list (1.2 MB at the default capacity) in ONE copy back and one host wait: asking for the
        # count first costs a second round trip -- with the stream's other work in front of it each time
        c, yx, val = fetch(ctx, cnt, yx, val, check_device_errors=True)
        n = min(int(c[0]), max_out)
        yx, val = yx[:n], val[:n]
    else:
        n = min(int(fetch(ctx, cnt, check_device_errors=True)[0]), max_out)
        yx, val = fetch(ctx, yx[:n], val[:n])
    order = np.lexsort((yx[:, 1], yx[:, 0])) if n else np.zeros(0, int)
    return yx[order, 0], yx[order, 1], val[order]


def find_peaks_arrays(ctx, Scorr, nsigma=None, max_out=100000):
    """the same as arrays (y int32, x int32, peak float32), sorted by (y, x): no per-source Python work"""
    return find_peaks_collect(ctx, find_peaks_enqueue(ctx, Scorr, nsigma, max_out))


def window_sigma(stamps):
    """window sigma of the centroid from unit-sum PSF stamps [..., S, S] (device tensor or numpy): sigma_w =
    sqrt(1 / (4 pi sum P^2)), the sigma of the Gaussian with the stamp's effective area.  Stays where the stamps are"""
    if torch.is_tensor(stamps):
        return (1.0 / (4.0 * np.pi * (stamps * stamps).sum(dim=(-2, -1)))).sqrt().to(torch.float32).contiguous()
    stamps = np.asarray(stamps, np.float64)
    return np.sqrt(1.0 / (4.0 * np.pi * (stamps * stamps).sum(axis=(-2, -1))))


def win_centroid(ctx, img, d_ys, d_xs, d_sigw, size, nsy, nsx, radius=None, niter=None):
    """bbx_win_centroid: windowed centroids of the sources at the int32 device peaks (d_ys, d_xs) of the frame [img] ->
    device float32 [n, 2] = (dy, dx) relative to the integer peak, NaN where there is none.  No host wait"""
    radius = settings.centroid_radius if radius is None else radius
    niter = settings.centroid_niter if niter is None else niter
    _args.frame(img)
    n = int(d_ys.numel())
    off = torch.empty((n, 2), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_win_centroid(ctx.h, img.shape[0], img.shape[1], _p(img), n, _p(d_ys), _p(d_xs), _p(d_sigw), int(size), int(nsy), int(nsx),
                               int(radius), int(niter), _p(off), ctx.stream()), 'bbx_win_centroid', ctx.h)
    return off
