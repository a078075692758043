"""Flux ratio and dx, dy from the stars matched between the new frame and the reference (bbx_match_mutual, bbx_match_stats):
the reference's catalogue, the match, the table and the scalars and header keys made of it."""
import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, fetch, push, ptr as _p
from .peaks import find_peaks_arrays, win_centroid, window_sigma
from .psfphot import psf_optflux, psf_optflux_centroid, source_psfs, subimage_psfs
from .zoom import MiniImage

# ---- flux ratio and dx, dy from matched stars ---------------------------------------------
# buildref.py:2782-3014 (get_fratio, "simplified version of zogy.get_fratio_dxdy") shows the computation; [EXT]
# get_fratio_dxdy, get_matches, get_mean_fratio are not in the reference tree (conventions: include/bbx.h).
MATCH_COLS = ('n_qualifying', 'n_fr', 'med_fr', 'mean_fr', 'std_fr', 'wmean_fr', 'werr_fr', 'n_dx', 'med_dx', 'mean_dx', 'std_dx',
              'n_dy', 'med_dy', 'mean_dy', 'std_dy', 'stride')
_MC = {k: i for i, k in enumerate(MATCH_COLS)}


def match_mutual(ctx, a, b, dist_max):
    """bbx_match_mutual of two lists (d_ys, d_xs, d_off), each sorted by (y, x) -> device int32 [n_a]: index into b, or -1"""
    n_a, n_b = int(a[0].numel()), int(b[0].numel())
    d_match = torch.empty(n_a, dtype=torch.int32, device=ctx.device)
    d_best = torch.empty(n_b, dtype=torch.int32, device=ctx.device)
    check(lib.bbx_match_mutual(ctx.h, n_a, _p(a[0]), _p(a[1]), _p(a[2]), n_b, _p(b[0]), _p(b[1]), _p(b[2]), float(dist_max),
                               _p(d_best), _p(d_match), ctx.stream()), 'bbx_match_mutual', ctx.h)
    return d_match


def empty_match_table(nsub):
    """the table of a frame without a pair: counts 0, stride 1, NaN elsewhere (what bbx_match_stats writes for empty segments)"""
    t = np.full((nsub + 1, 16), np.nan)
    t[:, [_MC['n_qualifying'], _MC['n_fr'], _MC['n_dx'], _MC['n_dy']]] = 0.0
    t[:, _MC['stride']] = 1.0
    return t


def match_stats(ctx, a, b, d_match, size, nsy, nsx, snr_min):
    """bbx_match_stats of the lists a, b = (d_ys, d_xs, d_off, d_flux, d_err) matched by d_match -> device float64
    [nsy * nsx + 1, 16] (MATCH_COLS; last row: the whole frame)"""
    n_a, n_b = int(a[0].numel()), int(b[0].numel())
    if not n_a:
        return torch.from_numpy(empty_match_table(nsy * nsx)).to(ctx.device)
    out = torch.empty((nsy * nsx + 1, 16), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_match_stats(ctx.h, n_a, *[_p(t) for t in a], n_b, *[_p(t) for t in b], _p(d_match), int(size), int(nsy), int(nsx),
                              float(snr_min), _p(out), ctx.stream()), 'bbx_match_stats', ctx.h)
    return out


_MATCH_HDR = (('Z-DX', 'med_dx', '[pix] dx median offset full image'), ('Z-DY', 'med_dy', '[pix] dy median offset full image'),
              ('Z-DXSTD', 'std_dx', '[pix] dx sigma (STD) offset full image'), ('Z-DYSTD', 'std_dy', '[pix] dy sigma (STD) offset full image'),
              ('Z-FNR', 'med_fr', 'median flux ratio (Fnew/Fref) full image'), ('Z-FNRSTD', 'std_fr', 'sigma (STD) flux ratio (Fnew/Fref) full image'),
              ('Z-FNRERR', 'werr_fr', 'weighted error flux ratio (Fnew/Fref) full image'))


def match_scalars(table, fratio, dx, dy, nmin):
    """the table of bbx_match_stats [nsub + 1, 16] (host) -> dict(success, fratio_sub, dx_sub, dy_sub [nsub], header).
    A tile with n_fr >= nmin takes its clipped median ratio; with n_dx >= nmin sqrt(mean_dx^2 + std_dx^2) (the scatter about
    zero that enters V(S)), likewise dy; a tile below nmin takes the full-frame row's value.  A full-frame row with any of the
    three counts below nmin: success False, every tile takes the caller's fratio, dx, dy (one number or one per tile).
    header: Z-DX, Z-DY, Z-DXSTD, Z-DYSTD, Z-FNR, Z-FNRSTD, Z-FNRERR from the full-frame row (set_qc.py:370-375, 425); without
    success the caller's medians for Z-DX, Z-DY, Z-FNR and the string 'None', set_qc's default, for the other four.  Pure numpy"""
    table = np.asarray(table, np.float64)
    nsub = table.shape[0] - 1
    full = table[nsub]
    caller = [np.broadcast_to(np.asarray(v, np.float64), (nsub,)).copy() for v in (fratio, dx, dy)]
    success = bool(full[_MC['n_fr']] >= nmin and full[_MC['n_dx']] >= nmin and full[_MC['n_dy']] >= nmin)
    if not success:
        fall = {'Z-DX': float(np.median(dx)), 'Z-DY': float(np.median(dy)), 'Z-FNR': float(np.median(fratio))}
        hdr = {key: (fall.get(key, 'None'), comment) for key, _, comment in _MATCH_HDR}
        return dict(success=False, fratio_sub=caller[0], dx_sub=caller[1], dy_sub=caller[2], header=hdr)
    hdr = {}

    def scatter(rows, q):
        return np.sqrt(rows[..., _MC['mean_' + q]] ** 2 + rows[..., _MC['std_' + q]] ** 2)
    t = table[:nsub]
    out = [np.where(t[:, _MC['n_fr']] >= nmin, t[:, _MC['med_fr']], full[_MC['med_fr']])]
    for q in ('dx', 'dy'):
        out.append(np.where(t[:, _MC['n_' + q]] >= nmin, scatter(t, q), scatter(full, q)))
    for key, col, comment in _MATCH_HDR:
        hdr[key] = (float(full[_MC[col]]), comment)
    return dict(success=True, fratio_sub=out[0], dx_sub=out[1], dy_sub=out[2], header=hdr)


class RefCatalog:
    """The reference's half of the star match, made once for a reference that stays the same over many frames: the peaks of
    the reference as the subtraction sees it (background-subtracted, on the new frame's grid) above cat_nsigma x the median
    of its sigma mini image, those on masked pixels dropped, with their PSF-weighted fluxes (psf_optflux) and windowed
    centroids (bbx_win_centroid), all on the device in (y, x) order.  Holds what it was made of (the reference and its sigma
    map: a frame or a MiniImage); optimal_subtraction uses it for calls with that very reference, sigma map and geometry.
    Made on ctx's current stream with host waits (once per run): a caller that hands the object to other streams waits for
    that stream first."""
    builds = 0                                   # catalogues made so far (tests: once per run, not per frame)

    def __init__(self, ctx, ref, sig_ref, ref_mask, psf_ref, size, border, cat_nsigma=5.0, sigma_median=None, sub_psfs=None,
                 max_sources=200000, phot_centroid=False):
        ny, nx = _args.frame(ref)
        self.phot_centroid = bool(phot_centroid)
        size, border = int(size), int(border)
        nsy, nsx = ny // size, nx // size
        if sigma_median is None:
            if isinstance(sig_ref, MiniImage):
                raise ValueError('sigma_median (median of the sigma mini image) is needed with a MiniImage')
            sigma_median = float(np.median(fetch(ctx, sig_ref)))
        self.ref, self.sig_ref, self.geom = ref, sig_ref, (ny, nx, size, border)
        sub_pr = sub_psfs if sub_psfs is not None else subimage_psfs(ctx, psf_ref, nsy, nsx, size)
        thr = float(cat_nsigma) * float(sigma_median)
        if np.isfinite(thr) and thr > 0:
            ys, xs, pk = find_peaks_arrays(ctx, ref, thr, max_out=max_sources)
        else:
            ys = xs = np.zeros(0, np.int32); pk = np.zeros(0, np.float32)
        keep = pk > 0
        if ref_mask is not None and ys.size:
            d_ys, d_xs = push(ctx, ys.astype(np.int64), xs.astype(np.int64))
            keep &= fetch(ctx, ref_mask[d_ys, d_xs]) == 0
        ys, xs = ys[keep], xs[keep]
        self.n = int(ys.size)
        dev = ctx.device
        if self.n and self.phot_centroid:
            # the centroids first: the photometry places the PSF on them, as the new frame's does (both sides of a pair alike)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_pr), size, nsy, nsx)
            self.flux, self.err, _ = psf_optflux_centroid(ctx, ref, sig_ref, psf_ref, sub_pr, ys, xs, self.off, ref_mask, nsx, size,
                                                             d_peaks=(self.ys, self.xs))
        elif self.n:
            stamps = source_psfs(ctx, psf_ref, sub_pr, ys, xs, nsx, size)
            self.flux, self.err = psf_optflux(ctx, ref, sig_ref, stamps, ys, xs, v_is_sigma=True)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_pr), size, nsy, nsx)
        else:
            self.ys = self.xs = torch.empty(0, dtype=torch.int32, device=dev)
            self.flux = self.err = torch.empty(0, dtype=torch.float32, device=dev)
            self.off = torch.empty((0, 2), dtype=torch.float32, device=dev)
        RefCatalog.builds += 1

    def lists(self):
        return self.ys, self.xs, self.off, self.flux, self.err

    def matches(self, ref, sig_ref, size, border, phot_centroid=False):
        """made of these very tensors, for this geometry, with its PSFs placed the same way (phot_centroid)?"""
        return (ref is self.ref or (ref.data_ptr() == self.ref.data_ptr() and ref.shape == self.ref.shape)) and sig_ref is self.sig_ref \
            and (ref.shape[0], ref.shape[1], int(size), int(border)) == self.geom and bool(phot_centroid) == self.phot_centroid


def match_enqueue(ctx, work, ys, xs, d_mk, f, e, sub_pn, rc, size, nsy, nsx, dist_max=None, snr_min=None, peaks_off=None):
    """queue the new frame's half of the star match behind its photometry: centroids of the peaks (ys, xs: host, sorted by
    (y, x)) of the background-subtracted frame [work], the mutual match against the RefCatalog [rc] and the table.  Peaks
    on masked pixels (d_mk != 0) are taken out on the device: NaN offset (matches nothing) and flux 0.
    peaks_off: (d_y32, d_x32, off) where the caller has the peaks on the device as int32 and their centroids already (the
    source shapes start from the same ones); they are not changed.
    -> device (table float64 [nsub + 1, 16], number of pairs int64 [1]); no host wait"""
    dist_max = settings.match_dist_pix if dist_max is None else dist_max
    snr_min = settings.match_snr_min if snr_min is None else snr_min
    if peaks_off is not None:
        d_y32, d_x32, off = peaks_off
    else:
        d_y32, d_x32 = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
        off = win_centroid(ctx, work, d_y32, d_x32, window_sigma(sub_pn), size, nsy, nsx)
    bad = d_mk != 0
    off = torch.where(bad[:, None], torch.full_like(off, float('nan')), off).contiguous()
    f_m = torch.where(bad, torch.zeros_like(f), f).contiguous()
    a = (d_y32, d_x32, off, f_m, e)
    d_match = match_mutual(ctx, a[:3], rc.lists()[:3], dist_max)
    d_tab = match_stats(ctx, a, rc.lists(), d_match, size, nsy, nsx, snr_min)
    return d_tab, (d_match >= 0).sum().reshape(1)
