"""The PSF model of a frame from its own stars (bbx_psfbuild.hip): selection, vignettes, fit, chi2 rounds and
the PSF-* header keys."""
import logging

import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, fetch, push, ptr as _p, BBXError as _lib_BBXError
from .peaks import find_peaks_arrays, win_centroid
from .psfphot import _source_sigma, psf_poly_terms
from .shapes import _SC, shape_stats, src_shapes

# ---- PSF model from the frame's own stars ---------------------------------------------------
# `_psf.fits` and the header keys PSF-P PSF-NOBJ PSF-CHI2 PSF-FWHM PSF-SEE PSF-SIZE PSF-CFGS PSF-SAMP PSF-PLDG PSF-FIX
# (blackbox.py:3085-3110, set_qc.py:293-296, 408-409).  [EXT] zogy runs PSFEx; here: the rules of include/bbx.h
# (bbx_psfbuild.hip), parity unpinned.
BBX_ERR_NOTCONV = -5
PSF_REASONS = ('star', 'no shape or flagged', 'peak S/N', 'FWHM or elongation', 'frame edge', 'neighbour')
_PSF_HDR = (('PSF-P', 'successfully processed by the PSF build?'), ('PSF-NOBJ', 'number of stars in the final PSF fit'),
            ('PSF-CHI2', 'mean reduced chi2 of the stars in the final PSF fit'), ('PSF-FWHM', '[pix] median FWHM of the PSF stars'),
            ('PSF-SEE', '[arcsec] PSF-FWHM x pixel scale'), ('PSF-SIZE', '[pix] size of the PSF model image'),
            ('PSF-CFGS', '[pix] size of the PSF vignettes'), ('PSF-SAMP', '[pix] sampling step of the PSF model'),
            ('PSF-PLDG', 'degree of the polynomial in the frame position'), ('PSF-FIX', 'single fixed PSF used for the entire image?'))


def psf_ncoef(poldeg):
    return (poldeg + 1) * (poldeg + 2) // 2


def psf_select(ctx, d_ys, d_xs, d_pk, d_shapes, d_flags, sigma_bkg, fwhm_med, V, ny, nx, cap=None, snr_min=None, fwhm_tol=None,
               elong_max=None, iso_frac=None):
    """bbx_psf_select of the (y, x)-sorted list; fwhm_med: a number, or a one-element float64 device tensor (the frame row of
    bbx_shape_stats, no host wait) -> device (reason uint8 [n], star int32 [cap] (zeros past the kept ones), nstar int32 [2])"""
    S = settings
    cap = int(S.psf_stars_nmax if cap is None else cap)
    n = int(d_ys.numel())
    reason = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    star = torch.zeros(cap, dtype=torch.int32, device=ctx.device)
    nstar = torch.empty(2, dtype=torch.int32, device=ctx.device)
    dev_med = torch.is_tensor(fwhm_med)
    if dev_med and (fwhm_med.dtype != torch.float64 or fwhm_med.numel() != 1):
        raise ValueError('fwhm_med: a number or a one-element float64 device tensor expected')
    check(lib.bbx_psf_select(ctx.h, n, _p(d_ys), _p(d_xs), _p(d_pk), _p(d_shapes), _p(d_flags), float(sigma_bkg),
                             float(S.psf_snr_min if snr_min is None else snr_min), 0.0 if dev_med else float(fwhm_med),
                             _p(fwhm_med) if dev_med else None, float(S.psf_fwhm_tol if fwhm_tol is None else fwhm_tol),
                             float(S.psf_elong_max if elong_max is None else elong_max), float(S.psf_iso_frac if iso_frac is None else iso_frac),
                             int(V), int(ny), int(nx), cap, _p(reason), _p(star), _p(nstar), ctx.stream()), 'bbx_psf_select', ctx.h)
    return reason, star, nstar


def psf_stamps(ctx, img, mask, d_ys, d_xs, d_shapes, d_sig, V, nstar, d_star=None, d_nstar=None, acc=None):
    """bbx_psf_stamps: [nstar] vignettes V x V about the centroids of the sources d_star (None: the first nstar of the list)
    -> device (I float32 [nstar, V, V], w float32 [nstar, V, V], norm float64 [nstar], ok uint8 [nstar])"""
    _args.mask(mask, _args.frame(img))
    nstar, V = int(nstar), int(V)
    dev = ctx.device
    I = torch.empty((nstar, V, V), dtype=torch.float32, device=dev)
    w = torch.empty((nstar, V, V), dtype=torch.float32, device=dev)
    norm = torch.empty(nstar, dtype=torch.float64, device=dev)
    ok = torch.empty(nstar, dtype=torch.uint8, device=dev)
    check(lib.bbx_psf_stamps(ctx.h, img.shape[0], img.shape[1], _p(img), _p(mask), int(d_ys.numel()), _p(d_ys), _p(d_xs), _p(d_shapes),
                             _p(d_sig), nstar, _p(d_star), _p(d_nstar), V, float(settings.psf_accuracy if acc is None else acc), _p(I), _p(w),
                             _p(norm), _p(ok), ctx.stream()), 'bbx_psf_stamps', ctx.h)
    return I, w, norm, ok


def psf_fit(ctx, I, w, terms, ok, chi2=None, chi2_med=None, clip=None):
    """bbx_psf_fit over the stars with ok set and, where chi2 [nstar] and chi2_med [1] (device float32) are given, chi2 <=
    clip * chi2_med -> device basis float32 [ncoef, V, V]"""
    nstar, V = int(I.shape[0]), int(I.shape[1])
    ncoef = int(terms.shape[1])
    basis = torch.empty((ncoef, V, V), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_fit(ctx.h, nstar, V, ncoef, _p(I), _p(w), _p(terms), _p(ok), _p(chi2), _p(chi2_med),
                          float(settings.psf_chi2_clip if clip is None else clip), _p(basis), ctx.stream()), 'bbx_psf_fit', ctx.h)
    return basis


def psf_chi2(ctx, I, w, terms, basis, ok):
    """bbx_psf_chi2 -> device float32 [nstar], NaN where ok is 0"""
    nstar, V = int(I.shape[0]), int(I.shape[1])
    chi2 = torch.empty(nstar, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_chi2(ctx.h, nstar, V, int(terms.shape[1]), _p(I), _p(w), _p(terms), _p(basis), _p(ok), _p(chi2), ctx.stream()),
          'bbx_psf_chi2', ctx.h)
    return chi2


def psf_chi2_median(ctx, chi2, ok):
    """np.median of chi2 over the stars with ok set, on the device without knowing their number there: bbx_mini_median of the
    values taken twice, the others replaced once by the lowest and once by the highest float32 -- the middle pair of that
    sample is the middle (pair) of the ok values.  No ok star: 0.  -> device float32 [1]"""
    good = ok != 0
    big = torch.finfo(torch.float32).max
    both = torch.cat([torch.where(good, chi2, torch.full_like(chi2, -big)), torch.where(good, chi2, torch.full_like(chi2, big))]).contiguous()
    med = torch.empty(1, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_mini_median(ctx.h, both.numel(), _p(both), _p(med), ctx.stream()), 'bbx_mini_median', ctx.h)
    return med


def psf_header(ok, nobj=None, chi2=None, fwhm=None, V=None, poldeg=None, pixscale=None):
    """{PSF-P, PSF-NOBJ, PSF-CHI2, PSF-FWHM, PSF-SEE, PSF-SIZE, PSF-CFGS, PSF-SAMP, PSF-PLDG, PSF-FIX: (value, comment)}; a build that
    failed: PSF-P False and the string 'None', set_qc's default, for the rest.  Pure Python"""
    pixscale = settings.pixscale if pixscale is None else pixscale
    if ok:
        vals = (True, int(nobj), float(chi2), float(fwhm), float(fwhm) * float(pixscale), int(V), int(V), 1.0, int(poldeg), False)
    else:
        vals = (False,) + ('None',) * 9
    return {k: (v, c) for (k, c), v in zip(_PSF_HDR, vals)}


def build_psf(ctx, data_bkgsub, sigma, mask, size, nsy, nsx, cat_nsigma=5.0, sigma_median=None, peaks=None, psf_size=None,
              poldeg=None, max_sources=200000):
    """A PSFEx-style model of the frame's PSF from its own stars (include/bbx.h, bbx_psfbuild.hip):
      peaks of the background-subtracted frame above cat_nsigma x sigma_median (peaks = (ys, xs, pk), host arrays sorted by
      (y, x), where the caller has searched already) -> windowed centroids and adaptive moments from the seed window
      settings.psf_seed_fwhm / 2.3548 -> the frame's median FWHM (bbx_shape_stats, flux = peak, err = sigma) -> bbx_psf_select
      -> bbx_psf_stamps -> bbx_psf_fit over all stars, then settings.psf_nclip rounds of {bbx_psf_chi2, median, fit of the stars
      within settings.psf_chi2_clip x the median} and a last bbx_psf_chi2.
    sigma: the background sigma: a number, a frame, a mini image or a MiniImage (_source_sigma); sigma_median: its median
    (S-BKGSTD; needed unless sigma is a number).  The polynomial terms are those of the integer peak in FITS pixels, where
    source_psfs evaluates the model.  Every degree up to poldeg (settings.psf_poldeg) that the list could support is fitted, and
    the degree taken is the largest with 5 coefficients' worth of stars with a vignette; fewer than settings.psf_nstars_min
    stars in its final fit: no model.  ONE host wait (two when a fit raised the device's soft-fault word), besides the search.
    -> dict(model: dict(basis device float32 [ncoef, V, V], polzero, polscal, poldeg, psf_samp, psf_fwhm) as fitsio.read_psfex
            gives it, or None; header: psf_header; stars: dict(n_sources, n_qualifying, stride, reason [n_sources], index, ys,
            xs [m], ok, used [m], chi2 [m], norm [m]))"""
    S = settings
    V = int(psf_size or S.psf_size)
    poldeg = int(S.psf_poldeg if poldeg is None else poldeg)
    if V < 1 or V > 49 or not V % 2 or not 0 <= poldeg <= 3:
        raise ValueError('psf_size odd and at most 49, psf_poldeg 0..3 expected')
    ny, nx = _args.frame(data_bkgsub)
    if sigma_median is None:
        if not np.isscalar(sigma):
            raise ValueError('sigma_median (median of the sigma image) is needed unless sigma is a number')
        sigma_median = float(sigma)
    sigma_median = float(sigma_median)
    fail = dict(model=None, header=psf_header(False), stars=dict(n_sources=0, n_qualifying=0, stride=1))
    if peaks is None:
        thr = float(cat_nsigma) * sigma_median
        if not (np.isfinite(thr) and thr > 0):
            return fail
        peaks = find_peaks_arrays(ctx, data_bkgsub, thr, max_out=max_sources)
    ys, xs, pk = (np.asarray(a) for a in peaks)
    keep = pk > 0
    ys, xs, pk = ys[keep].astype(np.int32), xs[keep].astype(np.int32), pk[keep].astype(np.float32)
    n = int(ys.size)
    fail['stars']['n_sources'] = n
    if not n or not (np.isfinite(sigma_median) and sigma_median > 0):
        return fail
    nsub = nsy * nsx
    dev = ctx.device
    d_y32, d_x32, d_pk = push(ctx, ys, xs, pk)
    d_sig = _source_sigma(ctx, sigma, (ny, nx), ys, xs)
    sigw = torch.full((nsub,), float(S.psf_seed_fwhm) / 2.3548, dtype=torch.float32, device=dev)
    off = win_centroid(ctx, data_bkgsub, d_y32, d_x32, sigw, size, nsy, nsx)
    d_shp, d_sfl = src_shapes(ctx, data_bkgsub, mask, d_y32, d_x32, off, sigw, size, nsy, nsx)
    d_stab = shape_stats(ctx, d_y32, d_x32, d_shp, d_sfl, d_pk, d_sig, size, nsy, nsx, S.psf_snr_min)
    d_fmed = d_stab[nsub, _SC['med_fwhm']:_SC['med_fwhm'] + 1]         # (a view: one float64 of the frame row)
    cap = max(1, min(int(S.psf_stars_nmax), n))
    d_reason, d_star, d_nstar = psf_select(ctx, d_y32, d_x32, d_pk, d_shp, d_sfl, sigma_median, d_fmed, V, ny, nx, cap=cap)
    I, w, d_norm, d_ok = psf_stamps(ctx, data_bkgsub, mask, d_y32, d_x32, d_shp, d_sig, V, cap, d_star=d_star, d_nstar=d_nstar)
    polzero, polscal = ((nx + 1) / 2.0, (ny + 1) / 2.0), (nx / 2.0, ny / 2.0)
    degs = [d for d in range(poldeg + 1) if 5 * psf_ncoef(d) <= cap] or [0]
    idx = d_star.to(torch.int64)
    fits, back = [], [d_nstar, d_star, d_ok, d_norm, d_reason, d_fmed]
    for d in degs:
        terms = push(ctx, psf_poly_terms(xs + 1.0, ys + 1.0, polzero, polscal, d)).index_select(0, idx).contiguous()
        basis = psf_fit(ctx, I, w, terms, d_ok)
        used = d_ok != 0
        for _ in range(int(S.psf_nclip)):
            chi2 = psf_chi2(ctx, I, w, terms, basis, d_ok)
            med = psf_chi2_median(ctx, chi2, d_ok)
            basis = psf_fit(ctx, I, w, terms, d_ok, chi2, med, S.psf_chi2_clip)
            used = (d_ok != 0) & (chi2 <= float(S.psf_chi2_clip) * med)
        chi2 = psf_chi2(ctx, I, w, terms, basis, d_ok)
        nfit = used.sum().reshape(1)
        csum = torch.where(used, chi2, torch.zeros_like(chi2)).to(torch.float64).sum().reshape(1)
        fits.append(basis)
        back += [used.to(torch.uint8), chi2, nfit, csum]
    try:
        got = fetch(ctx, *back, check_device_errors=True)
    except _lib_BBXError as e:
        if e.code != BBX_ERR_NOTCONV:
            raise
        # a fit met a pixel without a positive definite matrix (a degree with too few stars): the numbers decide below
        got = fetch(ctx, *back)
    (nq, stride), star, ok, norm, reason, fmed = got[:6]
    m = min(-(-int(nq) // max(int(stride), 1)), cap)
    star, ok, norm = star[:m], ok[:m], norm[:m]
    n_ok = int((ok != 0).sum())
    k = max([j for j, d in enumerate(degs) if n_ok >= 5 * psf_ncoef(d)] or [0])
    used, chi2, nfit, csum = got[6 + 4 * k:10 + 4 * k]
    nfit, fwhm = int(nfit[0]), float(fmed[0])
    stars = dict(n_sources=n, n_qualifying=int(nq), stride=int(stride), reason=reason, index=star, ys=ys[star], xs=xs[star], ok=ok,
                 used=used[:m] != 0, chi2=chi2[:m], norm=norm)
    chi2_mean = float(csum[0]) / nfit if nfit else float('nan')
    if nfit < int(S.psf_nstars_min) or not np.isfinite(fwhm) or not np.isfinite(chi2_mean):
        logging.getLogger(__name__).warning('PSF build: %d stars in the final fit (%d sources, %d selected), fewer than the minimum or no '
                                            'finite statistics: no model', nfit, n, int(nq))
        return dict(model=None, header=psf_header(False), stars=stars)
    model = dict(basis=fits[k], polzero=polzero, polscal=polscal, poldeg=degs[k], psf_samp=1.0, psf_fwhm=fwhm)
    return dict(model=model, header=psf_header(True, nfit, chi2_mean, fwhm, V, degs[k]), stars=stars)
