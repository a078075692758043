"""Transient vetting: the PSF of D per sub-image (bbx_zogy_pd_stamps), its fit to D at every candidate (bbx_trans_psffit,
DESIGN.md 4j), the Gauss and Moffat fits (bbx_trans_shapefit), their header keys, the vetting, and the
thumbnails of the candidates (bbx_thumbnails)."""
import ctypes as C

import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, push, ptr as _p
from .peaks import window_sigma

PD_FOLD_WARN = 0.01             # a T-PDFOLD above this is logged: P_D does not fit its stamp (Moffat pairs fold 1e-4 at most, a point / box pair 0.15)
TRANS_AT_BOUND, TRANS_MASKED, TRANS_NO_FIT, TRANS_NOT_CONVERGED = 1, 2, 4, 8       # FLAGS_PSF_D bits (include/bbx.h, bbx_trans_psffit)


def pd_stamps(ctx, sub_pn, sub_pr, scal, M=None):
    """bbx_zogy_pd_stamps: the PSF of the difference image of every sub-image from its two PSF stamps [nsub, S, S] (device float32,
    unit sum) and scal [nsub, 6] = (sn, sr, fn, fr, dx, dy) (host), on a grid of M x M (settings.trans_pd_grid)
    -> device (pd float32 [nsub, S, S], fold float32 [nsub]: the share of sum |p| on the grid that the stamp leaves out).  No host wait"""
    M = int(settings.trans_pd_grid if M is None else M)
    if sub_pn.dim() != 3 or sub_pn.dtype != torch.float32 or sub_pr.dtype != torch.float32 or tuple(sub_pn.shape) != tuple(sub_pr.shape) or \
            sub_pn.shape[1] != sub_pn.shape[2]:
        raise ValueError('two float32 stamp tensors [nsub, S, S] of one shape expected')
    nsub, S = int(sub_pn.shape[0]), int(sub_pn.shape[1])
    scal = _args.scal6(scal, nsub)
    sub_pn, sub_pr = sub_pn.contiguous(), sub_pr.contiguous()
    pd = torch.empty((nsub, S, S), dtype=torch.float32, device=ctx.device)
    fold = torch.empty(nsub, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_zogy_pd_stamps(ctx.h, nsub, S, M, _p(sub_pn), _p(sub_pr), scal.ctypes.data_as(C.POINTER(C.c_float)), _p(pd), _p(fold),
                                 ctx.stream()), 'bbx_zogy_pd_stamps', ctx.h)
    return pd, fold


def trans_psffit(ctx, D, N, R, sig_n, sig_r, mask, pd, ys, xs, scal, size, nsx, fit_size=None, niter=None, maxshift=None, d_peaks=None):
    """bbx_trans_psffit: the PSF of D (pd [nsub, S, S], pd_stamps) fitted to D with free position in a window of fit_size x fit_size
    pixels around every candidate's integer peak (ys, xs: host arrays; d_peaks: the same as int32 device tensors where the caller
    has them).  N, R: the background-subtracted new and reference frames; sig_n, sig_r: their sigma maps, two frames or two
    MiniImage; mask: uint8 frame or None, its pixels are left out; scal [nsub, 6] (host); fit_size, niter, maxshift: settings.trans_fit_*
    -> device (flux, err, dy, dx, chi2 float32 [n], flags uint8 [n]: TRANS_AT_BOUND | TRANS_MASKED | TRANS_NO_FIT |
    TRANS_NOT_CONVERGED).  No host wait"""
    ny, nx = _args.frames(D, N, R)
    _args.mask(mask, (ny, nx))
    sigmas = _args.sigma_maps(sig_n, sig_r, (ny, nx))
    if pd.dim() != 3 or pd.dtype != torch.float32 or pd.shape[1] != pd.shape[2] or not pd.is_contiguous():
        raise ValueError('contiguous float32 stamps [nsub, S, S] expected')
    nsub, S = int(pd.shape[0]), int(pd.shape[1])
    scal = _args.scal6(scal, nsub)
    n, d_ys, d_xs = _args.peaks(ctx, ys, xs, d_peaks)
    dev = ctx.device
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(5)] + [torch.empty(n, dtype=torch.uint8, device=dev)]
    W = int(settings.trans_fit_size if fit_size is None else fit_size)
    check(lib.bbx_trans_psffit(ctx.h, ny, nx, _p(D), _p(N), _p(R), *sigmas, _p(mask) if mask is not None else None, S, nsub,
                               _p(pd), int(size), int(nsx), scal.ctypes.data_as(C.POINTER(C.c_float)), n, _p(d_ys), _p(d_xs), W,
                               int(settings.trans_fit_niter if niter is None else niter),
                               float(settings.trans_fit_maxshift if maxshift is None else maxshift), *[_p(o) for o in outs], ctx.stream()),
          'bbx_trans_psffit', ctx.h)
    return tuple(outs)


def trans_fit_header(on, fit_size=None, rows=None, fold=None):
    """the keys of `_trans_hdr.fits` for the fit of P_D to D: T-PSFD, and with it T-FITSZ, T-NFIT (rows with flags & 12 == 0),
    T-PDFOLD (the largest fold over the sub-images), T-CHI2MD (the median chi2 of those rows; 'None' without any)"""
    h = {'T-PSFD': (bool(on), 'PSF of D fitted to the transient candidates?')}
    if on:
        good = [r['chi2_psf_d'] for r in rows if not r['flags_psf_d'] & (TRANS_NO_FIT | TRANS_NOT_CONVERGED)]
        h['T-FITSZ'] = (int(fit_size), '[pix] side of the window of the fit of P_D to D')
        h['T-NFIT'] = (len(good), 'number of candidates with a converged fit')
        h['T-PDFOLD'] = (float(np.max(fold)) if len(fold) else 'None', 'largest share of |P_D| outside its stamp')
        h['T-CHI2MD'] = (float(np.median(good)) if good else 'None', 'median CHI2_PSF_D of the converged fits')
    return h


TRANS_SHAPE_REFUSED = 16                                             # FLAGS_GAUSS_D / FLAGS_MOFFAT_D: bits 1 2 4 8 as above, and this (bbx_trans_shapefit)
SHAPE_GAUSS, SHAPE_MOFFAT = 1, 2                                     # `models` of bbx_trans_shapefit
SHAPE_OUT = ('y', 'x', 'yerr', 'xerr', 'fwhm', 'elong', 'chi2')      # the planes of its output


def trans_shapefit(ctx, D, N, R, sig_n, sig_r, mask, fwhm0, ys, xs, scal, size, nsx, fit_size=None, niter=None, maxshift=None, models=3,
                   beta=None, fwhm_lo=None, fwhm_hi=None, d_peaks=None):
    """bbx_trans_shapefit: an elliptical Gaussian and an elliptical Moffat (beta fixed) fitted to D in the window of trans_psffit
    (fit_size x fit_size pixels around every candidate's integer peak, the same used pixels and V_D) by Levenberg-Marquardt.  The
    arguments are trans_psffit's, but for fwhm0 (device float32 [nsub]: the FWHM the fits start with in every sub-image) in the
    place of the P_D stamps; fit_size, niter, maxshift, beta, fwhm_lo, fwhm_hi: settings.trans_shape_* / trans_moffat_beta (fwhm_hi
    None: twice the window's side); models: SHAPE_GAUSS | SHAPE_MOFFAT
    -> device (out float32 [2, 7, n]: per model (Gauss, Moffat) the planes SHAPE_OUT, y and x relative to the integer peak;
    flags uint8 [2, n]: TRANS_AT_BOUND | TRANS_MASKED | TRANS_NO_FIT | TRANS_NOT_CONVERGED | TRANS_SHAPE_REFUSED).  No host wait"""
    ny, nx = _args.frames(D, N, R)
    _args.mask(mask, (ny, nx))
    sigmas = _args.sigma_maps(sig_n, sig_r, (ny, nx))
    scal = _args.scal6(scal)
    nsub = int(scal.shape[0])
    if not torch.is_tensor(fwhm0) or fwhm0.dtype != torch.float32 or tuple(fwhm0.shape) != (nsub,) or not fwhm0.is_contiguous():
        raise ValueError('fwhm0: a contiguous float32 device tensor [nsub] expected')
    n, d_ys, d_xs = _args.peaks(ctx, ys, xs, d_peaks)
    dev = ctx.device
    out = torch.zeros((2, len(SHAPE_OUT), n), dtype=torch.float32, device=dev)
    flags = torch.full((2, n), TRANS_NO_FIT, dtype=torch.uint8, device=dev)        # (what a call with models == 0 leaves)
    W = int(settings.trans_shape_size if fit_size is None else fit_size)
    hi = settings.trans_shape_fwhm_hi if fwhm_hi is None else fwhm_hi
    check(lib.bbx_trans_shapefit(ctx.h, ny, nx, _p(D), _p(N), _p(R), *sigmas, _p(mask) if mask is not None else None, nsub,
                                 int(size), int(nsx), scal.ctypes.data_as(C.POINTER(C.c_float)), _p(fwhm0), n, _p(d_ys), _p(d_xs), W,
                                 int(settings.trans_shape_niter if niter is None else niter),
                                 float(settings.trans_shape_maxshift if maxshift is None else maxshift), int(models),
                                 float(settings.trans_moffat_beta if beta is None else beta),
                                 float(settings.trans_shape_fwhm_lo if fwhm_lo is None else fwhm_lo), float(2 * W if hi is None else hi),
                                 _p(out), _p(flags), ctx.stream()), 'bbx_trans_shapefit', ctx.h)
    return out, flags


def shape_start_fwhm(sub_pn, sub_pr):
    """the FWHM the shape fits start with, per sub-image: 2.3548 x the larger window_sigma of the two PSF stamps; device float32
    [nsub], no fetch"""
    return (2.3548 * torch.maximum(window_sigma(sub_pn), window_sigma(sub_pr))).to(torch.float32).contiguous()


def trans_shape_header(on, fit_size=None, beta=None, rows=None):
    """the keys of `_trans_hdr.fits` for the Gauss and Moffat fits to D: T-SHAPE, and with it T-SHPSZ, T-MBETA, T-NGAUS, T-NMOFF (rows
    with flags & 12 == 0), T-FWGMD, T-ELGMD (the medians over the converged Gauss rows; 'None' without any)"""
    h = {'T-SHAPE': (bool(on), 'Gauss and Moffat fitted to the transient candidates?')}
    if on:
        bad = TRANS_NO_FIT | TRANS_NOT_CONVERGED
        good = [r for r in rows if not r['flags_gauss_d'] & bad]
        h['T-SHPSZ'] = (int(fit_size), '[pix] side of the window of the Gauss and Moffat fits')
        h['T-MBETA'] = (float(beta), 'beta of the Moffat fit (fixed)')
        h['T-NGAUS'] = (len(good), 'number of candidates with a converged Gauss fit')
        h['T-NMOFF'] = (sum(1 for r in rows if not r['flags_moffat_d'] & bad), 'number of candidates with a converged Moffat fit')
        h['T-FWGMD'] = (float(np.median([r['fwhm_gauss_d'] for r in good])) if good else 'None', '[pix] median FWHM_GAUSS_D of the converged fits')
        h['T-ELGMD'] = (float(np.median([r['elong_gauss_d'] for r in good])) if good else 'None', 'median ELONG_GAUSS_D of the converged fits')
    return h


def vet_transients(rows, chi2_max=None, fwhm_gauss_min=None, fwhm_gauss_max=None, elong_gauss_max=None):
    """the rows that pass the vetting -> (kept rows, their indices).  chi2_max (--trans_chi2_max): those with a fit of P_D (no
    TRANS_NO_FIT) and chi2_psf_d <= chi2_max.  With any of the Gauss bounds (--trans_fwhm_gauss_min / _max, --trans_elong_gauss_max):
    those with a Gauss fit (no TRANS_NO_FIT) inside every bound given"""
    keep = list(range(len(rows)))
    if chi2_max is not None:
        keep = [i for i in keep if not rows[i]['flags_psf_d'] & TRANS_NO_FIT and rows[i]['chi2_psf_d'] <= chi2_max]
    if fwhm_gauss_min is not None or fwhm_gauss_max is not None or elong_gauss_max is not None:
        keep = [i for i in keep if not rows[i]['flags_gauss_d'] & TRANS_NO_FIT
                and (fwhm_gauss_min is None or rows[i]['fwhm_gauss_d'] >= fwhm_gauss_min)
                and (fwhm_gauss_max is None or rows[i]['fwhm_gauss_d'] <= fwhm_gauss_max)
                and (elong_gauss_max is None or rows[i]['elong_gauss_d'] <= elong_gauss_max)]
    return [rows[i] for i in keep], keep


# ---- the candidate table from the host copies of what the subtraction queued (numpy arrays and lists of dicts only: nothing
# here touches the device)
def candidate_rows(ys, xs, scorr, fe):
    """the rows of the candidate table: the peaks of Scorr and (Fpsf, Fpsferr) = fe[0], fe[1] at them"""
    return [dict(y=y, x=x, scorr=sc, fpsf=f, fpsferr=e)
            for y, x, sc, f, e in zip(ys.tolist(), xs.tolist(), scorr.tolist(), fe[0].tolist(), fe[1].tolist())]


def sky_columns(rows, sky):
    """ra_peak, dec_peak from sky [n, 2] and, where the fitted positions' rows follow ([2n, 2]), ra_psf_d, dec_psf_d"""
    n = len(rows)
    for i, d in enumerate(rows):
        d.update(ra_peak=float(sky[i, 0]), dec_peak=float(sky[i, 1]))
        if len(sky) == 2 * n:
            d.update(ra_psf_d=float(sky[n + i, 0]), dec_psf_d=float(sky[n + i, 1]))


def pd_columns(rows, tf):
    """the columns of the fit of P_D from its flat copy back: six planes of n (flux, error, dy, dx, chi2, flags), then the fold
    of P_D per sub-image, which is returned"""
    n = len(rows)
    cols, fold = tf[:6 * n].reshape(6, n), tf[6 * n:]
    for i, d in enumerate(rows):
        d.update(y_psf_d=float(d['y'] + cols[2, i]), x_psf_d=float(d['x'] + cols[3, i]), flux_psf_d=float(cols[0, i]),
                 fluxerr_psf_d=float(cols[1, i]), chi2_psf_d=float(cols[4, i]), flags_psf_d=int(cols[5, i]))
    return fold


def shapefit_columns(rows, ts):
    """the sixteen Gauss / Moffat columns from the flat copy back of the shape fits: two models x seven planes of n (dy, dx, yerr,
    xerr, fwhm, elongation, chi2), then two flag planes"""
    n = len(rows)
    planes, sfl = ts[:14 * n].reshape(2, 7, n), ts[14 * n:].reshape(2, n)
    for m, name in enumerate(('gauss', 'moffat')):
        for i, d in enumerate(rows):
            d.update({'x_%s_d' % name: float(d['x'] + planes[m, 1, i]), 'xerr_%s_d' % name: float(planes[m, 3, i]),
                      'y_%s_d' % name: float(d['y'] + planes[m, 0, i]), 'yerr_%s_d' % name: float(planes[m, 2, i]),
                      'fwhm_%s_d' % name: float(planes[m, 4, i]), 'elong_%s_d' % name: float(planes[m, 5, i]),
                      'chi2_%s_d' % name: float(planes[m, 6, i]), 'flags_%s_d' % name: int(sfl[m, i])})


def drop_edge_rows(rows, edge_at):
    """the rows with a reference under their peak (edge_at: the registered reference's edge bit per row) -> (kept rows, their indices)"""
    keep = [i for i, v in enumerate(edge_at.tolist()) if not v]
    return [rows[i] for i in keep], keep


def vet_rows(rows, have_fit, have_shapes, chi2_max=None, fwhm_gauss_min=None, fwhm_gauss_max=None, elong_gauss_max=None):
    """the vetting with the bounds that apply: the chi2 bound needs the fit of P_D, the Gauss bounds the shape fits -> (kept rows,
    their indices); (rows, None) where no bound applies"""
    bounds = dict(chi2_max=chi2_max if have_fit else None)
    if have_shapes:
        bounds.update(fwhm_gauss_min=fwhm_gauss_min, fwhm_gauss_max=fwhm_gauss_max, elong_gauss_max=elong_gauss_max)
    if not any(v is not None for v in bounds.values()):
        return rows, None
    return vet_transients(rows, **{k: None if v is None else float(v) for k, v in bounds.items()})


def thumbnail_stamps(ctx, res, frames, ys, xs, size, new_mask, ref_mask=None, floats=True, pngs=False, flag_win=None):
    """bbx_thumbnails (+ bbx_thumb_png8) at the integer positions (ys, xs) of the four frames (RED, REF, D, SCORR): puts
    'thumbnails' (device float32 [n, 4, size, size], when [floats]) and 'thumbnail_png8' (device uint8, same shape, when [pngs])
    into [res] and returns the device flags [n] (uint8: OR of the masks over the flag window); n = 0 gives empty tensors and
    launches nothing.  No host wait"""
    n = int(len(ys))
    dev = ctx.device
    out = torch.empty((n, 4, size, size), dtype=torch.float32, device=dev)
    d_fl = torch.empty(n, dtype=torch.uint8, device=dev)
    png = torch.empty((n, 4, size, size), dtype=torch.uint8, device=dev) if pngs else None
    if n:
        frames = [f.contiguous() for f in frames]
        ny, nx = _args.frames(*frames)
        for m in (new_mask, ref_mask):
            _args.mask(m, (ny, nx))
        d_y32, d_x32 = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
        planes = (C.c_void_p * 4)(*[f.data_ptr() for f in frames])
        win = int(settings.trans_flags_window if flag_win is None else flag_win)
        check(lib.bbx_thumbnails(ctx.h, ny, nx, planes, n, _p(d_y32), _p(d_x32), size, _p(new_mask),
                                 _p(ref_mask) if ref_mask is not None else None, win, _p(out), _p(d_fl), ctx.stream()),
              'bbx_thumbnails', ctx.h)
        if pngs:
            check(lib.bbx_thumb_png8(ctx.h, 4 * n, size, _p(out), _p(png), None, ctx.stream()), 'bbx_thumb_png8', ctx.h)
    if floats:
        res['thumbnails'] = out
    if pngs:
        res['thumbnail_png8'] = png
    return d_fl
