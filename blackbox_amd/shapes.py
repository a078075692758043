"""Source shapes of the catalogue (bbx_src_shapes, bbx_shape_stats): adaptive second moments, the frame's seeing and elongation
statistics and their header keys."""
import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, ptr as _p

# ---- source shapes of the catalogue and the frame's seeing / elongation statistics ---------
# header keys S-NOBJ S-FWHM S-FWSTD S-SEEING S-SEESTD S-ELONG S-ELOSTD (blackbox.py:3051-3057; ranges set_qc.py:256-266).
# [EXT] zogy takes them from SExtractor; here: adaptive second moments (include/bbx.h), parity unpinned.
SHAPE_COLS = ('c_y', 'c_x', 'Tyy', 'Txx', 'Txy', 'FWHM', 'ELONGATION', 'THETA')
SHAPE_STAT_COLS = ('n_qualifying', 'stride', 'n_fwhm', 'med_fwhm', 'std_fwhm', 'n_elong', 'med_elong', 'std_elong')
_SC = {k: i for i, k in enumerate(SHAPE_STAT_COLS)}


def src_shapes(ctx, img, mask, d_ys, d_xs, d_off, d_sigw, size, nsy, nsx, radius=None, niter=None):
    """bbx_src_shapes: adaptive second moments of the sources at the int32 device peaks (d_ys, d_xs) of the frame [img],
    starting at the centroid offsets d_off [n, 2] (win_centroid) -> device (float32 [n, 8] (SHAPE_COLS), NaN rows where a source
    fails; uint8 [n]: OR of [mask] (or None) over each window).  No host wait"""
    radius = settings.centroid_radius if radius is None else radius
    niter = settings.centroid_niter if niter is None else niter
    _args.mask(mask, _args.frame(img))
    n = int(d_ys.numel())
    if d_off.dtype != torch.float32 or tuple(d_off.shape) != (n, 2) or not d_off.is_contiguous():
        raise ValueError('contiguous float32 offsets [n, 2] expected')
    out = torch.empty((n, 8), dtype=torch.float32, device=ctx.device)
    flags = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    check(lib.bbx_src_shapes(ctx.h, img.shape[0], img.shape[1], _p(img), _p(mask) if mask is not None else None, n, _p(d_ys), _p(d_xs),
                             _p(d_off), _p(d_sigw), int(size), int(nsy), int(nsx), int(radius), int(niter), _p(out), _p(flags),
                             ctx.stream()), 'bbx_src_shapes', ctx.h)
    return out, flags


def empty_shape_table(nsub):
    """the table of a frame without a qualifying source: counts 0, stride 1, NaN elsewhere (bbx_shape_stats's empty segments)"""
    t = np.full((nsub + 1, 8), np.nan)
    t[:, [_SC['n_qualifying'], _SC['n_fwhm'], _SC['n_elong']]] = 0.0
    t[:, _SC['stride']] = 1.0
    return t


def shape_stats(ctx, d_ys, d_xs, d_shapes, d_flags, d_flux, d_err, size, nsy, nsx, snr_min=None):
    """bbx_shape_stats of the (y, x)-sorted list -> device float64 [nsy * nsx + 1, 8] (SHAPE_STAT_COLS; last row: the whole
    frame).  No host wait"""
    snr_min = settings.shape_snr_min if snr_min is None else snr_min
    n = int(d_ys.numel())
    if not n:
        return torch.from_numpy(empty_shape_table(nsy * nsx)).to(ctx.device)
    out = torch.empty((nsy * nsx + 1, 8), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_shape_stats(ctx.h, n, _p(d_ys), _p(d_xs), _p(d_shapes), _p(d_flags), _p(d_flux), _p(d_err), int(size), int(nsy), int(nsx),
                              float(snr_min), _p(out), ctx.stream()), 'bbx_shape_stats', ctx.h)
    return out


def shape_columns(ys, xs, shp, flags):
    """the catalogue columns made of the rows of bbx_src_shapes (host, float32 [n, 8]) and its flags: X_POS / Y_POS = peak + 1 +
    offset (the integer peak where the source has no shape), FWHM, ELONGATION, A, B = sqrt of the eigenvalues of T, THETA,
    X2 = Txx, Y2 = Tyy, XY = Txy, FLAGS_MASK"""
    shp = np.asarray(shp, np.float32).reshape(-1, 8)
    F = np.float32
    cy, cx, Tyy, Txx, Txy = (shp[:, k] for k in range(5))
    with np.errstate(invalid='ignore'):
        tr, df = Tyy + Txx, Txx - Tyy
        rad = np.sqrt(df * df + F(4) * (Txy * Txy))
        A, B = np.sqrt((tr + rad) / F(2)), np.sqrt((tr - rad) / F(2))
    return dict(Y_POS=(np.asarray(ys).astype(F) + F(1)) + np.where(np.isnan(cy), F(0), cy),
                X_POS=(np.asarray(xs).astype(F) + F(1)) + np.where(np.isnan(cx), F(0), cx),
                FWHM=shp[:, 5].copy(), ELONGATION=shp[:, 6].copy(), A=A.astype(F), B=B.astype(F), THETA=shp[:, 7].copy(),
                X2=Txx.copy(), Y2=Tyy.copy(), XY=Txy.copy(), FLAGS_MASK=np.asarray(flags, np.uint8).copy())


_SHAPE_HDR = (('S-FWHM', 'med_fwhm', 1, '[pix] median FWHM of the unflagged stars'), ('S-FWSTD', 'std_fwhm', 1, '[pix] sigma (STD) FWHM'),
              ('S-SEEING', 'med_fwhm', 0, '[arcsec] median seeing of the unflagged stars'), ('S-SEESTD', 'std_fwhm', 0, '[arcsec] sigma (STD) seeing'),
              ('S-ELONG', 'med_elong', 1, 'median elongation of the unflagged stars'), ('S-ELOSTD', 'std_elong', 1, 'sigma (STD) elongation'))


def shape_header(table, nobj, nmin, pixscale):
    """the table of bbx_shape_stats [nsub + 1, 8] (host) -> {S-NOBJ, S-FWHM, S-FWSTD, S-SEEING, S-SEESTD, S-ELONG, S-ELOSTD:
    (value, comment)} from the full-frame row; S-SEEING, S-SEESTD = the FWHM values x pixscale.  With fewer than nmin clipped
    values of either quantity in that row the six statistics are the string 'None' (set_qc's default).  Pure numpy"""
    full = np.asarray(table, np.float64)[-1]
    hdr = {'S-NOBJ': (int(nobj), 'number of objects in the catalogue')}
    good = bool(full[_SC['n_fwhm']] >= nmin and full[_SC['n_elong']] >= nmin)
    for key, col, plain, comment in _SHAPE_HDR:
        hdr[key] = ((float(full[_SC[col]]) if plain else float(full[_SC[col]]) * float(pixscale)) if good else 'None', comment)
    return hdr
