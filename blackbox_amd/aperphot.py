"""Aperture photometry of the catalogue with a local sky annulus (bbx_aper_phot): the model-independent fluxes
E_FLUX_APER_R<r>xFWHM / E_FLUXERR_APER_R<r>xFWHM of the reference's catalogues (qc.py:489-502, set_zogy.apphot_radii), the local sky
of every source and the AP-* header keys.  [EXT] zogy's get_apflux and SExtractor are not in the reference tree: only the column
names and the radii follow the reference, the rules are this project's own (include/bbx.h), parity unpinned."""
import ctypes as C

import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, ptr as _p

# FLAGS_APER bits (include/bbx.h, bbx_aper_phot)
APER_NO_CENTROID, APER_MASKED, APER_OFF_FRAME, APER_FEW_SKY, APER_SKY_CUT, APER_TOO_BIG = 1, 2, 4, 8, 16, 32
APER_RMAX, APER_NMAX = 48, 8                                         # BBX_APER_RMAX, BBX_APER_NMAX
FWHM_PER_SIGMA = 2.0 * np.sqrt(2.0 * np.log(2.0))
APER_EXTRA = ('BKG_APER', 'BKGSTD_APER', 'NSKY_APER', 'FWHM_APER', 'FLAGS_APER')


def _radii(radii):
    radii = settings.apphot_radii if radii is None else radii
    radii = tuple(float(r) for r in np.atleast_1d(radii))
    if not 1 <= len(radii) <= APER_NMAX or not all(np.isfinite(r) and r > 0 for r in radii):
        raise ValueError('1 to %d positive aperture radii expected, got %r' % (APER_NMAX, radii))
    return radii


def aper_fwhm(sub_psfs):
    """the frame's FWHM of the apertures from the unit-sum PSF stamps of its sub-images [nsub, S, S] (device): 2 sqrt(2 ln 2) x the
    lower median (torch.median) over the tiles of peaks.window_sigma, the sigma of the Gaussian with the PSF's effective area -> device
    float32 [1].  One number per frame, so that a column name means one thing in a frame.  No host wait"""
    from .peaks import window_sigma
    return (window_sigma(sub_psfs).reshape(-1).median() * np.float32(FWHM_PER_SIGMA)).to(torch.float32).reshape(1)


def aper_phot(ctx, D, sigma, mask, d_ys, d_xs, d_off, d_fwhm, size, nsy, nsx, radii=None, sky_inout=None, sub_sky=None, sky_nmin=None):
    """bbx_aper_phot: aperture fluxes of the sources at the int32 device peaks (d_ys, d_xs) of the frame [D] about peak + d_off
    [n, 2] (win_centroid; None: the peaks themselves), in circles of radii x d_fwhm [nsy * nsx] (float32, per tile) with the exact
    circle-pixel overlap as weight, and the clipped median of the annulus sky_inout x FWHM.  sigma: the sigma frame of D or a
    MiniImage; mask: uint8 frame or None, its pixels are left out.
    -> device (flux float32 [n, naper], err float32 [n, naper], sky float32 [n, 3] = (median, std, n), flags uint8 [n]: APER_*).
    No host wait"""
    radii = _radii(radii)
    sky_in, sky_out = (float(v) for v in (settings.apphot_sky_inout if sky_inout is None else sky_inout))
    sub_sky = settings.apphot_local_sky if sub_sky is None else sub_sky
    sky_nmin = int(settings.apphot_sky_nmin if sky_nmin is None else sky_nmin)
    if not 0 <= sky_in < sky_out or not np.isfinite(sky_out) or sky_nmin < 1:
        raise ValueError('sky annulus 0 <= inner < outer and sky_nmin >= 1 expected')
    ny, nx = _args.frame(D)
    _args.mask(mask, (ny, nx))
    sig = _args.sigma_map(sigma, (ny, nx))
    for t in (d_ys, d_xs):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError('contiguous int32 peaks [n] expected')
    n = int(d_ys.numel())
    if int(d_xs.numel()) != n:
        raise ValueError('as many x as y peaks expected')
    if d_off is not None and (d_off.dtype != torch.float32 or tuple(d_off.shape) != (n, 2) or not d_off.is_contiguous()):
        raise ValueError('contiguous float32 offsets [n, 2] expected')
    size, nsy, nsx = int(size), int(nsy), int(nsx)
    if size < 1 or nsy < 1 or nsx < 1:
        raise ValueError('size, nsy, nsx must be positive')
    if d_fwhm.dtype != torch.float32 or d_fwhm.numel() != nsy * nsx or not d_fwhm.is_contiguous():
        raise ValueError('contiguous float32 FWHM [nsy * nsx] expected')
    naper = len(radii)
    dev = ctx.device
    flux = torch.empty((n, naper), dtype=torch.float32, device=dev)
    err = torch.empty((n, naper), dtype=torch.float32, device=dev)
    sky = torch.empty((n, 3), dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    h_r = (C.c_float * naper)(*radii)
    check(lib.bbx_aper_phot(ctx.h, ny, nx, _p(D), *sig, _p(mask) if mask is not None else None, n, _p(d_ys), _p(d_xs),
                            _p(d_off) if d_off is not None else None, _p(d_fwhm), size, nsy, nsx, naper, h_r, sky_in, sky_out,
                            1 if sub_sky else 0, sky_nmin, _p(flux), _p(err), _p(sky), _p(flags), ctx.stream()), 'bbx_aper_phot', ctx.h)
    return flux, err, sky, flags


def aper_column_names(radii=None):
    """E_FLUX_APER_R<r>xFWHM, E_FLUXERR_APER_R<r>xFWHM per radius (written by '%g', qc.py:494-497), then BKG_APER, BKGSTD_APER,
    NSKY_APER, FWHM_APER, FLAGS_APER"""
    names = []
    for r in _radii(radii):
        names += ['E_FLUX_APER_R%gxFWHM' % r, 'E_FLUXERR_APER_R%gxFWHM' % r]
    return names + list(APER_EXTRA)


def aper_columns(flux, err, sky, flags, fwhm, radii=None):
    """the catalogue columns made of bbx_aper_phot's outputs (host) and the frame's FWHM, in aper_column_names's order"""
    radii = _radii(radii)
    F = np.float32
    flux, err = np.asarray(flux, F).reshape(-1, len(radii)), np.asarray(err, F).reshape(-1, len(radii))
    sky = np.asarray(sky, F).reshape(-1, 3)
    names = aper_column_names(radii)
    cols = {}
    for k in range(len(radii)):
        cols[names[2 * k]], cols[names[2 * k + 1]] = flux[:, k].copy(), err[:, k].copy()
    cols.update(BKG_APER=sky[:, 0].copy(), BKGSTD_APER=sky[:, 1].copy(), NSKY_APER=sky[:, 2].astype(np.int32),
                FWHM_APER=np.full(len(flux), fwhm, F), FLAGS_APER=np.asarray(flags, np.uint8).copy())
    return cols


def _clipped_median(v, nsigma=3.0, rounds=5):
    """median of v after clipping at nsigma x the population std about the median, until nothing leaves -> (median, n)"""
    v = np.asarray(v, np.float64)
    for _ in range(rounds):
        if not v.size:
            break
        med, sd = np.median(v), v.std()
        keep = np.abs(v - med) <= nsigma * sd
        if keep.all():
            break
        v = v[keep]
    return (float(np.median(v)), int(v.size)) if v.size else (float('nan'), 0)


def aper_header(ok, fwhm=None, radii=None, sky_inout=None, local_sky=None, cols=None, flux_opt=None, snr_opt=None, snr_min=None, nmin=None):
    """{AP-P, AP-FWHM, AP-NAPER, AP-R1..n, AP-SKYIN, AP-SKYOU, AP-LSKY, AP-NSTAR, AP-OPT1..n: (value, comment)}.  AP-OPTk = the
    3 sigma clipped median of E_FLUX_APER_k / E_FLUX_OPT over the AP-NSTAR sources with FLAGS_APER == 0 and SNR_OPT >= snr_min
    (settings.shape_snr_min); with fewer than nmin (settings.shape_nmin) of them the string 'None'.  ok False: AP-P alone.
    Pure numpy"""
    hdr = {'AP-P': (bool(ok), 'aperture photometry of the catalogue made?')}
    if not ok:
        return hdr
    radii = _radii(radii)
    sky_in, sky_out = settings.apphot_sky_inout if sky_inout is None else sky_inout
    snr_min = settings.shape_snr_min if snr_min is None else snr_min
    nmin = settings.shape_nmin if nmin is None else nmin
    names = aper_column_names(radii)
    hdr['AP-FWHM'] = (float(fwhm), '[pix] FWHM the aperture radii are multiples of')
    hdr['AP-NAPER'] = (len(radii), 'number of apertures')
    for k, r in enumerate(radii):
        hdr['AP-R%d' % (k + 1)] = (float(r), '[FWHM] radius of aperture %d' % (k + 1))
    hdr['AP-SKYIN'] = (float(sky_in), '[FWHM] inner radius of the sky annulus')
    hdr['AP-SKYOU'] = (float(sky_out), '[FWHM] outer radius of the sky annulus')
    hdr['AP-LSKY'] = (bool(settings.apphot_local_sky if local_sky is None else local_sky), 'local sky subtracted from the aperture fluxes?')
    fo, so = np.asarray(flux_opt, np.float64), np.asarray(snr_opt, np.float64)
    with np.errstate(invalid='ignore'):
        good = (np.asarray(cols['FLAGS_APER']) == 0) & (so >= snr_min)
    hdr['AP-NSTAR'] = (int(good.sum()), 'unflagged sources behind AP-OPT*')
    for k in range(len(radii)):
        val = 'None'
        if good.sum() >= nmin:
            ratio = np.asarray(cols[names[2 * k]], np.float64)[good] / fo[good]
            val = _clipped_median(ratio[np.isfinite(ratio)])[0]
            val = val if np.isfinite(val) else 'None'
        hdr['AP-OPT%d' % (k + 1)] = (val, 'median E_FLUX_APER_%d / E_FLUX_OPT of these' % (k + 1))
    return hdr
