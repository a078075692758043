"""Limiting-flux image of the reduced frame (bbx_limflux_image): `_red_limmag.fits` of set_blackbox.py:157-159 and
the frame keys LIMEFLUX, LIMFNU, LIMMAG of blackbox.py:3151-3153.  At every pixel nsigma x the error of the PSF-weighted optimal
flux of a faint source centred there, on sky noise alone: what bbx_psf_optflux* return as err, dense.  [EXT]
zogy.get_psfoptflux(get_limflux_array=True) is not in the reference tree: only the file name, the key names and the 5 sigma
convention follow the reference, the rules are this project's own (include/bbx.h), parity unpinned."""
import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, ptr as _p

LIM_SMAX = 49                                                        # BBX_LIMFLUX_SMAX
_NONE = 'None'


def _nsigma(nsigma):
    nsigma = float(settings.limmag_nsigma if nsigma is None else nsigma)
    if not (np.isfinite(nsigma) and nsigma > 0):
        raise ValueError('limmag_nsigma: a positive number expected, got %r' % (nsigma,))
    return nsigma


def _frac(frac):
    frac = float(settings.limmag_psf_frac if frac is None else frac)
    if not 0.0 <= frac < 1.0:
        raise ValueError('limmag_psf_frac: a number in [0, 1) expected, got %r' % (frac,))
    return frac


def check_parameters(nsigma=None, frac=None):
    """(nsigma, frac) with the settings in place of None; a ValueError for an nsigma that is not positive or a frac outside [0, 1)"""
    return _nsigma(nsigma), _frac(frac)


def limflux_image(ctx, sigma, mask, sub_psfs, size, nsy, nsx, nsigma=None, frac=None):
    """bbx_limflux_image: the limiting flux at every pixel of the frame whose sigma map is [sigma] (a contiguous float32 frame or a
    MiniImage with a .shape) and whose mask is [mask] (uint8 frame or None: its pixels carry no weight), with the unit-sum PSF stamps
    sub_psfs [nsy * nsx, S, S] of its tiles of [size] pixels (S odd, <= 49).  nsigma, frac: settings.limmag_nsigma,
    settings.limmag_psf_frac.  -> device (lim float32 [ny, nx], win int32 [nsy * nsx]: the window T of every tile, 0 for a stamp
    without a sum).  No host wait"""
    nsigma, frac = _nsigma(nsigma), _frac(frac)
    shape = tuple(int(v) for v in sigma.shape)
    if len(shape) != 2:
        raise ValueError('sigma: a contiguous float32 frame or a MiniImage expected')
    ny, nx = shape
    _args.mask(mask, shape)
    sig = _args.sigma_map(sigma, shape)
    size, nsy, nsx = int(size), int(nsy), int(nsx)
    if size < 1 or nsy < 1 or nsx < 1:
        raise ValueError('size, nsy, nsx must be positive')
    if sub_psfs.dtype != torch.float32 or sub_psfs.dim() != 3 or not sub_psfs.is_contiguous() or sub_psfs.shape[0] != nsy * nsx or \
            sub_psfs.shape[1] != sub_psfs.shape[2]:
        raise ValueError('contiguous float32 PSF stamps [nsy * nsx, S, S] expected')
    S = int(sub_psfs.shape[1])
    if S % 2 == 0 or S > LIM_SMAX:
        raise ValueError('PSF stamps of an odd side of at most %d expected, got %d' % (LIM_SMAX, S))
    dev = ctx.device
    lim = torch.empty((ny, nx), dtype=torch.float32, device=dev)
    win = torch.empty(nsy * nsx, dtype=torch.int32, device=dev)
    check(lib.bbx_limflux_image(ctx.h, ny, nx, *sig, _p(mask) if mask is not None else None, S, _p(sub_psfs), size, nsy, nsx, nsigma, frac,
                                _p(lim), _p(win), ctx.stream()), 'bbx_limflux_image', ctx.h)
    return lim, win


def limit_magnitudes(lim, zp, exptime, ext=0.0):
    """a limiting flux [e-] per pixel (device tensor) -> magnitudes: zp - 2.5 log10(lim / exptime) - ext, 0 where lim is not
    positive.  The one conversion of `_trans_limmag` and `_red_limmag`"""
    return torch.where(lim > 0, zp - 2.5 * torch.log10(lim.clamp(min=1e-30) / exptime) - ext, torch.zeros_like(lim))


def limflux_header(ok, stat=None, win=None, nsigma=None, frac=None, exptime=None, zp=None, ext=0.0):
    """{LIMMAG-P, LIMNSIG, LIMEFLUX, LIMMAG, LIMFNU, LIMPFRAC, LIMWIN, LIMNPIX: (value, comment)}.  stat: the eight doubles of
    bbx_frame_clipped_stats of the image (n, median, ...); win: the tiles' windows.  LIMEFLUX = median / exptime [e-/s]; with a
    zeropoint LIMMAG = zp - 2.5 log10(LIMEFLUX) - ext and LIMFNU = 10^(-0.4 (LIMMAG - 23.9)) [uJy], 'None' without one.  ok False,
    or a statistic without a positive finite median: LIMMAG-P False and 'None' everywhere else.  LIMWIN: the lower median of the
    windows of the tiles that have one (T > 0), so that it is a window side, an odd number.  Pure numpy"""
    med = n = None
    if ok and stat is not None:
        st = np.asarray(stat, np.float64).reshape(-1)
        n, med = int(st[0]), float(st[1])
    ok = bool(bool(ok) and med is not None and n > 0 and np.isfinite(med) and med > 0)
    hdr = {'LIMMAG-P': (ok, 'limiting-flux image of the reduced frame made?')}
    eflux = mag = fnu = _NONE
    if ok and exptime is not None and np.isfinite(float(exptime)) and float(exptime) > 0:
        eflux = med / float(exptime)
        if zp is not None:
            mag = float(zp) - 2.5 * np.log10(eflux) - float(ext)
            fnu = float(10.0 ** (-0.4 * (mag - 23.9)))
    w = np.asarray(win if win is not None else [], np.int64).reshape(-1)
    w = np.sort(w[w > 0])                                            # (a tile whose stamp has no sum has no window)
    hdr['LIMNSIG'] = (_nsigma(nsigma) if ok else _NONE, '[sigma] significance of the limit')
    hdr['LIMEFLUX'] = (eflux, '[e-/s] full-frame %s-sigma limiting flux' % ('%g' % _nsigma(nsigma) if ok else 'n'))
    hdr['LIMMAG'] = (mag, '[mag] full-frame limiting magnitude')
    hdr['LIMFNU'] = (fnu, '[microJy] full-frame limiting flux')
    hdr['LIMPFRAC'] = (_frac(frac) if ok else _NONE, 'share of PSF^2 left outside the window')
    hdr['LIMWIN'] = (int(w[(w.size - 1) // 2]) if ok and w.size else _NONE, '[pix] median window side over the sub-images')
    hdr['LIMNPIX'] = (n if ok else _NONE, 'pixels behind LIMEFLUX')
    return hdr
