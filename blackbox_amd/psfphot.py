"""PSF stamps from a PSFEx model or per sub-image, and the PSF-weighted optimal photometry at integer peaks (zogy.get_psfoptflux;
bbx_psf_optflux*) or with the PSF shifted to the centroid (bbx_psf_optflux_shift)."""
import numpy as np
import torch
from scipy import ndimage

from . import _args
from ._lib import lib, check, push, ptr as _p
from .zoom import MiniImage


def psf_poly_terms(x, y, polzero, polscal, poldeg):
    """PSFEx polynomial terms of the source positions (pixel coordinates x, y; one
    polynomial group over (x, y)): x' = (x - polzero[0]) / polscal[0], same for y; order
    1, x', x'^2, .., y', x'y', .., y'^2, .. (y power outer, x power inner), float32.
    -> array [nsrc, (poldeg+1)(poldeg+2)/2]"""
    xn = ((np.asarray(x, np.float64) - polzero[0]) / polscal[0]).astype(np.float32)
    yn = ((np.asarray(y, np.float64) - polzero[1]) / polscal[1]).astype(np.float32)
    cols = []
    for j in range(poldeg + 1):
        for i in range(poldeg + 1 - j):
            cols.append((xn ** np.float32(i)) * (yn ** np.float32(j)) if (i or j) else np.ones_like(xn))
    return np.stack(cols, axis=1).astype(np.float32)


def resample_psf_basis(basis, psf_samp):
    """PSFEx tabulates its model every PSF_SAMP image pixels (automatic sampling: usually != 1).  zogy.get_psf_ima
    (buildref.py:3357-3366 passes psf_samp) resamples the model image to image pixels: psf_size =
    ceil(S_config * psf_samp) made odd, scipy.ndimage.zoom by psf_size / S_config [EXT: order 2, mode 'nearest';
    oracle/zogy_core.get_psf_ima].  The resampling is linear, so it is applied once to every basis plane (host,
    ncoef small images) and the per-source contraction (bbx_psf_model) then works on image pixels.
    -> float32 [ncoef, psf_size, psf_size]"""
    basis = np.asarray(basis, np.float64)
    s_cfg = basis.shape[1]
    size = int(np.ceil(s_cfg * float(psf_samp)))
    size += 1 - size % 2
    if size == s_cfg:
        return basis.astype(np.float32)
    out = np.stack([ndimage.zoom(b, size / s_cfg, order=2, mode='nearest') for b in basis])
    if out.shape[1:] != (size, size):
        raise ValueError('PSF resampling gave {} instead of {}'.format(out.shape[1:], (size, size)))
    return out.astype(np.float32)


def psf_model_stamps(ctx, basis, x, y, polzero, polscal, poldeg, normalize=True):
    """PSF stamp of every source from a PSFEx model: basis [ncoef, S, S] float32 device
    tensor (PSF_MASK), positions x, y (host arrays).  The contraction runs on the f32 MFMA
    (bbx_psf_model).  -> device tensor [nsrc, S, S]; normalize: each stamp sums to one"""
    terms = torch.from_numpy(psf_poly_terms(x, y, polzero, polscal, poldeg)).to(ctx.device)
    ncoef, S = basis.shape[0], basis.shape[1]
    if terms.shape[1] != ncoef:
        raise ValueError('basis has %d planes, polynomial degree %d needs %d' % (ncoef, poldeg, terms.shape[1]))
    nsrc = terms.shape[0]
    out = torch.empty((nsrc, S, S), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_model(ctx.h, nsrc, ncoef, S * S, _p(terms), _p(basis.contiguous()), _p(out), ctx.stream()),
          'bbx_psf_model', ctx.h)
    if normalize:
        out /= out.sum(dim=(1, 2), keepdim=True)
    return out


def embed_psfs(ctx, stamps, L):
    """PSF stamps [nsub, S, S] (unit sum, centre at S//2) -> [nsub, L, L] centred on pixel [0,0]"""
    nsub, S, _ = stamps.shape
    out = torch.empty((nsub, L, L), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_embed_psf(ctx.h, nsub, S, L, _p(stamps), _p(out), ctx.stream()), 'bbx_embed_psf', ctx.h)
    return out


def subimage_psfs(ctx, psf, nsy, nsx, size):
    """PSF stamps of the sub-images [nsub, S, S] (unit sum) from either such a tensor, a single
    stamp [S, S], or a PSFEx model dict(basis=[ncoef,S,S] device tensor, polzero, polscal, poldeg)
    evaluated at the sub-image centres on the f32 MFMA (zogy.get_psf_ima at the tile centre)"""
    nsub = nsy * nsx
    if isinstance(psf, dict):
        yc = (np.arange(nsy) + 0.5) * size + 0.5          # FITS pixel coordinates of the tile centres
        xc = (np.arange(nsx) + 0.5) * size + 0.5
        yy, xx = np.meshgrid(yc, xc, indexing='ij')
        return psf_model_stamps(ctx, psf['basis'], xx.ravel(), yy.ravel(), psf['polzero'], psf['polscal'], psf['poldeg'])
    if psf.dim() == 2:
        return psf.unsqueeze(0).expand(nsub, -1, -1).contiguous()
    if psf.shape[0] != nsub:
        raise ValueError('need one PSF stamp per sub-image ({}), got {}'.format(nsub, psf.shape[0]))
    return psf.contiguous()


def tile_index(ys, xs, size, nsy, nsx):
    """index of the sub-image tile (size x size pixels, nsy x nsx tiles) of the integer peaks (ys, xs): numpy arrays or
    tensors.  Clamped as the kernels clamp it (bbx_match.hip, k_win_centroid): min(max(y // size, 0), nsy - 1), likewise x -- a
    peak of a frame that is no multiple of the tile (a reference on its own grid) takes the last tile, not one past the end
    of the stamps.  For a frame of nsy size x nsx size pixels nothing changes"""
    size, nsy, nsx = int(size), int(nsy), int(nsx)
    if nsy < 1 or nsx < 1 or size < 1:
        raise ValueError('tile_index: size, nsy, nsx must be positive, got {} {} {}'.format(size, nsy, nsx))
    if torch.is_tensor(ys):
        return torch.clamp(ys // size, 0, nsy - 1) * nsx + torch.clamp(xs // size, 0, nsx - 1)
    return np.clip(np.asarray(ys) // size, 0, nsy - 1) * nsx + np.clip(np.asarray(xs) // size, 0, nsx - 1)


def source_psfs(ctx, psf, sub_psfs, ys, xs, nsx, size):
    """unit-sum PSF stamp of every source: the PSFEx model at the source position, or the stamp
    of the sub-image the source falls in"""
    if isinstance(psf, dict):
        return psf_model_stamps(ctx, psf['basis'], np.asarray(xs) + 1.0, np.asarray(ys) + 1.0, psf['polzero'],
                                psf['polscal'], psf['poldeg'])
    k = push(ctx, tile_index(np.asarray(ys), np.asarray(xs), size, int(sub_psfs.shape[0]) // int(nsx), nsx).astype(np.int64))
    return sub_psfs.index_select(0, k).contiguous()


def _source_sigma(ctx, sigma, shape, ys, xs):
    """the background sigma at the integer peaks (host arrays): a number, a frame, a mini image (a small 2-D tensor or array: the
    value of the box the peak falls in) or a MiniImage (its frame is made) -> device float32 [n]"""
    ny, nx = shape
    n = len(ys)
    if isinstance(sigma, MiniImage):
        sigma = sigma.frame(ctx)
    if np.isscalar(sigma):
        return torch.full((n,), float(sigma), dtype=torch.float32, device=ctx.device)
    if not torch.is_tensor(sigma):
        sigma = push(ctx, np.ascontiguousarray(sigma, np.float32))
    if sigma.dim() != 2:
        raise ValueError('sigma: a number, a frame, a mini image or a MiniImage expected')
    if tuple(sigma.shape) == (ny, nx):
        iy, ix = ys, xs
    else:
        by, bx = -(-ny // sigma.shape[0]), -(-nx // sigma.shape[1])
        iy, ix = np.minimum(np.asarray(ys) // by, sigma.shape[0] - 1), np.minimum(np.asarray(xs) // bx, sigma.shape[1] - 1)
    d_iy, d_ix = push(ctx, np.asarray(iy, np.int64), np.asarray(ix, np.int64)) if n else (torch.empty(0, dtype=torch.int64, device=ctx.device),) * 2
    return sigma[d_iy, d_ix].to(torch.float32).contiguous()


def psf_optflux(ctx, D, V, psfs, ys, xs, v_is_sigma=False):
    """zogy.get_psfoptflux at integer positions -> (flux, fluxerr) float32 device tensors; with v_is_sigma
    V is the sigma image of the background-subtracted frame D -- a frame, or a MiniImage read at the stamp pixels --
    and the variance max(D, 0) + sigma^2 is formed at the stamp pixels only"""
    nsrc, S, _ = psfs.shape
    dev = ctx.device
    d_ys, d_xs = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
    flux = torch.empty(nsrc, dtype=torch.float32, device=dev)
    err = torch.empty(nsrc, dtype=torch.float32, device=dev)
    ny, nx = D.shape
    if isinstance(V, MiniImage):
        check(lib.bbx_psf_optflux_mini(ctx.h, ny, nx, _p(D), V.ref(), _p(psfs), S, nsrc, _p(d_ys), _p(d_xs), _p(flux), _p(err), ctx.stream()),
              'bbx_psf_optflux_mini', ctx.h)
        return flux, err
    fn = lib.bbx_psf_optflux_sigma if v_is_sigma else lib.bbx_psf_optflux
    check(fn(ctx.h, ny, nx, _p(D), _p(V), _p(psfs), S, nsrc, _p(d_ys), _p(d_xs), _p(flux), _p(err), ctx.stream()), 'bbx_psf_optflux', ctx.h)
    return flux, err


PHOT_NO_CENTROID, PHOT_MASKED, PHOT_NO_SUM = 1, 2, 4                # FLAGS_OPT bits (include/bbx.h, bbx_psf_optflux_shift)


def psf_optflux_centroid(ctx, D, sigma, psf, sub_psfs, ys, xs, d_off, mask, nsx, size, d_peaks=None):
    """bbx_psf_optflux_shift: the photometry of psf_optflux(source_psfs(...)) with every source's PSF shifted to its centroid
    d_off [n, 2] (win_centroid: relative to the integer peak; device float32) inside the kernel -- no stamp is written.
    psf: a PSFEx model dict (its terms at the integer peaks, as source_psfs) or anything else, and then sub_psfs [nsub, S, S],
    of which each source takes the plane of its sub-image; sigma: the sigma frame of D or a MiniImage; mask: uint8 frame or
    None, its pixels are left out of the sums; ys, xs: host arrays; d_peaks: (d_ys, d_xs), the same as int32 device tensors
    where the caller has them.
    -> device (flux float32 [n], err float32 [n], flags uint8 [n]: PHOT_NO_CENTROID | PHOT_MASKED | PHOT_NO_SUM).  No host wait"""
    ny, nx = _args.frame(D)
    _args.mask(mask, (ny, nx))
    dev = ctx.device
    n, d_ys, d_xs = _args.peaks(ctx, ys, xs, d_peaks)
    if d_off.dtype != torch.float32 or tuple(d_off.shape) != (n, 2) or not d_off.is_contiguous():
        raise ValueError('contiguous float32 offsets [n, 2] expected')
    terms = idx = None
    if isinstance(psf, dict):
        cube = psf['basis'].contiguous()
        terms = torch.from_numpy(psf_poly_terms(np.asarray(xs) + 1.0, np.asarray(ys) + 1.0, psf['polzero'], psf['polscal'], psf['poldeg'])).to(dev)
        if terms.shape[1] != cube.shape[0]:
            raise ValueError('basis has %d planes, polynomial degree %d needs %d' % (cube.shape[0], psf['poldeg'], terms.shape[1]))
    else:
        cube = sub_psfs.contiguous()
        idx = tile_index(d_ys, d_xs, size, int(cube.shape[0]) // int(nsx), nsx).to(torch.int32)
    if cube.dim() != 3 or cube.dtype != torch.float32 or cube.shape[1] != cube.shape[2]:
        raise ValueError('float32 PSF planes [n, S, S] expected')
    sig = _args.sigma_map(sigma, (ny, nx))
    flux = torch.empty(n, dtype=torch.float32, device=dev)
    err = torch.empty(n, dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib.bbx_psf_optflux_shift(ctx.h, ny, nx, _p(D), *sig,
                                    _p(mask) if mask is not None else None, int(cube.shape[1]), int(cube.shape[0]), _p(cube), _p(terms), _p(idx),
                                    n, _p(d_ys), _p(d_xs), _p(d_off), _p(flux), _p(err), _p(flags), ctx.stream()), 'bbx_psf_optflux_shift', ctx.h)
    return flux, err, flags
