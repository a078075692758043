"""Registration of the reference on the new frame from the two star lists (bbx_align.hip): vote, fit, lattice,
the reference's mask on the new frame's grid and the A-* header keys."""
import numpy as np
import torch

from . import settings
from ._lib import lib, check, fetch, push, ptr as _p, expect as _expect
from .peaks import find_peaks_arrays, win_centroid, window_sigma
from .psfphot import psf_optflux, source_psfs
from .starmatch import match_mutual

# ---- registration of the reference on the new frame from the two star lists (bbx_align.hip) ---------
# [EXT] zogy registers with SWarp and two astrometric solutions; the method and its rules are this project's own, stated in
# float64 numpy by tests/test_align_host.py.  A list is (ys int32, xs int32, off float32 [n, 2], flux float32, err float32) on
# the device; T maps new-frame to reference pixels, coef float64 [12].
ALIGN_PAIR_CAP, ALIGN_NMIN, ALIGN_FAR, ALIGN_CLIP = 8192, 15, 8, 3.0
ALIGN_VOTE_FAILED, ALIGN_FEW_PAIRS, ALIGN_NOT_PD, ALIGN_DET = 1, 2, 4, 8          # the flag word


def _expect_list(lst, name, n_cols=5):
    """a star list crosses the C ABI as bare pointers: every column is checked against the list's length here"""
    n = int(lst[0].numel())
    for t, dt, shape, col in zip(lst[:n_cols], (torch.int32, torch.int32, torch.float32, torch.float32, torch.float32),
                                 ((n,), (n,), (n, 2), (n,), (n,)), ('ys', 'xs', 'off', 'flux', 'err')):
        _expect(t, dt, shape, '{} {}'.format(name, col))
    return n


def align_vote(ctx, a, b, nbright=None, max_shift=None, bin=None, nmin=ALIGN_NMIN, far=ALIGN_FAR, cap=ALIGN_PAIR_CAP):
    """bbx_align_vote of the lists a, b = (ys, xs, off, flux[, ...]) -> device (info int32 [8], coarse float64 [2] = (dy, dx),
    pairs int32 [cap, 2]; (-1, -1) past info[4] pairs).  No host wait"""
    nbright = settings.align_nbright if nbright is None else nbright
    max_shift = settings.align_max_shift if max_shift is None else max_shift
    bin = settings.align_bin if bin is None else bin
    n_a, n_b = _expect_list(a, 'list a', 4), _expect_list(b, 'list b', 4)
    nbytes = int(lib.bbx_align_vote_bytes(int(nbright), float(max_shift), float(bin), int(cap)))
    if nbytes == 0:
        raise ValueError('align_vote: nbright {} (1 .. 2048), cap {} (1 .. 8192), max_shift {} or bin {} out of range'.format(nbright, cap, max_shift, bin))
    dev = ctx.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    coarse = torch.empty(2, dtype=torch.float64, device=dev)
    pairs = torch.empty((int(cap), 2), dtype=torch.int32, device=dev)
    check(lib.bbx_align_vote(ctx.h, n_a, *[_p(t) for t in a[:4]], n_b, *[_p(t) for t in b[:4]], int(nbright), float(max_shift), float(bin),
                             int(nmin), int(far), int(cap), _p(work), nbytes, _p(info), _p(coarse), _p(pairs), ctx.stream()),
          'bbx_align_vote', ctx.h)
    return info, coarse, pairs


def align_fit(ctx, a, b, items, shape, poldeg, snr_min=None, clip=ALIGN_CLIP, nmin=ALIGN_NMIN):
    """bbx_align_fit of the pairs items int32 [N, 2] (index into a, into b; -1: none) of the lists a, b (five columns each);
    shape: the new frame's -> device (coef float64 [12], stats float64 [4] = n_used, rms_x, rms_y, flags; kept uint8 [N])"""
    snr_min = settings.match_snr_min if snr_min is None else snr_min
    if poldeg not in (1, 2):
        raise ValueError('align_fit: degree 1 or 2, got {}'.format(poldeg))
    n_a, n_b = _expect_list(a, 'list a'), _expect_list(b, 'list b')
    N = int(items.shape[0])
    _expect(items, torch.int32, (N, 2), 'items')
    dev = ctx.device
    coef = torch.empty(12, dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    kept = torch.empty(N, dtype=torch.uint8, device=dev)
    check(lib.bbx_align_fit(ctx.h, n_a, *[_p(t) for t in a[:5]], n_b, *[_p(t) for t in b[:5]], N, _p(items), int(shape[0]), int(shape[1]),
                            int(poldeg), float(snr_min), float(clip), int(nmin), _p(coef), _p(stats), _p(kept), ctx.stream()),
          'bbx_align_fit', ctx.h)
    return coef, stats, kept


def align_apply(ctx, b, coef, shape, poldeg):
    """bbx_align_apply: the list b = (ys, xs, off) through the inverse of T (coef: device float64 [12]; shape: the new frame's)
    -> device (ys int32, xs int32, off float32 [n, 2]), not sorted; a source T^-1 sends beyond 1e9 keeps its integers and gets
    a NaN offset (it matches nothing)"""
    if poldeg not in (1, 2):
        raise ValueError('align_apply: degree 1 or 2, got {}'.format(poldeg))
    n = _expect_list(b, 'list b', 3)
    _expect(coef, torch.float64, (12,), 'coef')
    dev = ctx.device
    oys, oxs = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ooff = torch.empty((n, 2), dtype=torch.float32, device=dev)
    check(lib.bbx_align_apply(ctx.h, n, _p(b[0]), _p(b[1]), _p(b[2]), _p(coef), int(shape[0]), int(shape[1]), int(poldeg), _p(oys), _p(oxs),
                              _p(ooff), ctx.stream()), 'bbx_align_apply', ctx.h)
    return oys, oxs, ooff


def align_sort(ys, xs, off):
    """(ys, xs, off) in (y, x) order of the integer peak, as bbx_match_mutual wants it, and the permutation that made it
    (stable: equal peaks keep their list order).  Plumbing: a torch sort of the key y W + x and gathers"""
    if not ys.numel():
        return ys, xs, off, torch.empty(0, dtype=torch.int64, device=ys.device)
    x64, y64 = xs.to(torch.int64), ys.to(torch.int64)
    x0 = x64.min()
    W = x64.max() - x0 + 1
    perm = torch.sort(y64 * W + (x64 - x0), stable=True).indices
    return ys[perm].contiguous(), xs[perm].contiguous(), off[perm].contiguous(), perm


def align_grid_shape(shape, step):
    """nodes of the lattice of a frame: one past the last pixel in both directions (coadd.projection_grid's count)"""
    return -(-(int(shape[0]) + int(step)) // int(step)), -(-(int(shape[1]) + int(step)) // int(step))


def align_grid(ctx, coef, shape, step=32):
    """bbx_align_grid: T at the lattice nodes of the new frame -> device float64 [gny, gnx, 2] = (x, y), what coadd.resample
    and remap_mask take as grid.  No host wait"""
    _expect(coef, torch.float64, (12,), 'coef')
    gny, gnx = align_grid_shape(shape, step)
    grid = torch.empty((gny, gnx, 2), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_align_grid(ctx.h, _p(coef), int(shape[0]), int(shape[1]), int(step), gny, gnx, _p(grid), ctx.stream()), 'bbx_align_grid', ctx.h)
    return grid


def align_grid_host(coef, shape, step=32):
    """the same lattice on the host, float64 numpy [gny, gnx, 2]: for remap_mini, which works there"""
    c = np.asarray(coef, np.float64)
    gny, gnx = align_grid_shape(shape, step)
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    v, u = np.meshgrid((np.arange(gny) * float(step) - hy) / hy, (np.arange(gnx) * float(step) - hx) / hx, indexing='ij')
    b = np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], axis=-1)
    return np.ascontiguousarray(np.stack([b @ c[:6], b @ c[6:12]], axis=-1))


def remap_mask(ctx, mask, in_shape, grid, out_shape, step=32, edge=None):
    """bbx_remap_mask: the mask (uint8 [in_shape] or None) of the reference on the new frame's grid through the lattice [grid]
    (device float64 [gny, gnx, 2]) -> device (mask uint8 [out_shape] with the edge bit where the resampler has no footprint,
    number of such pixels int64 [1]).  No host wait"""
    edge = settings.mask_value['edge'] if edge is None else edge
    in_ny, in_nx = int(in_shape[0]), int(in_shape[1])
    out_ny, out_nx = int(out_shape[0]), int(out_shape[1])
    if mask is not None:
        _expect(mask, torch.uint8, (in_ny, in_nx), 'mask')
    if not torch.is_tensor(grid) or grid.dim() != 3:
        raise ValueError('remap_mask: the lattice as a device tensor [gny, gnx, 2] expected')
    gny, gnx = int(grid.shape[0]), int(grid.shape[1])
    _expect(grid, torch.float64, (gny, gnx, 2), 'grid')
    out = torch.empty((out_ny, out_nx), dtype=torch.uint8, device=ctx.device)
    nedge = torch.empty(1, dtype=torch.int64, device=ctx.device)
    check(lib.bbx_remap_mask(ctx.h, in_ny, in_nx, _p(mask), out_ny, out_nx, _p(grid), gny, gnx, int(step), int(edge), _p(out), _p(nedge),
                             ctx.stream()), 'bbx_remap_mask', ctx.h)
    return out, nedge


class RefStars:
    """The reference's star list ON ITS OWN GRID, for the registration: the peaks of the background-subtracted reference above
    cat_nsigma x the median of its sigma mini image, those on masked pixels dropped, with windowed centroids and PSF-weighted
    fluxes, in (y, x) order on the device.  The PSF plane of a source is the one of its clamped tile (tile_index) among
    sub_psfs [nsy * nsx, S, S]: only the S/N cut and the brightness ranking rest on it.  sigma: the reference's sigma frame
    on its own grid.  Made once per run (host waits) and used while the reference tensor stays the same"""
    builds = 0

    def __init__(self, ctx, ref, sigma, ref_mask, sub_psfs, nsy, nsx, size, cat_nsigma=5.0, sigma_median=None, max_sources=200000,
                 made_of=None):
        rny, rnx = ref.shape
        _expect(ref, torch.float32, (rny, rnx), 'reference')
        _expect(sigma, torch.float32, (rny, rnx), 'reference sigma')
        if ref_mask is not None:
            _expect(ref_mask, torch.uint8, (rny, rnx), 'reference mask')
        nsy, nsx = int(nsy), int(nsx)
        _expect(sub_psfs, torch.float32, (nsy * nsx, sub_psfs.shape[1], sub_psfs.shape[1]), 'PSF stamps')
        # made_of: the tensor the list is kept for, where [ref] is a background-subtracted copy of it made for this call
        self.ref, self.shape = (ref if made_of is None else made_of), (rny, rnx)
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
        if self.n:
            stamps = source_psfs(ctx, None, sub_psfs, ys, xs, nsx, size)
            self.flux, self.err = psf_optflux(ctx, ref, sigma, stamps, ys, xs, v_is_sigma=True)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_psfs), size, nsy, nsx)
        else:
            self.ys = self.xs = torch.empty(0, dtype=torch.int32, device=dev)
            self.flux = self.err = torch.empty(0, dtype=torch.float32, device=dev)
            self.off = torch.empty((0, 2), dtype=torch.float32, device=dev)
        RefStars.builds += 1

    def lists(self):
        return self.ys, self.xs, self.off, self.flux, self.err

    def matches(self, ref):
        return ref is self.ref or (ref.data_ptr() == self.ref.data_ptr() and tuple(ref.shape) == self.shape)


def align_header(fit=None, shape=None, poldeg=None, n_edge=None):
    """the A-* keys of _trans_hdr.fits from the host copy of a registration: fit = dict(coef [12], n_used, rms_x, rms_y, flags,
    info [8]); shape: the new frame's.  A-DX, A-DY: new - ref at the frame centre; A-ROT [deg] and A-SCALE from the linear part
    in pixels.  No fit, or a flag word that is not 0: A-P False and the string 'None', set_qc's default, for the rest"""
    keys = (('A-PLDG', 'degree of the registration polynomial'), ('A-NVOTE', 'votes of the winning offset block'),
            ('A-NRUN', 'votes of the runner-up block'), ('A-NFAR', 'votes of the largest far block'),
            ('A-NPAIR', 'star pairs in the last fit'), ('A-RMSX', '[pix] rms of the fit in x'), ('A-RMSY', '[pix] rms of the fit in y'),
            ('A-DX', '[pix] x offset new - ref at the frame centre'), ('A-DY', '[pix] y offset new - ref at the frame centre'),
            ('A-ROT', '[deg] rotation of ref against new'), ('A-SCALE', 'pixel scale new / ref'),
            ('A-FLAGS', 'flags: 1 vote 2 pairs 4 singular 8 det'), ('A-NEDGE', 'pixels without reference coverage'))
    ok = fit is not None and int(fit['flags']) == 0
    hdr = {'A-P': (bool(ok), 'reference registered from its stars?')}
    if not ok:
        for k, c in keys:
            hdr[k] = ('None', c)
        if fit is not None:
            hdr['A-FLAGS'] = (int(fit['flags']), keys[11][1])
        return hdr
    c = np.asarray(fit['coef'], np.float64)
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    # the linear part in pixels: d(x_ref) / d(x_new) ... ; T(centre) = (c[0], c[6])
    a11, a12, a21, a22 = c[1] / hx, c[2] / hy, c[7] / hx, c[8] / hy
    info = np.asarray(fit['info'])
    vals = (int(poldeg), int(info[0]), int(info[1]), int(info[7]), int(fit['n_used']), float(fit['rms_x']), float(fit['rms_y']),
            float(hx - c[0]), float(hy - c[6]), float(np.degrees(np.arctan2(a21 - a12, a11 + a22))),
            float(np.sqrt(abs(a11 * a22 - a12 * a21))), 0, int(n_edge) if n_edge is not None else 'None')
    for (k, cm), v in zip(keys, vals):
        hdr[k] = (v, cm)
    return hdr


def align_chain(ctx, a, b, shape, poldeg, rounds, dist, snr_min=None, nbright=None, max_shift=None, bin=None):
    """The chain both solves share (the registration of the reference, and astrometry.solve with the catalogue on its virtual
    grid as b): the vote of the lists a, b (five columns each; a sorted by (y, x)), the affine fit of its pairs, [rounds] times
    (b through the inverse of T, sort, bbx_match_mutual within dist, clipped fit of degree poldeg).  Queued on ctx's stream,
    no host wait -> device (info int32 [8], coarse float64 [2], coef float64 [12], stats float64 [4], items int32 [N, 2],
    kept uint8 [N]): the pairs the last fit was given and which of them it kept"""
    n_a = _expect_list(a, 'new list')
    _expect_list(b, 'reference list')
    info, coarse, items = align_vote(ctx, a, b, nbright, max_shift, bin)
    coef, stats, kept = align_fit(ctx, a, b, items, shape, 1, snr_min)
    ar = torch.arange(n_a, dtype=torch.int32, device=ctx.device)
    for _ in range(rounds):
        sy, sx, so, perm = align_sort(*align_apply(ctx, b[:3], coef, shape, poldeg))
        m = match_mutual(ctx, a[:3], (sy, sx, so), dist)
        if perm.numel():
            ib = torch.where(m >= 0, perm[m.clamp(min=0).to(torch.int64)].to(torch.int32), torch.full_like(m, -1))
        else:
            ib = torch.full_like(m, -1)
        items = torch.stack([torch.where(m >= 0, ar, torch.full_like(ar, -1)), ib], dim=1).contiguous()
        coef, stats, kept = align_fit(ctx, a, b, items, shape, poldeg, snr_min)
    return info, coarse, coef, stats, items, kept


def align_reference(ctx, new_lists, ref_stars, shape_new, shape_ref, ref_mask=None, poldeg=None, max_shift=None, bin=None, dist=None,
                    snr_min=None, step=32, rounds=None, nbright=None):
    """The registration of the reference on the new frame: new_lists = the new frame's (ys, xs, off, flux, err), sorted by
    (y, x); ref_stars: a RefStars (or its five columns).  Queued on ctx's stream: the vote, the affine fit of its pairs, [rounds]
    times (the reference's list through the inverse of T, sort, bbx_match_mutual, fit of degree poldeg), the lattice, the
    reference's mask on the new frame's grid; then ONE host wait for coef, stats and info.
    -> dict(grid, mask, coef, header, flags, n_edge, fit); flags != 0: grid and mask are None"""
    poldeg = settings.align_poldeg if poldeg is None else int(poldeg)
    rounds = settings.align_rounds if rounds is None else int(rounds)
    dist = settings.match_dist_pix if dist is None else dist
    if poldeg not in (1, 2):
        raise ValueError('align_reference: degree 1 or 2, got {}'.format(poldeg))
    a = tuple(new_lists)
    b = tuple(ref_stars.lists()) if hasattr(ref_stars, 'lists') else tuple(ref_stars)
    info, coarse, coef, stats, _, _ = align_chain(ctx, a, b, shape_new, poldeg, rounds, dist, snr_min, nbright, max_shift, bin)
    grid = align_grid(ctx, coef, shape_new, step)
    mask, nedge = remap_mask(ctx, ref_mask, shape_ref, grid, shape_new, step)
    h_coef, h_stats, h_info, h_coarse, h_nedge = fetch(ctx, coef, stats, info, coarse, nedge)
    flags = int(h_stats[3]) | int(h_info[5])
    if not np.isfinite(h_coef).all():
        flags |= int(h_stats[3]) or ALIGN_FEW_PAIRS
    fit = dict(coef=h_coef, n_used=int(h_stats[0]), rms_x=float(h_stats[1]), rms_y=float(h_stats[2]), flags=flags, info=h_info, coarse=h_coarse)
    ok = flags == 0
    n_edge = int(h_nedge[0]) if ok else None
    return dict(grid=grid if ok else None, mask=mask if ok else None, coef=h_coef, flags=flags, n_edge=n_edge, fit=fit,
                header=align_header(fit, shape_new, poldeg, n_edge))
