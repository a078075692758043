"""Fake stars (bbx_fake.hip): stars of an asked S/N planted in the background-subtracted new frame just before it is
cut into sub-images (bbx_fake_inject, in place), read back from Scorr / Fpsf / Fpsferr behind the subtraction (bbx_fake_recover) and
matched against the candidate list on the host; the table of `_trans_fakestars.fits` and the T-NFAKE / T-FAKESN / T-FK* keys.  zogy's
own fake stars are not in the reference tree: the rules are this project's (include/bbx.h), parity is unpinned."""
import numpy as np
import torch

from . import _args
from ._lib import lib, check, push, ptr as _p
from .psfphot import psf_poly_terms, tile_index

FAKE_MASKED, FAKE_ON_SOURCE, FAKE_OFF_FRAME, FAKE_NO_PSF, FAKE_NO_FLUX = 1, 2, 4, 8, 16       # FLAGS_IN (include/bbx.h, bbx_fake_inject)
FOUND_PEAK, FOUND_ROW, FOUND_KEPT = 1, 2, 4                           # FOUND bits
FAKE_S2N_MAX = 8                                                      # asked S/N values of one run (T-FKSN1..8)
FAKE_STAT_SNR, FAKE_STAT_NMIN = 10.0, 5                               # the flux statistics: stars of at least this S/N, at least so many
FAKE_COLS = ('NUMBER', 'X_IN', 'Y_IN', 'SNR_IN', 'SNR_SKY_IN', 'E_FLUX_IN', 'E_FLUX_REAL', 'FLAGS_IN', 'X_PEAK', 'Y_PEAK', 'SCORR_OUT',
             'E_FLUX_OUT', 'E_FLUXERR_OUT', 'E_FLUX_OUT_AT', 'FOUND', 'NUMBER_TRANS')


def fake_s2n_list(s2n):
    """the asked S/N values: a number, a sequence or a comma list -> tuple of 1 .. FAKE_S2N_MAX floats"""
    if isinstance(s2n, str):
        s2n = [v for v in s2n.split(',') if v.strip()]
    vals = tuple(float(v) for v in np.atleast_1d(s2n).tolist())
    if not 1 <= len(vals) <= FAKE_S2N_MAX:
        raise ValueError('fake stars: 1 to %d S/N values expected, got %d' % (FAKE_S2N_MAX, len(vals)))
    return vals


def fake_layout(ny, nx, size, nsy, nsx, S, nper, s2n_list, seed):
    """Where the stars go: every sub-image is divided into g x g cells, g = ceil(sqrt(nper)); nper cells are drawn by a seeded
    permutation and take one star each, its pixel uniform in the cell shrunk by m = (S + 1) / 2 + 3 on every side, its sub-pixel
    offset uniform in [-0.5, 0.5).  Centres are therefore at least S + 7 apart in each axis, across sub-images too, and no stamp
    leaves the frame or overlaps another.  Star i asks for s2n_list[i mod n].  A cell smaller than 2 m + 1: ValueError.
    Pure numpy, deterministic per seed.  -> dict(ys, xs int32 [n]; off float32 [n, 2] (dy, dx); s2n float32 [n]; sub int32 [n];
    S, nper, s2n_list, seed)"""
    size, nsy, nsx, S, nper = int(size), int(nsy), int(nsx), int(S), int(nper)
    s2n_list = fake_s2n_list(s2n_list)
    if nper < 1 or S < 1 or not S & 1 or size < 1 or nsy < 1 or nsx < 1 or nsy * size > ny or nsx * size > nx:
        raise ValueError('fake_layout: nper >= 1, S odd, nsy x nsx sub-images of size inside the frame expected')
    g = int(np.ceil(np.sqrt(nper)))
    while g * g < nper:
        g += 1
    cell, m = size // g, (S + 1) // 2 + 3
    if cell < 2 * m + 1:
        raise ValueError('fake_layout: %d stars per sub-image of %d pixels need cells of %d, a stamp of %d needs %d' % (nper, size, cell, S, 2 * m + 1))
    rng = np.random.default_rng(int(seed))
    nsub = nsy * nsx
    # one permutation of the cells per sub-image (row), of which the first nper are taken; then the pixels and the offsets
    cells = rng.permuted(np.broadcast_to(np.arange(g * g), (nsub, g * g)), axis=1)[:, :nper].reshape(-1)
    py, px = rng.integers(0, cell - 2 * m, (2, nsub * nper))
    off = np.clip(rng.uniform(-0.5, 0.5, (nsub * nper, 2)).astype(np.float32), -0.5, 0.5)
    sub = np.repeat(np.arange(nsub, dtype=np.int32), nper)
    ys = ((sub // nsx) * size + (cells // g) * cell + m + py).astype(np.int32)
    xs = ((sub % nsx) * size + (cells % g) * cell + m + px).astype(np.int32)
    s2n = np.asarray(s2n_list, np.float32)[np.arange(nsub * nper) % len(s2n_list)]
    return dict(ys=ys, xs=xs, off=off, s2n=s2n, sub=sub, S=S, nper=nper, s2n_list=s2n_list, seed=int(seed))


def check_apart(ys, xs, S):
    """ValueError unless every two stars are at least S apart (Chebyshev): their stamps must not overlap (bbx_fake_inject)"""
    ys, xs = np.asarray(ys, np.int64).reshape(-1), np.asarray(xs, np.int64).reshape(-1)
    if ys.size < 2:
        return
    # cells of S x S pixels: two stars of one cell overlap; otherwise a star's partners are in the eight cells around its own
    cy, cx = (ys - ys.min()) // S + 1, (xs - xs.min()) // S + 1
    stride = int(cx.max()) + 2
    key = cy * stride + cx
    order = np.argsort(key, kind='stable')
    skey = key[order]
    dup = np.nonzero(skey[1:] == skey[:-1])[0]
    if dup.size:
        raise ValueError('fake stars %d and %d are closer than the stamp size %d: their stamps overlap' % (order[dup[0]], order[dup[0] + 1], S))
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):                     # (each pair once: the cell to the right and the three below)
        nkey = key + dy * stride + dx
        pos = np.minimum(np.searchsorted(skey, nkey), skey.size - 1)
        hit = skey[pos] == nkey
        j = order[pos]
        close = hit & (np.maximum(np.abs(ys - ys[j]), np.abs(xs - xs[j])) < S)
        if close.any():
            i = int(np.nonzero(close)[0][0])
            raise ValueError('fake stars %d and %d are closer than the stamp size %d: their stamps overlap' % (i, int(j[i]), S))


def fake_prepare(ctx, work, rwork, bstd, new_mask, ref_mask, psf_new, sub_pn, layout, nsx, size, clear_half=3, clear_nsigma=5.0, noise=True,
                 seed=0):
    """Everything of fake_inject that can fail before the frame is touched: the argument rules, the stars' distances, the terms or
    plane indices, the uploads and the output tensors -> the prepared call, for fake_launch.  Nothing is written to `work`.  rwork: the reference's background-subtracted frame on the same grid, or None; bstd: the sigma frame of work or a
    MiniImage; new_mask, ref_mask: uint8 frames or None; psf_new: a PSFEx model dict (its terms at the stars' pixels, as
    psf_optflux_centroid forms them) or anything else, and then sub_pn [nsub, S, S], of which each star takes the plane of its
    sub-image."""
    ny, nx = _args.frame(work)
    if rwork is not None:
        _args.frame(rwork, (ny, nx))
    _args.mask(new_mask, (ny, nx))
    _args.mask(ref_mask, (ny, nx))
    sig = _args.sigma_map(bstd, (ny, nx))
    ys, xs = np.asarray(layout['ys'], np.int32), np.asarray(layout['xs'], np.int32)
    n = int(ys.size)
    off, s2n = np.ascontiguousarray(layout['off'], np.float32), np.ascontiguousarray(layout['s2n'], np.float32)
    if xs.size != n or off.shape != (n, 2) or s2n.shape != (n,):
        raise ValueError('fake_inject: ys, xs, s2n [n] and off [n, 2] expected')
    terms = None
    if isinstance(psf_new, dict):
        cube = psf_new['basis'].contiguous()
        terms = psf_poly_terms(xs + 1.0, ys + 1.0, psf_new['polzero'], psf_new['polscal'], psf_new['poldeg'])
        if terms.shape[1] != cube.shape[0]:
            raise ValueError('basis has %d planes, polynomial degree %d needs %d' % (cube.shape[0], psf_new['poldeg'], terms.shape[1]))
    else:
        cube = sub_pn.contiguous()
    if cube.dim() != 3 or cube.dtype != torch.float32 or cube.shape[1] != cube.shape[2]:
        raise ValueError('float32 PSF planes [n, S, S] expected')
    S = int(cube.shape[1])
    check_apart(ys, xs, S)
    if not 0 <= int(clear_half) <= S // 2 or not float(clear_nsigma) >= 0:
        raise ValueError('fake_inject: clear_half in [0, S / 2] and clear_nsigma >= 0 expected')
    dev = ctx.device
    d_ys, d_xs, d_off, d_s2n = push(ctx, ys, xs, off, s2n)
    idx = None
    if terms is not None:
        terms = push(ctx, terms)
    else:
        idx = tile_index(d_ys, d_xs, size, int(cube.shape[0]) // int(nsx), nsx).to(torch.int32)
    flux, real, snr = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    # (the tensors travel with the pointers made of them: nothing the kernel reads may be freed before it is queued)
    keep = (work, rwork, bstd, new_mask, ref_mask, cube, terms, idx, d_ys, d_xs, d_off, d_s2n)
    args = (ny, nx, _p(work), _p(rwork)) + tuple(sig) + (_p(new_mask), _p(ref_mask), S, int(cube.shape[0]), _p(cube), _p(terms), _p(idx), n,
                                                          _p(d_ys), _p(d_xs), _p(d_off), _p(d_s2n), int(clear_half), float(clear_nsigma),
                                                          int(bool(noise)), int(seed) & 0xffffffffffffffff, _p(flux), _p(real), _p(snr), _p(flags))
    return dict(args=args, keep=keep, out=(flux, real, snr, flags), d_peaks=(d_ys, d_xs))


def fake_launch(ctx, prepared):
    """bbx_fake_inject on a prepared call (fake_prepare): from here on the frame is being modified, and an error is the caller's to
    raise, not to survive.  -> device (flux, real, snr_sky float32 [n], flags uint8 [n]), d_peaks = (d_ys, d_xs) int32.  No host wait"""
    check(lib.bbx_fake_inject(ctx.h, *prepared['args'], ctx.stream()), 'bbx_fake_inject', ctx.h)
    return prepared['out'], prepared['d_peaks']


def fake_inject(ctx, work, rwork, bstd, new_mask, ref_mask, psf_new, sub_pn, layout, nsx, size, clear_half=3, clear_nsigma=5.0, noise=True,
                seed=0):
    """bbx_fake_inject: the layout's stars added to the background-subtracted new frame `work` IN PLACE, queued on the frame's
    stream: fake_launch(fake_prepare(...)), whose arguments these are.  Everything that can fail on the host (shapes, the stars'
    distances, the terms) comes before the launch: an exception there leaves the frame untouched.
    -> device (flux, real, snr_sky float32 [n], flags uint8 [n]), d_peaks = (d_ys, d_xs) int32.  No host wait"""
    return fake_launch(ctx, fake_prepare(ctx, work, rwork, bstd, new_mask, ref_mask, psf_new, sub_pn, layout, nsx, size, clear_half=clear_half,
                                         clear_nsigma=clear_nsigma, noise=noise, seed=seed))


def fake_recover(ctx, Scorr, Fpsf, Fpsferr, layout, radius=2, d_peaks=None):
    """bbx_fake_recover: per star the largest finite Scorr within `radius` (<= 4) of its pixel -> device float32 [n, 6] = (dy, dx of the
    peak, Scorr, Fpsf, Fpsferr there, Fpsf at the star's own pixel).  No host wait"""
    ny, nx = _args.frames(Scorr, Fpsf, Fpsferr)
    if not 0 <= int(radius) <= 4:
        raise ValueError('fake_recover: a radius of 0 .. 4 pixels expected')
    n, d_ys, d_xs = _args.peaks(ctx, layout['ys'], layout['xs'], d_peaks)
    out = torch.empty((n, 6), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_fake_recover(ctx.h, ny, nx, _p(Scorr), _p(Fpsf), _p(Fpsferr), n, _p(d_ys), _p(d_xs), int(radius), _p(out), ctx.stream()),
          'bbx_fake_recover', ctx.h)
    return out


def fake_match(transients, layout, radius=2, flags=None):
    """The candidate rows that are fake stars: a row with positive Scorr whose peak lies within `radius` (Chebyshev) of a star's pixel
    belongs to that star (flags given: only to a star that was injected, flags == 0).  -> int32 [len(transients)]: the 1-based star
    index, 0 for a real candidate"""
    radius = int(radius)
    ys, xs = np.asarray(layout['ys'], np.int64).reshape(-1), np.asarray(layout['xs'], np.int64).reshape(-1)
    star = np.arange(1, ys.size + 1)
    if flags is not None:
        keep = np.asarray(flags).reshape(-1) == 0
        ys, xs, star = ys[keep], xs[keep], star[keep]
    out = np.zeros(len(transients), np.int32)
    if not len(transients) or not ys.size:
        return out
    ty, tx = np.array([t['y'] for t in transients], np.int64), np.array([t['x'] for t in transients], np.int64)
    pos = np.array([t['scorr'] > 0 for t in transients], bool)
    # the pixels of every star's window as sorted keys (a pixel of two windows: the first star's); the rows are looked up in them
    d = np.arange(-radius, radius + 1)
    stride = int(max(xs.max(), tx.max())) + radius + 2
    lo = min(int(xs.min()), int(tx.min())) - radius
    wy, wx = (ys[:, None, None] + d[None, :, None]), (xs[:, None, None] + d[None, None, :])
    keys = ((wy * stride) + (wx - lo)).reshape(-1)
    who = np.repeat(star, d.size * d.size)
    order = np.argsort(keys, kind='stable')
    skeys = keys[order]
    tkey = ty * stride + (tx - lo)
    at = np.minimum(np.searchsorted(skeys, tkey, side='left'), skeys.size - 1)
    hit = (skeys[at] == tkey) & pos
    out[hit] = who[order[at[hit]]]
    return out


def fake_table(layout, inject, rec, nsigma, first_rows, final_rows):
    """The table of `_trans_fakestars.fits`.  inject: the host copies of bbx_fake_inject's (flux, real, snr_sky, flags); rec: of
    bbx_fake_recover's array; first_rows: fake_match of the candidate list as the peak search made it, with its Scorr values
    (star index per row, scorr per row); final_rows: the star index per row of the table that is written.
    FOUND: 1 the Scorr peak of the window reaches nsigma, 2 a candidate row matched, 4 that row survived every drop;
    NUMBER_TRANS: the number (1-based) of the star's row in the final table -- of several, the one with the largest Scorr, which
    the table lists first -- or 0"""
    flux, real, snr, flags = (np.asarray(a) for a in inject)
    rec = np.asarray(rec, np.float32).reshape(-1, 6)
    n = int(flags.size)
    ys, xs, off = np.asarray(layout['ys']), np.asarray(layout['xs']), np.asarray(layout['off'], np.float32)
    inj = flags == 0
    found = np.zeros(n, np.int16)
    with np.errstate(invalid='ignore'):
        found[inj & np.isfinite(rec[:, 0]) & (rec[:, 2] >= np.float32(nsigma))] |= FOUND_PEAK
    first = np.asarray(first_rows, np.int64).reshape(-1)
    found[np.unique(first[first > 0]) - 1] |= FOUND_ROW
    number = np.zeros(n, np.int32)
    final = np.asarray(final_rows, np.int64).reshape(-1)
    stars, rows = np.unique(final, return_index=True)                  # (the first row of every star)
    number[stars[stars > 0] - 1] = rows[stars > 0] + 1
    found[number > 0] |= FOUND_KEPT
    peak = np.isfinite(rec[:, 0])
    nan = np.float32('nan')
    return dict(NUMBER=np.arange(1, n + 1, dtype=np.int32),
                X_IN=(xs.astype(np.float32) + np.float32(1)) + off[:, 1], Y_IN=(ys.astype(np.float32) + np.float32(1)) + off[:, 0],
                SNR_IN=np.asarray(layout['s2n'], np.float32), SNR_SKY_IN=snr.astype(np.float32), E_FLUX_IN=flux.astype(np.float32),
                E_FLUX_REAL=real.astype(np.float32), FLAGS_IN=flags.astype(np.int16),
                X_PEAK=np.where(peak, xs + 1 + np.where(peak, rec[:, 1], 0), nan).astype(np.float32),
                Y_PEAK=np.where(peak, ys + 1 + np.where(peak, rec[:, 0], 0), nan).astype(np.float32),
                SCORR_OUT=rec[:, 2].copy(), E_FLUX_OUT=rec[:, 3].copy(), E_FLUXERR_OUT=rec[:, 4].copy(), E_FLUX_OUT_AT=rec[:, 5].copy(),
                FOUND=found, NUMBER_TRANS=number)


def _clipped(v, nsig=3.0, rounds=5):
    """median and population std of v after clipping at nsig about the median, at most `rounds` times"""
    v = np.asarray(v, np.float64)
    for _ in range(rounds):
        med, sd = np.median(v), v.std()
        keep = np.abs(v - med) <= nsig * sd
        if keep.all():
            break
        v = v[keep]
    return float(np.median(v)), float(v.std())


def fake_header(ok, table=None, layout=None, noise=None, radius=None, ntrans_fake=None):
    """the keys of header_trans.  ok False (the stage did not run): T-FKP False, the reference's two keys at their 'nothing was
    injected' values, no others"""
    h = {'T-FKP': (bool(ok), 'fake stars injected and recovered?')}
    if not ok:
        h['T-NFAKE'] = (0, 'number of fake stars added to the new image')
        h['T-FAKESN'] = ('None', 'fake stars: first asked S/N')
        return h
    s2n_list = layout['s2n_list']
    inj = table['FLAGS_IN'] == 0
    h['T-NFAKE'] = (int(inj.sum()), 'number of fake stars added to the new image')
    h['T-FAKESN'] = (float(s2n_list[0]), 'fake stars: first asked S/N')
    h['T-FKNASK'] = (int(inj.size), 'fake stars asked for')
    h['T-FKNREJ'] = (int((~inj).sum()), 'fake stars rejected (FLAGS_IN)')
    h['T-FKSEED'] = (int(layout['seed']), 'fake stars: seed')
    h['T-FKNOIS'] = (bool(noise), 'fake stars: source noise added?')
    h['T-FKRAD'] = (int(radius), '[pix] fake stars: recovery radius')
    h['T-NFKTR'] = (int(ntrans_fake), 'transient candidates that are fake stars')
    k_of = np.arange(inj.size) % len(s2n_list)
    for k, s in enumerate(s2n_list):
        sel = inj & (k_of == k)
        ns = int(sel.sum())
        h['T-FKSN%d' % (k + 1)] = (float(s), 'fake stars: asked S/N %d' % (k + 1))
        h['T-FKN%d' % (k + 1)] = (ns, 'fake stars injected at S/N %d' % (k + 1))
        h['T-FKEF%d' % (k + 1)] = (float(((table['FOUND'][sel] & FOUND_ROW) != 0).mean()) if ns else 'None', 'share found as candidates')
        h['T-FKVT%d' % (k + 1)] = (float(((table['FOUND'][sel] & FOUND_KEPT) != 0).mean()) if ns else 'None', 'share in the final table')
    sel = inj & ((table['FOUND'] & FOUND_PEAK) != 0) & (table['SNR_IN'] >= FAKE_STAT_SNR)
    real, out, err = (table[c][sel].astype(np.float64) for c in ('E_FLUX_REAL', 'E_FLUX_OUT', 'E_FLUXERR_OUT'))
    sel_ok = (real > 0) & (err > 0) & np.isfinite(out)
    real, out, err, snr, sc = real[sel_ok], out[sel_ok], err[sel_ok], table['SNR_IN'][sel][sel_ok].astype(np.float64), \
        table['SCORR_OUT'][sel][sel_ok].astype(np.float64)
    frat = fstd = pull = scrt = 'None'
    if real.size >= FAKE_STAT_NMIN:
        frat, fstd = _clipped(out / real)
        p = (out - real) / err
        pull = float(1.4826 * np.median(np.abs(p - np.median(p))))
        scrt = float(np.median(sc / snr))
    h['T-FKFRAT'] = (frat, 'fake stars: median E_FLUX_OUT / E_FLUX_REAL')
    h['T-FKFSTD'] = (fstd, 'fake stars: sigma (STD) of that ratio')
    h['T-FKPULL'] = (pull, 'fake stars: 1.4826 MAD of the flux pulls')
    h['T-FKSCRT'] = (scrt, 'fake stars: median SCORR_OUT / SNR_IN')
    return h
