"""Astrometric solution on the GPU (bbx_wcs.hip, blackbox_amd/astrometry.py): the three kernels against the float64
numpy restatement of their rules (astrometry_ref.py), the solve against the restatement of the whole chain and against the truth
of a toy scene, the paths on which it must fail without a fault, optimal_subtraction's columns, and the command line.

Bounds.  Offsets of list B: one rounding to float32 of a value below 0.5 (2^-24) plus what the libm calls of device and host may
differ by (1e-9 px).  Sky positions: 1e-10 deg of angular separation (0.36 uas, about 2e3 ulp of 360 deg).  Residual statistics:
1e-12 arcsec against the restatement's sums in the kernel's order over the residuals of the DEVICE's own sky positions (which
isolates the sums from the libm calls; the restatement from scratch is held to the sky positions' bound).  The chain: vote and
pairs equal, T within 1e-12 px at the frame corners against the restated chain on the device's own list B.

Measured on an MI355X: offsets of list B bit-equal; sky positions within 2.5e-14 deg; statistics equal to the same-order sums and
within 5e-11 arcsec of the restatement from scratch; T within 5e-14 .. 8.9e-13 px of the restated chain at the three pointings;
the corners' sky within 0.030 .. 0.063 arcsec of the truth (bound 0.114); tables against the header file 6e-14 deg (bound 1e-7)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
import astrometry_ref as W                      # noqa: E402
import test_align_host as A                     # noqa: E402  (the scene, the chain's restatements, the corner bound)
import test_match_host as H                     # noqa: E402
from blackbox_amd import astrometry as AST      # noqa: E402
from blackbox_amd import reduce as R            # noqa: E402
from blackbox_amd import zogy as G              # noqa: E402
from blackbox_amd._lib import lib               # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SHAPE, PIXSCALE = (A.NY, A.NX), 0.564
SHAPES = ((97, 130), (240, 480))
MARGIN = 256.0 + 16.0


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def dev_list(ctx, lst):
    n = len(lst[0])
    cols = [np.asarray(lst[0], np.int32), np.asarray(lst[1], np.int32), np.asarray(lst[2], F).reshape(n, 2)]
    cols += [np.asarray(t, F) for t in lst[3:5]]
    return tuple(dev(ctx, c) for c in cols)


def host(ctx, *tensors):
    ctx.sync()
    out = [t.cpu().numpy() for t in tensors]
    return out if len(out) > 1 else out[0]


# ---- the kernels -----------------------------------------------------------------------------------------------------
def kernel_catalogue(pointing, shape, n, seed=17):
    """n rows about the pointing, out to twice the margin around the frame (so that some lie outside it); with n >= 100 the first
    rows are the special ones: beyond 90 deg, NaN positions, a NaN magnitude, far outside the margin"""
    rs = np.random.RandomState(seed + n)
    cd = W.cd0_of(PIXSCALE)
    half_x, half_y = 0.5 * shape[1] + 2 * MARGIN, 0.5 * shape[0] + 2 * MARGIN
    dx, dy = rs.uniform(-half_x, half_x, n), rs.uniform(-half_y, half_y, n)
    ra, dec = W.sky_of_std(cd[0, 0] * dx + cd[0, 1] * dy, cd[1, 0] * dx + cd[1, 1] * dy, *pointing)
    mag = rs.uniform(12.0, 20.0, n).astype(F)
    if n >= 100:
        ra[0], dec[0] = (pointing[0] + 180.0) % 360.0, -pointing[1]              # the antipode
        ra[1], dec[1] = (pointing[0] + 100.0) % 360.0, 0.0                       # more than 90 deg away (not for the polar pointing: see the test)
        ra[2] = np.nan
        dec[3] = np.nan
        mag[4] = np.nan
        ra[5], dec[5] = W.sky_of_std(0.0, 0.5, *pointing)                        # 0.5 deg north: 3200 px outside
        mag[6] = np.inf
        ra[7] = np.inf
    return ra, dec, mag


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('n', [0, 1, 1000])
@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_cat_list_meets_the_restatement(ctx, pointing, n, shape):
    ra, dec, mag = kernel_catalogue(pointing, shape, n)
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    want, ok, (x, y) = W.cat_list_ref(ra, dec, mag, pointing, shape, cd, MARGIN)
    # no restated position of an eligible row within 1e-6 px of a half-integer: every integer is compared
    fr = np.abs(np.stack([x[ok], y[ok]]) - np.floor(np.stack([x[ok], y[ok]])) - 0.5)
    assert not fr.size or fr.min() > 1e-6
    cat = AST.AstCatalog(ctx, ra, dec, mag)
    lst, count = AST.cat_list(ctx, cat, pointing, shape, cd, MARGIN)
    ys, xs, off, flux, err, count = host(ctx, *lst, count)
    assert int(count[0]) == int(ok.sum())
    assert np.array_equal(flux > 0, ok)
    assert np.array_equal(ys, want[0]) and np.array_equal(xs, want[1])
    assert np.array_equal(np.isnan(off), np.isnan(want[2])) and np.array_equal(np.isnan(off[:, 0]), ~ok)
    d = np.abs(off[ok].astype(np.float64) - want[2][ok].astype(np.float64))
    print('pointing %s n %d shape %s: %d eligible, offsets differ by at most %.3g px' % (pointing, n, shape, ok.sum(), d.max() if d.size else 0.0))
    assert not d.size or d.max() <= 2.0 ** -24 + 1e-9
    assert (np.abs(flux - want[3]) <= 2 * np.spacing(want[3])).all() and np.array_equal(err, (flux / F(1000.0)).astype(F))
    assert (flux[~ok] == 0).all() and (err[~ok] == 0).all() and (ys[~ok] == 0).all() and (xs[~ok] == 0).all()
    if n >= 100:
        assert not ok[:8].any() and 0.2 * n < ok.sum() < 0.9 * n             # the special rows, and rows outside the margin
        if pointing[0] < 1 or pointing[0] > 359:
            assert (ra[ok] < 1).any() and (ra[ok] > 359).any()                # stars on both sides of RA = 0


def test_cat_list_arguments(ctx):
    cat = AST.AstCatalog(ctx, [1.0], [2.0], [15.0])
    cd = AST.cd0(PIXSCALE)
    n = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    bad = np.zeros(4)
    pd = lambda a: a.ctypes.data_as(lib.bbx_wcs_cat_list.argtypes[8])      # noqa: E731
    assert lib.bbx_wcs_cat_list(None, 0, None, None, 0.0, 0.0, 10, 10, pd(cd.reshape(4)), 1.0, 25.0, None, None, None, None, None, None, None) == -1
    assert lib.bbx_wcs_cat_list(ctx.h, 0, None, None, 0.0, 0.0, 10, 10, pd(bad), 1.0, 25.0, None, None, None, None, None, n.data_ptr(), ctx.stream()) == -1
    assert lib.bbx_wcs_cat_list(ctx.h, 1, None, None, 0.0, 0.0, 10, 10, pd(cd.reshape(4)), 1.0, 25.0, None, None, None, None, None, n.data_ptr(),
                                ctx.stream()) == -1
    assert lib.bbx_wcs_cat_list(ctx.h, 0, None, None, 0.0, 91.0, 10, 10, pd(cd.reshape(4)), 1.0, 25.0, None, None, None, None, None, n.data_ptr(),
                                ctx.stream()) == -1
    with pytest.raises(ValueError):
        AST.AstCatalog(ctx, [1.0, 2.0], [2.0], [15.0])
    with pytest.raises(ValueError):
        AST.AstCatalog(ctx, np.zeros(5), np.zeros(5), np.zeros(5), max_rows=4)
    assert cat.n == 1 and cat.sky.dtype == torch.float64 and cat.mag.dtype == torch.float32


def quad_coef(shape, seed=3):
    """a T of degree 2 near the identity with an offset: what a solve returns"""
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    return np.array([hx - 0.5 + 31.7, 1.0006 * hx, 0.004 * hy, 0.11, -0.07, 0.05, hy - 0.5 - 22.3, -0.0041 * hx, 1.0004 * hy, -0.06, 0.09, 0.12], np.float64)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('n', [0, 1, 1000])
@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_pix2sky_meets_the_restatement(ctx, pointing, n, shape):
    rs = np.random.RandomState(5 + n)
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    coef = quad_coef(shape)
    x, y = rs.uniform(-300, shape[1] + 300, n), rs.uniform(-300, shape[0] + 300, n)
    iy, ix = np.floor(y + 0.5).astype(np.int32), np.floor(x + 0.5).astype(np.int32)
    off = np.stack([y - iy, x - ix], axis=1).astype(F)
    d_coef = dev(ctx, coef)
    worst = 0.0
    for name, kw, (px, py) in (('list', dict(ys=dev(ctx, iy), xs=dev(ctx, ix), off=dev(ctx, off)), W.list_positions((iy, ix, off))),
                               ('peaks', dict(ys=dev(ctx, iy), xs=dev(ctx, ix)), (ix.astype(np.float64), iy.astype(np.float64))),
                               ('positions', dict(pos=dev(ctx, np.stack([x, y], axis=1))), (x, y))):
        sky = host(ctx, AST.pix2sky(ctx, d_coef, shape, cd, pointing, **kw))
        assert sky.shape == (n, 2) and sky.dtype == np.float64
        ra, dec = W.pix2sky_ref(coef, shape, cd, pointing, px, py)
        sep = W.separation(sky[:, 0], sky[:, 1], ra, dec)
        worst = max(worst, sep.max() if n else 0.0)
        assert ((sky[:, 0] >= 0) & (sky[:, 0] < 360)).all()
        assert not n or sep.max() <= 1e-10, name
    print('pointing %s n %d shape %s: largest separation from the restatement %.3g deg' % (pointing, n, shape, worst))
    if n >= 100:
        pos = np.stack([x, y], axis=1)
        pos[3, 0], pos[7, 1] = np.nan, np.inf
        sky = host(ctx, AST.pix2sky(ctx, d_coef, shape, cd, pointing, pos=dev(ctx, pos)))
        assert np.isnan(sky[3]).all() and np.isnan(sky[7]).all() and np.isfinite(np.delete(sky, (3, 7), axis=0)).all()
        if pointing[0] < 1 or pointing[0] > 359:
            assert (sky[np.isfinite(sky[:, 0]), 0] < 1).any() and (sky[np.isfinite(sky[:, 0]), 0] > 359).any()


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('n', [0, 1, 1000])
@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_pair_stats_meets_the_restatement(ctx, pointing, n, shape):
    rs = np.random.RandomState(9 + n)
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    coef = quad_coef(shape)
    x, y = rs.uniform(0, shape[1] - 1, n), rs.uniform(0, shape[0] - 1, n)
    iy, ix = np.floor(y + 0.5).astype(np.int32), np.floor(x + 0.5).astype(np.int32)
    a = (iy, ix, np.stack([y - iy, x - ix], axis=1).astype(F))
    ra, dec = W.pix2sky_ref(coef, shape, cd, pointing, *W.list_positions(a))
    m = n + 7                                                          # the catalogue: the chain's sky displaced, in another order, and rows of no pair
    perm = rs.permutation(m)[:n]
    cat_ra, cat_dec = rs.uniform(0, 360, m), rs.uniform(-80, 80, m)
    cat_dec[perm] = dec + rs.normal(-0.05, 0.08, n) / 3600.0
    cat_ra[perm] = (ra + rs.normal(0.1, 0.12, n) / 3600.0 / np.cos(np.radians(np.clip(cat_dec[perm], -89.99, 89.99)))) % 360.0
    items = np.stack([np.arange(n), perm], axis=1).astype(np.int32)
    kept = (rs.uniform(size=n) < 0.8).astype(np.uint8)
    if n >= 100:
        items[5], items[6], items[7] = (-1, -1), (n, 3), (3, m)            # no pair, and indices past either list
        kept[5:8] = 1
    cat = AST.AstCatalog(ctx, cat_ra, cat_dec, np.zeros(m))
    d_a, d_coef = tuple(dev(ctx, t) for t in a), dev(ctx, coef)
    out = host(ctx, AST.pair_stats(ctx, dev(ctx, items), dev(ctx, kept), d_a, cat, d_coef, shape, cd, pointing))
    sky = host(ctx, AST.pix2sky(ctx, d_coef, shape, cd, pointing, ys=d_a[0], xs=d_a[1], off=d_a[2]))
    want = W.pair_stats_ref(items, kept, a, cat_ra, cat_dec, coef, shape, cd, pointing)
    same = W.pair_stats_ref(items, kept, a, cat_ra, cat_dec, coef, shape, cd, pointing, sky=(sky[:, 0], sky[:, 1]))
    assert out[0] == want[0] == same[0] and (out[5:] == 0).all()
    if want[0] == 0:
        assert np.isnan(out[1:5]).all()
        return
    d_same, d_want = np.abs(out[1:5] - same[1:]).max(), np.abs(out[1:5] - want[1:]).max()
    print('pointing %s n %d shape %s: %d pairs, stats %s arcsec; against the same-order sums %.3g, against the restatement from scratch %.3g arcsec'
          % (pointing, n, shape, out[0], np.round(out[1:5], 5).tolist(), d_same, d_want))
    assert d_same <= 1e-12
    assert d_want <= 1e-10 * 3600.0
    if n >= 100:
        # fit - catalogue: the catalogue was displaced by +0.1 +- 0.12 arcsec in RA cos DEC and -0.05 +- 0.08 in DEC
        assert abs(out[1] + 0.1) < 0.03 and abs(out[3] - 0.05) < 0.02 and abs(out[2] - 0.12) < 0.03 and abs(out[4] - 0.08) < 0.02


# ---- the chain -------------------------------------------------------------------------------------------------------
POINTING_ERR = (30.0, -26.5)                                           # [pix] east, north: 40 px
TRUE = dict(rot=0.2, scale=1.0005, quad=2e-6)


def true_sky_of(pointing):
    off = (POINTING_ERR[0] * PIXSCALE / 3600.0, POINTING_ERR[1] * PIXSCALE / 3600.0)
    return lambda x, y: W.true_sky(x, y, SHAPE, pointing, PIXSCALE, tangent_offset=off, **TRUE)


def catalogue_of(stars, pointing, seed=4, missing=0.15, extra=0.15):
    """the scene's stars through the true WCS, [missing] of them left out (frame stars without a row) and as many rows added at
    random positions (rows without a star)"""
    rs = np.random.RandomState(seed)
    x, y, flux = stars['nx'], stars['ny'], stars['flux']
    keep = rs.uniform(size=x.size) >= missing
    nx_ = int(round(extra * keep.sum()))
    ex, ey = rs.uniform(x.min(), x.max(), nx_), rs.uniform(y.min(), y.max(), nx_)
    ra, dec = true_sky_of(pointing)(np.concatenate([x[keep], ex]), np.concatenate([y[keep], ey]))
    fl = np.concatenate([flux[keep], 10 ** rs.uniform(np.log10(A.FLUX_LO), np.log10(A.FLUX_HI), nx_)])
    mag = (25.0 - 2.5 * np.log10(fl) + rs.normal(0, 0.05, fl.size)).astype(F)
    order = rs.permutation(ra.size)
    return ra[order], dec[order], mag[order]


@pytest.fixture(scope='module')
def scene():
    sc = A.make_align_scene()
    a = H.host_catalog(sc['new'], H.SKY_NEW, sc['psf_new'])
    return sc, a


@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_solve_on_the_scene(ctx, scene, pointing):
    sc, a = scene
    ra, dec, mag = catalogue_of(sc['stars'], pointing)
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    cat = AST.AstCatalog(ctx, ra, dec, mag, name='toy.fits')
    sol = AST.solve(ctx, dev_list(ctx, a), cat, pointing, SHAPE, pixscale=PIXSCALE)
    b_dev = host(ctx, *sol['pending']['b'])
    want = W.solve_ref(a, ra, dec, mag, pointing, SHAPE, cd, poldeg=2, dist=H.DIST, snr_min=H.SNR_MIN, b=b_dev)
    fit = sol['fit']
    chain = A.corner_errors(sol['coef'], want['coef'])
    print('pointing %s: %d rows, %d eligible; flags %d, vote %s, n_used %d (restatement %d), rms (%.4f, %.4f) px; T against the restated chain '
          '%s px' % (pointing, cat.n, sol['n_eligible'], sol['flags'], fit['info'].tolist(), fit['n_used'], want['n_used'], fit['rms_x'],
                     fit['rms_y'], chain.tolist()))
    assert sol['ok'] and sol['flags'] == 0 and want['flags'] == 0
    assert sol['n_eligible'] == want['n_eligible']
    assert np.array_equal(fit['info'], want['vote']['info'])
    items, kept = host(ctx, sol['pending']['items'], sol['pending']['kept'])
    assert np.array_equal(items, want['items']) and np.array_equal(kept.astype(bool), want['kept']) and fit['n_used'] == want['n_used']
    assert (chain <= 1e-12).all()
    assert np.abs(sol['resid'] - want['stats']).max() <= 1e-10 * 3600.0
    # against the truth: the sky at the four corners within the bound the fit's own rms and pair count give, in arcsec
    cx, cy = np.array([0.0, SHAPE[1] - 1.0, 0.0, SHAPE[1] - 1.0]), np.array([0.0, 0.0, SHAPE[0] - 1.0, SHAPE[0] - 1.0])
    got = host(ctx, AST.pix2sky(ctx, sol['d_coef'], SHAPE, cd, pointing, pos=dev(ctx, np.stack([cx, cy], axis=1))))
    err = W.separation(got[:, 0], got[:, 1], *true_sky_of(pointing)(cx, cy)) * 3600.0
    bound = A.corner_bound(fit, 2) * PIXSCALE * TRUE['scale']
    h = sol['header']
    print('    corners against the truth %s arcsec, bound %.4f arcsec; %s' % (np.round(err, 4).tolist(), bound, {
        k: h[k][0] for k in ('A-PSCALE', 'A-ROT', 'A-NAST', 'A-TNAST', 'A-DRA', 'A-DRASTD', 'A-DDEC', 'A-DDESTD', 'A-MSHFT', 'RA-CNTR', 'DEC-CNTR')}))
    assert (err <= bound).all()
    # the header states the device's positions
    hra, hdec = AST.wcs_pix2sky(h, cx + 1.0, cy + 1.0)
    assert W.separation(got[:, 0], got[:, 1], hra, hdec).max() <= 1e-10
    assert h['A-P'][0] is True and h['A-CAT-F'][0] == 'toy.fits' and h['A-PLDG'][0] == 2 and h['CTYPE1'][0] == 'RA---TAN-SIP'
    assert h['A-NAST'][0] == fit['n_used'] and h['A-TNAST'][0] == sol['n_eligible'] and h['A-NVOTE'][0] == fit['info'][0]
    assert abs(h['A-MSHFT'][0] - 40.0) < 2.0 and abs(h['A-PSCALE'][0] - PIXSCALE * TRUE['scale']) < 5e-4
    assert abs(h['A-DRA'][0]) < 3 * h['A-DRASTD'][0] / np.sqrt(fit['n_used']) + 1e-3 and h['A-DRASTD'][0] < 0.1


def test_solve_of_degree_one(ctx, scene):
    sc, a = scene
    pointing = W.POINTINGS[0]
    ra, dec, mag = catalogue_of(sc['stars'], pointing)
    sol = AST.solve(ctx, dev_list(ctx, a), AST.AstCatalog(ctx, ra, dec, mag), pointing, SHAPE, pixscale=PIXSCALE, poldeg=1)
    h = sol['header']
    assert sol['ok'] and h['CTYPE1'][0] == 'RA---TAN' and 'A_ORDER' not in h and h['A-PLDG'][0] == 1 and (sol['coef'][[3, 4, 5, 9, 10, 11]] == 0).all()


# ---- optimal_subtraction ---------------------------------------------------------------------------------------------
BORDER, BOX = 12, 20


def frame_inputs(ctx, sc):
    new = dev(ctx, sc['new'] + F(300.0))
    return new, torch.zeros(new.shape, dtype=torch.uint8, device=ctx.device), dict(
        psf_new=dev(ctx, sc['psf_new']), subimage_size=H.SIZE, subimage_border=BORDER, bkg_boxsize=BOX, cat_extract=True)


def ast_keys_of(hdr):
    return {k: v[0] for k, v in hdr.items() if k.startswith('A-') or k in ('RA-CNTR', 'DEC-CNTR') or k in AST.WCS_KEYS + AST.SIP_KEYS}


@pytest.mark.parametrize('more', [dict(), dict(shapes=True), dict(phot_centroid=True)], ids=['peaks', 'shapes', 'centroid'])
def test_catalogue_columns(ctx, scene, more):
    """RA / DEC of the catalogue are the header's at the very X_POS / Y_POS the table states, and nothing else changes"""
    sc, _ = scene
    pointing = W.POINTINGS[2]
    ra, dec, mag = catalogue_of(sc['stars'], pointing)
    new, mask, kw = frame_inputs(ctx, sc)
    kw.update(more)
    off = G.optimal_subtraction(ctx, new, None, mask, None, psf_ref=None, **kw)
    ctx.sync()
    on = G.optimal_subtraction(ctx, new, None, mask, None, psf_ref=None, astrometry=True, ast_catalog=AST.AstCatalog(ctx, ra, dec, mag, name='c'),
                               ast_pointing=pointing, ast_pixscale=PIXSCALE, **kw)
    ctx.sync()
    h = on['header_new']
    print('%s: %s' % (sorted(more), ast_keys_of(h)))
    assert h['A-P'][0] is True and on['astrometry']['ok'] and 'astrometry' not in off and not ast_keys_of(off['header_new'])
    cat = on['catalog']
    assert list(cat)[:-2] == list(off['catalog']) and list(cat)[-2:] == ['RA', 'DEC'] and cat['RA'].dtype == np.float64
    for k in off['catalog']:
        assert np.array_equal(cat[k], off['catalog'][k], equal_nan=True), k
    assert {k: v for k, v in h.items() if k not in ast_keys_of(h)} == off['header_new']
    hra, hdec = AST.wcs_pix2sky(h, cat['X_POS'].astype(np.float64), cat['Y_POS'].astype(np.float64))
    sep = W.separation(cat['RA'], cat['DEC'], hra, hdec).max()
    print('    %d rows, table against header at X_POS / Y_POS: %.3g deg' % (len(cat['RA']), sep))
    assert len(cat['RA']) > 100 and sep <= 1e-10
    if more:
        assert (cat['X_POS'] != np.round(cat['X_POS'])).any()                 # sub-pixel positions


FAILURES = {'empty': dict(rows=0), 'ten_rows': dict(rows=10), 'wrong_pointing': dict(shift=2 * 256.0), 'wrong_parity': dict(parity=-1),
            'no_pointing': dict(pointing=None), 'no_psf': dict(psf=False)}


@pytest.mark.parametrize('name', sorted(FAILURES))
def test_failures_are_flag_paths(ctx, scene, name):
    """A-P False, every other key 'None', no WCS key, no RA / DEC column, no exception -- and the frame's products as without the switch"""
    sc, _ = scene
    case = FAILURES[name]
    pointing = W.POINTINGS[0]
    ra, dec, mag = catalogue_of(sc['stars'], pointing)
    if 'rows' in case:
        ra, dec, mag = ra[:case['rows']], dec[:case['rows']], mag[:case['rows']]
    given = pointing
    if 'shift' in case:                                                # the header's pointing is off by 2 x ast_max_shift in declination
        given = (pointing[0], pointing[1] + case['shift'] * PIXSCALE / 3600.0)
    if 'pointing' in case:
        given = None
    new, mask, kw = frame_inputs(ctx, sc)
    if case.get('psf') is False:
        kw['psf_new'] = None
    off = G.optimal_subtraction(ctx, new, None, mask, None, psf_ref=None, **kw)
    ctx.sync()
    on = G.optimal_subtraction(ctx, new, None, mask, None, psf_ref=None, astrometry=True, ast_catalog=AST.AstCatalog(ctx, ra, dec, mag),
                               ast_pointing=given, ast_pixscale=PIXSCALE, ast_parity=case.get('parity', 1), **kw)
    ctx.sync()
    h = on['header_new']
    sol = on['astrometry']
    print('%s: flags %s, vote %s' % (name, None if sol is None else sol['flags'], None if sol is None else sol['fit']['info'].tolist()))
    keys = ast_keys_of(h)
    assert keys.pop('A-P') is False and sorted(keys) == sorted(k for k, _ in AST.AST_KEYS) and all(v == 'None' for v in keys.values())
    assert sol is None or (not sol['ok'] and sol['flags'] != 0)
    assert (on['catalog'] is None) == (off['catalog'] is None)
    if on['catalog'] is not None:
        assert list(on['catalog']) == list(off['catalog']) and 'RA' not in on['catalog']
        for k in off['catalog']:
            assert np.array_equal(on['catalog'][k], off['catalog'][k], equal_nan=True), k
    assert {k: v for k, v in h.items() if k not in ast_keys_of(h)} == off['header_new']


def test_transient_columns(ctx, scene):
    """with a reference: RA_PEAK / DEC_PEAK at the integer peaks and, with the fit of P_D, RA_PSF_D / DEC_PSF_D at X_PSF_D / Y_PSF_D"""
    from blackbox_amd import catalogs
    sc, _ = scene
    pointing = W.POINTINGS[1]
    ra, dec, mag = catalogue_of(sc['stars'], pointing)
    rs = np.random.RandomState(8)
    pos = np.array([(60.3, 100.8), (150.6, 333.1), (200.2, 50.4)])
    new_np = sc['new'] + H.render(A.NY, A.NX, pos[:, 0], pos[:, 1], np.full(3, 6000.0), H.FWHM_NEW).astype(F)
    ref_np = (sc['new'] + rs.normal(0, 2.0, sc['new'].shape)).astype(F)                  # the same field without the three
    new, mask, kw = frame_inputs(ctx, dict(sc, new=new_np))
    kw.update(psf_ref=dev(ctx, sc['psf_new']), ref_is_bkgsub=True, ref_bkg_std_mini=np.full((A.NY // BOX, A.NX // BOX), H.SKY_NEW, F),
              trans_psffit=True)
    ref, rmask = dev(ctx, ref_np), torch.zeros(new.shape, dtype=torch.uint8, device=ctx.device)
    psf_new = kw.pop('psf_new')
    psf_ref = kw.pop('psf_ref')
    off = G.optimal_subtraction(ctx, new, ref, mask, rmask, psf_new, psf_ref, **kw)
    ctx.sync()
    on = G.optimal_subtraction(ctx, new, ref, mask, rmask, psf_new, psf_ref, astrometry=True, ast_catalog=AST.AstCatalog(ctx, ra, dec, mag),
                               ast_pointing=pointing, ast_pixscale=PIXSCALE, **kw)
    ctx.sync()
    h = on['header_new']
    assert h['A-P'][0] is True and len(on['transients']) >= 3 and len(on['transients']) == len(off['transients'])
    assert torch.equal(on['D'], off['D']) and on['header_trans'] == off['header_trans']
    for d_on, d_off in zip(on['transients'], off['transients']):
        assert {k: v for k, v in d_on.items() if k not in ('ra_peak', 'dec_peak', 'ra_psf_d', 'dec_psf_d')} == d_off
    tab = catalogs.transient_table(on['transients'])
    assert 'RA_PEAK' not in catalogs.transient_table(off['transients'])
    for (cr, cdec), (cx, cy) in ((('RA_PEAK', 'DEC_PEAK'), ('X_PEAK', 'Y_PEAK')), (('RA_PSF_D', 'DEC_PSF_D'), ('X_PSF_D', 'Y_PSF_D'))):
        hra, hdec = AST.wcs_pix2sky(h, tab[cx].astype(np.float64), tab[cy].astype(np.float64))
        sep = W.separation(tab[cr], tab[cdec], hra, hdec).max()
        print('%s: %d rows, table against header at %s / %s: %.3g deg' % (cr, len(tab[cr]), cx, cy, sep))
        assert tab[cr].dtype == np.float64 and sep <= 1e-10


# ---- pipeline --------------------------------------------------------------------------------------------------------
def test_pipeline_equals_serial_calls(ctx):
    """three frames of one field through a two-lane FramePipeline with astrometry=True: every frame's pointing is read off its own
    header (degrees, sexagesimal, none at all), and its header and catalogue are those of a serial call with that pointing"""
    import bbx_oracle as O
    from blackbox_amd import synth
    from blackbox_amd.pipeline import FramePipeline, HostPool
    tel, ys, xs, nframes, lanes = 'ML1', 124, 124, 3, 2
    size, border, box, S = 124, 8, 31, 11
    case = synth.make_case(ys, xs, 300, tel=tel, os_y=20, os_x=45, n_stars=150, n_sat=2, n_cr=30)
    rs = np.random.RandomState(2)
    flat, bpm = dev(ctx, case['flat']), dev(ctx, case['bpm'])
    coeffs = O.xtalk_coeffs(case['xtalk'])
    raws = [dev(ctx, np.clip(case['raw'].astype(np.int64) + rs.randint(-3, 4, case['raw'].shape), 0, 65535).astype(case['raw'].dtype))
            for _ in range(nframes)]
    geom = R.geometry(raws[0].shape, ys, xs)
    red = [R.reduce_object(ctx, raw, {}, tel, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, ysize_chan=ys, xsize_chan=xs,
                           detect_sats=False)[:2] for raw in raws]
    ny, nx = red[0][0].shape
    nsub = (ny // size) * (nx // size)
    g = np.arange(S) - S // 2
    psf = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2 * 1.5 ** 2))
    psf = dev(ctx, np.repeat((psf / psf.sum()).astype(F)[None], nsub, 0))
    plain = dict(ref=None, ref_mask=None, psf_new=psf, psf_ref=None, cat_extract=True, trans_extract=False, phot_centroid=True,
                 subimage_size=size, subimage_border=border, bkg_boxsize=box)
    stars = G.optimal_subtraction(ctx, red[0][0], new_mask=red[0][1], **plain)['catalog']
    ctx.sync()
    good = stars['SNR_OPT'] > 20
    pointing = (0.01, 89.2)
    off = (-22.0 * PIXSCALE / 3600.0, 17.0 * PIXSCALE / 3600.0)
    ra, dec = W.true_sky(stars['X_POS'][good].astype(np.float64) - 1.0, stars['Y_POS'][good].astype(np.float64) - 1.0, (ny, nx), pointing, PIXSCALE,
                         tangent_offset=off, rot=0.1, scale=1.0004, quad=1e-7)
    cat = AST.AstCatalog(ctx, ra, dec, 25.0 - 2.5 * np.log10(stars['E_FLUX_OPT'][good]), name='field')
    sub_kw = dict(plain, astrometry=True, ast_catalog=cat, ast_pixscale=PIXSCALE)
    headers = [{'RA': 0.01, 'DEC': 89.2}, {'RA': '00:00:02.4', 'DEC': '+89:12:00'}, {}]
    serial = []
    for (data, mask), hdr in zip(red, headers):
        res = G.optimal_subtraction(ctx, data, new_mask=mask, ast_pointing=AST.frame_pointing(hdr), **sub_kw)
        ctx.sync()
        serial.append((res['header_new'], res['catalog']))
    print('serial: %s' % [{k: h[k][0] for k in ('A-P', 'A-NVOTE', 'A-NAST', 'A-MSHFT', 'A-DRASTD')} for h, _ in serial])
    assert [h['A-P'][0] for h, _ in serial] == [True, True, False]
    assert all(abs(h['A-MSHFT'][0] - np.hypot(22.0, 17.0)) < 1.0 and 'RA' in c for h, c in serial[:2]) and 'RA' not in serial[2][1]
    pool = HostPool(4)
    pipe = FramePipeline(ctx, tel, geom, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, pool=pool, depth=3, do_finish=True,
                         keep_outputs=True, lanes=lanes, subtract=sub_kw)
    got = {}

    def done(idx, f):
        assert not f.failed, f.failed
        got[idx] = (f.sub['header_new'], f.sub['catalog'])
    try:
        n = pipe.run([(r, dict(h)) for r, h in zip(raws, headers)], on_done=done)
    finally:
        pipe.close()
    assert n == nframes and sorted(got) == list(range(nframes))
    for k in range(nframes):
        assert got[k][0] == serial[k][0], k
        assert list(got[k][1]) == list(serial[k][1]) and all(np.array_equal(got[k][1][c], serial[k][1][c], equal_nan=True) for c in serial[k][1]), k
    # --ast_ra / --ast_dec over every header: the frame without a pointing is solved too
    pipe = FramePipeline(ctx, tel, geom, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, pool=pool, depth=3, do_finish=True,
                         keep_outputs=True, lanes=lanes, subtract=sub_kw, ast_pointing=pointing)
    got.clear()
    try:
        pipe.run([(raws[2], {})], on_done=done)
    finally:
        pipe.close()
        pool.close()
    assert got[0][0]['A-P'][0] is True and abs(got[0][0]['A-MSHFT'][0] - np.hypot(22.0, 17.0)) < 1.0


# ---- command line ----------------------------------------------------------------------------------------------------
def test_cli(tmp_path, ctx):
    """blackbox.py --image with --astrometry True --ast_cat: the tables' RA / DEC are the file header's at the tables' own positions
    within 1e-7 deg (a card with too few digits would show), and without the switch the products are those of the command without it"""
    import test_gpu_operator as OP
    from blackbox_amd import fitsio, synth
    cli = OP.load_cli()
    case = synth.make_case(OP.YS, OP.XS, 77, tel=OP.TEL, os_y=20, os_x=45, n_stars=150, n_sat=2, n_cr=40)
    raw = str(tmp_path / 'ML1_raw0.fits')
    fitsio.write_image(raw, case['raw'], {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q', 'DATE-OBS': '2024-01-02T03:04:00',
                                          'RA': 359.99, 'DEC': -5.0})
    fitsio.write_image(str(tmp_path / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp_path / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp_path / 'xtalk.dat'), case['xtalk'])
    fitsio.write_image(str(tmp_path / 'psf.fits'), OP.moffat(15, 3.5))
    common = ['--telescope', OP.TEL, '--mflat', str(tmp_path / 'flat.fits'), '--bpm', str(tmp_path / 'bpm.fits'),
              '--crosstalk', str(tmp_path / 'xtalk.dat'), '--ysize_chan', str(OP.YS), '--xsize_chan', str(OP.XS), '--cat_extract', 'True',
              '--phot_centroid', 'True', '--psf_new', str(tmp_path / 'psf.fits'), '--subimage_size', '120', '--subimage_border', '10',
              '--bkg_boxsize', '30', '--image', raw]
    base = 'ML1_20240102_030400_red'
    # first without the switch, and new-only: its catalogue gives the stars the catalogue file is made of
    cli.main(common + ['--red_dir', str(tmp_path / 'stars')])
    stars = fitsio.read_table(str(tmp_path / 'stars' / (base + '_cat.fits')))[0]
    data = fitsio.read_image(str(tmp_path / 'stars' / (base + '.fits')))
    ny, nx = data.shape
    good = stars['SNR_OPT'] > 20
    assert good.sum() > 40
    pointing = (359.99, -5.0)                                           # what the raw header says, in degrees
    off = (25.0 * PIXSCALE / 3600.0, 14.0 * PIXSCALE / 3600.0)
    truth = lambda x, y: W.true_sky(x, y, (ny, nx), pointing, PIXSCALE, tangent_offset=off, rot=0.1, scale=1.0004, quad=1e-6)      # noqa: E731
    x, y = stars['X_POS'][good].astype(np.float64) - 1.0, stars['Y_POS'][good].astype(np.float64) - 1.0
    ra, dec = truth(x, y)
    fitsio.write_table(str(tmp_path / 'gaia.fits'), {'ra': ra, 'dec': dec, 'phot_g': (25.0 - 2.5 * np.log10(stars['E_FLUX_OPT'][good])).astype(F)})
    # the reference: the reduced frame itself without three of its stars, so that they are transient candidates
    rs = np.random.RandomState(3)
    ref = (data - np.median(data)).astype(F)
    order = np.argsort(-stars['SNR_OPT'])
    gone = [k for k in order if 20 < stars['X_POS'][k] < nx - 20 and 20 < stars['Y_POS'][k] < ny - 20][5:8]
    for k in gone:
        yy, xx = int(round(stars['Y_POS'][k] - 1)), int(round(stars['X_POS'][k] - 1))
        ref[yy - 9:yy + 10, xx - 9:xx + 10] = rs.normal(0, 4, (19, 19)).astype(F)
    fitsio.write_image(str(tmp_path / 'ref.fits'), ref)
    sub = ['--trans_extract', 'True', '--ref', str(tmp_path / 'ref.fits'), '--ref_bkgsub', 'True', '--psf_ref', str(tmp_path / 'psf.fits')]
    ast = ['--astrometry', 'True', '--ast_cat', str(tmp_path / 'gaia.fits'), '--ast_cat_cols', 'ra,dec,phot_g', '--ast_pixscale', str(PIXSCALE)]
    cli.main(common + sub + ast + ['--red_dir', str(tmp_path / 'on')])
    h = fitsio.read_hdus(str(tmp_path / 'on' / (base + '_hdr.fits')), headers_only=True)[0][0]
    hi = fitsio.read_hdus(str(tmp_path / 'on' / (base + '.fits')), headers_only=True)[0][0]
    print('command line, switch on:', {k: R.hval(h, k) for k in h if k.startswith('A-') or k in AST.WCS_KEYS + ('RA-CNTR', 'DEC-CNTR')})
    assert bool(R.hval(h, 'A-P')) is True and R.hval(h, 'A-CAT-F') == 'gaia.fits' and R.hval(h, 'CTYPE1') == 'RA---TAN-SIP'
    for k in ('A-P',) + tuple(k for k, _ in AST.AST_KEYS) + AST.WCS_KEYS + AST.SIP_KEYS:
        assert k in h and k in hi and R.hval(h, k) == R.hval(hi, k), k
    assert abs(R.hval(h, 'A-MSHFT') - np.hypot(25.0, 14.0)) < 2.0
    cat = fitsio.read_table(str(tmp_path / 'on' / (base + '_cat.fits')))[0]
    tr = fitsio.read_table(str(tmp_path / 'on' / (base + '_trans.fits')))[0]
    assert cat['RA'].dtype == np.float64 and len(tr['RA_PEAK']) >= 3
    for name, tab, (cr, cdec), (cx, cy) in (('_cat', cat, ('RA', 'DEC'), ('X_POS', 'Y_POS')), ('_trans', tr, ('RA_PEAK', 'DEC_PEAK'), ('X_PEAK', 'Y_PEAK'))):
        hra, hdec = AST.wcs_pix2sky(h, tab[cx].astype(np.float64), tab[cy].astype(np.float64))
        sep = W.separation(tab[cr], tab[cdec], hra, hdec).max()
        print('%s: %d rows, table against the header file at %s / %s: %.3g deg' % (name, len(tab[cr]), cx, cy, sep))
        assert sep <= 1e-7
    # ... and the positions are the sky's: the truth at the catalogue's stars within 0.1 arcsec
    m = np.isin(cat['X_POS'], stars['X_POS'][good]) & np.isin(cat['Y_POS'], stars['Y_POS'][good])
    tra, tdec = truth(cat['X_POS'][m].astype(np.float64) - 1.0, cat['Y_POS'][m].astype(np.float64) - 1.0)
    assert m.sum() > 40 and W.separation(cat['RA'][m], cat['DEC'][m], tra, tdec).max() * 3600.0 < 0.1
    # without the switch: the products of the command without the flag, and none of the keys or columns
    cli.main(common + sub + ['--red_dir', str(tmp_path / 'plain')])
    cli.main(common + sub + ['--red_dir', str(tmp_path / 'off'), '--astrometry', 'False', '--ast_cat', str(tmp_path / 'gaia.fits')])
    for name in (base + '.fits', base + '_cat.fits', base + '_trans.fits', base + '_hdr.fits'):
        for (ha, da), (hb, db) in zip(fitsio.read_hdus(str(tmp_path / 'plain' / name)), fitsio.read_hdus(str(tmp_path / 'off' / name))):
            assert list(ha) == list(hb), name
            assert not [k for k in ha if k.startswith('A-') or k in AST.WCS_KEYS + AST.SIP_KEYS + ('RA-CNTR', 'DEC-CNTR')], name
            for k in ha:
                if k != 'BB-START':
                    assert R.hval(ha, k) == R.hval(hb, k) or (R.hval(ha, k) != R.hval(ha, k) and R.hval(hb, k) != R.hval(hb, k)), (name, k)
            assert (da is None) == (db is None) and (da is None or np.asarray(da).tobytes() == np.asarray(db).tobytes()), name
    assert 'RA' not in fitsio.read_table(str(tmp_path / 'plain' / (base + '_cat.fits')))[0]
    # the image and the tables of the run with the switch differ from those only by the keys and the columns
    on_img, plain_img = fitsio.read_image(str(tmp_path / 'on' / (base + '.fits'))), fitsio.read_image(str(tmp_path / 'plain' / (base + '.fits')))
    assert on_img.tobytes() == plain_img.tobytes()
    plain_cat = fitsio.read_table(str(tmp_path / 'plain' / (base + '_cat.fits')))[0]
    assert list(cat)[:-2] == list(plain_cat) and all(np.array_equal(cat[k], plain_cat[k], equal_nan=True) for k in plain_cat)
