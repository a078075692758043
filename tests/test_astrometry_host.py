"""Astrometric solution, host side (no GPU): the rules of DESIGN.md 4p as astrometry_ref.py states them, the closed-form TAN[-SIP]
header of blackbox_amd.astrometry against the pixel-to-sky chain it states, what a polynomial on the pointing's tangent plane can
absorb of a true WCS that is not the nominal one, and the plumbing: pointing, arguments, settings, key and column names, and the
switch that is off by default."""
import inspect
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import astrometry_ref as W                                  # noqa: E402
from blackbox_amd import astrometry as AST                  # noqa: E402
from blackbox_amd import catalogs, fitsio, settings         # noqa: E402

SHAPE, PIXSCALE = (240, 480), 0.564


def field(pointing, n=2000, half=0.6, seed=5):
    """sky positions within [half] deg of the pointing in both standard coordinates"""
    rs = np.random.RandomState(seed)
    xi, eta = rs.uniform(-half, half, (2, n))
    return W.sky_of_std(xi, eta, *pointing)


@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_round_trip_sky_standard_sky(pointing):
    ra, dec = field(pointing)
    xi, eta, ok = W.std_of_sky(ra, dec, *pointing)
    assert ok.all()
    for back in (W.sky_of_std, AST.sky_of_std):
        ra2, dec2 = back(xi, eta, *pointing)
        sep = W.separation(ra, dec, ra2, dec2).max()
        print('pointing %s: largest round-trip separation %.3g deg' % (pointing, sep))
        assert sep <= 1e-13 and np.abs(dec2 - dec).max() <= 1e-13
        assert (ra2 >= 0).all() and (ra2 < 360).all()
    if pointing[0] < 1 or pointing[0] > 359:
        assert (ra < 1).any() and (ra > 359).any()               # the field lies on both sides of RA = 0


def test_a_row_beyond_90_degrees_is_not_in_the_field():
    ra0, dec0 = 120.0, -30.0
    ra = np.array([120.0, 120.0 + 89.0, 120.0 + 91.0, 300.0, np.nan, 120.0])
    dec = np.array([-30.0, 0.0, 0.0, 30.0, 0.0, np.inf])
    _, _, ok = W.std_of_sky(ra, dec, ra0, dec0)
    assert ok.tolist() == [True, True, False, False, False, False]
    lst, elig, _ = W.cat_list_ref(ra, dec, np.full(6, 15.0), (ra0, dec0), SHAPE, W.cd0_of(PIXSCALE), 272.0)
    assert elig.tolist() == [True] + [False] * 5                   # 89 deg away is in the field but far outside the margin
    assert lst[3][0] > 0 and (lst[3][1:] == 0).all() and np.isnan(lst[2][1:]).all() and np.isfinite(lst[2][0]).all()


def test_cd0_conventions():
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    assert np.array_equal(cd, W.cd0_of(PIXSCALE, 0.0, 1))
    # north up, east left: +x is west (xi decreases), +y is north
    assert cd[0, 0] < 0 and cd[1, 1] > 0 and cd[0, 1] == 0 and abs(cd[1, 0]) == 0
    assert np.allclose(AST.cd0(PIXSCALE, 30.0, -1), W.cd0_of(PIXSCALE, 30.0, -1), rtol=0, atol=0)
    with pytest.raises(ValueError):
        AST.cd0(PIXSCALE, 0.0, 2)


def truth_of(pointing):
    return lambda x, y: W.true_sky(x, y, SHAPE, pointing, PIXSCALE)


@pytest.mark.parametrize('poldeg', [1, 2])
@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_header_states_the_chain(pointing, poldeg):
    """rule 7 against rule 5: the header, evaluated as a reader would, gives the chain's RA / DEC"""
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    coef, _ = W.fit_truth(SHAPE, pointing, cd, poldeg, truth_of(pointing))
    hdr = AST.wcs_header(coef, SHAPE, poldeg, cd, pointing)
    yy, xx = np.mgrid[0:SHAPE[0]:7, 0:SHAPE[1]:11]
    x, y = xx.ravel() + 0.37, yy.ravel() - 0.21
    ra, dec = W.pix2sky_ref(coef, SHAPE, cd, pointing, x, y)
    ra_h, dec_h = AST.wcs_pix2sky(hdr, x + 1.0, y + 1.0)
    sep = W.separation(ra, dec, ra_h, dec_h).max()
    print('pointing %s degree %d: header against chain %.3g deg' % (pointing, poldeg, sep))
    assert sep <= 1e-12
    ra_m, dec_m = AST.pix2sky_host(coef, SHAPE, cd, pointing, x, y)
    assert W.separation(ra, dec, ra_m, dec_m).max() <= 1e-13
    assert hdr['CTYPE1'][0] == ('RA---TAN-SIP' if poldeg == 2 else 'RA---TAN') and hdr['CTYPE2'][0] == ('DEC--TAN-SIP' if poldeg == 2 else 'DEC--TAN')
    assert (hdr['CRVAL1'][0], hdr['CRVAL2'][0]) == pointing and hdr['RADESYS'][0] == 'ICRS'
    assert ('A_ORDER' in hdr) == (poldeg == 2)
    if poldeg == 2:
        assert hdr['A_ORDER'][0] == hdr['B_ORDER'][0] == 2 and all(k in hdr for k in AST.SIP_KEYS)
    # the derived keys: the truth is 0.3 deg (plus the meridian's convergence towards the tangent point) and 1.0007 x the nominal scale
    assert abs(hdr['A-PSCALE'][0] - PIXSCALE * 1.0007) < 2e-4 and abs(hdr['A-PSCALX'][0] - hdr['A-PSCALY'][0]) < 2e-4
    assert abs(hdr['A-ROT'][0] - 0.5 * (hdr['A-ROTX'][0] + hdr['A-ROTY'][0])) < 1e-12
    assert abs(hdr['A-ROT'][0] - 0.3) < (0.02 if abs(pointing[1]) < 80 else 1.0)


@pytest.mark.parametrize('pointing', W.POINTINGS)
def test_what_the_polynomial_absorbs(pointing):
    """a tangent point 0.01 deg away, 0.3 deg, 1.0007 and 2e-6 / px of quadratic distortion: degree 2 leaves nothing, degree 1 little"""
    cd = AST.cd0(PIXSCALE, 0.0, 1)
    _, r1 = W.fit_truth(SHAPE, pointing, cd, 1, truth_of(pointing))
    coef, r2 = W.fit_truth(SHAPE, pointing, cd, 2, truth_of(pointing))
    X, Y = W.transform(coef, SHAPE, 0.5 * (SHAPE[1] - 1), 0.5 * (SHAPE[0] - 1))
    print('pointing %s: degree 1 leaves %.3g arcsec, degree 2 %.3g arcsec; offset of the virtual grid (%.1f, %.1f) px'
          % (pointing, r1, r2, X - 0.5 * (SHAPE[1] - 1), Y - 0.5 * (SHAPE[0] - 1)))
    assert r2 < 1e-6 and r1 < 0.1
    assert 30 < np.hypot(X - 0.5 * (SHAPE[1] - 1), Y - 0.5 * (SHAPE[0] - 1)) < 100      # the pointing error is an offset: the vote's business


def test_pair_stats_restatement():
    """rule 6 on pairs whose catalogue side is the chain's own sky, then the same catalogue displaced by a known offset"""
    pointing, cd = W.POINTINGS[2], W.cd0_of(PIXSCALE)
    rs = np.random.RandomState(2)
    n = 700
    x, y = rs.uniform(0, SHAPE[1] - 1, n), rs.uniform(0, SHAPE[0] - 1, n)
    iy, ix = np.floor(y + 0.5).astype(np.int32), np.floor(x + 0.5).astype(np.int32)
    a = (iy, ix, np.stack([y - iy, x - ix], axis=1).astype(np.float32))
    coef = np.array([239.5 + 3, 240, 0.5, 0, 0, 0, 119.5 - 2, -0.3, 120, 0, 0, 0], np.float64)
    ra, dec = W.pix2sky_ref(coef, SHAPE, cd, pointing, *W.list_positions(a))
    assert ra.min() < 1 and ra.max() > 359                         # the pairs lie on both sides of RA = 0
    perm = rs.permutation(n)
    items = np.stack([np.arange(n), perm], axis=1)
    cat_ra, cat_dec = np.empty(n), np.empty(n)
    cat_ra[perm], cat_dec[perm] = ra, dec
    kept = rs.uniform(size=n) < 0.8
    items[5] = (-1, -1)
    st = W.pair_stats_ref(items, kept, a, cat_ra, cat_dec, coef, SHAPE, cd, pointing)
    assert st[0] == kept.sum() - int(kept[5]) and np.abs(st[1:]).max() < 1e-9
    moved_ra = (cat_ra - 0.1 / 3600.0 / np.cos(np.radians(cat_dec))) % 360.0
    st = W.pair_stats_ref(items, kept, a, moved_ra, cat_dec + 0.05 / 3600.0, coef, SHAPE, cd, pointing)
    assert abs(st[1] - 0.1) < 1e-8 and abs(st[3] + 0.05) < 1e-8 and st[2] < 1e-8 and st[4] < 1e-8
    dra, _, idx = W.pair_residuals(items, kept, a, moved_ra, cat_dec, coef, SHAPE, cd, pointing)
    assert abs(W.ordered_sum(dra, idx) - dra.sum()) < 1e-9
    assert np.isnan(W.pair_stats_ref(items, np.zeros(n, bool), a, cat_ra, cat_dec, coef, SHAPE, cd, pointing)[1:]).all()


# ---- plumbing ------------------------------------------------------------------------------------------------------
def test_frame_pointing():
    fp = AST.frame_pointing
    assert fp({'RA': 120.5, 'DEC': -30.25}) == (120.5, -30.25)
    assert fp({'RA': (120.5, 'comment'), 'DEC': ('-30.25', '')}) == (120.5, -30.25)
    ra, dec = fp({'RA': '08:02:00.0', 'DEC': '-30:15:00'})
    assert abs(ra - 120.5) < 1e-12 and abs(dec + 30.25) < 1e-12
    assert fp({'RA': '00:00:02.4', 'DEC': '+89:12:00'}) == pytest.approx((0.01, 89.2), abs=1e-12)
    assert fp({'RA': 10.0, 'DEC': 5.0}, ra=359.99, dec=-5.0) == (359.99, -5.0)
    assert fp({'DEC': 5.0}, ra=1.0) == (1.0, 5.0)
    assert fp({'RA': -0.01, 'DEC': 0.0}) == (pytest.approx(359.99), 0.0)
    for bad in ({}, {'RA': 1.0}, {'RA': 'x', 'DEC': 1.0}, {'RA': 1.0, 'DEC': 91.0}, {'RA': float('nan'), 'DEC': 0.0}):
        assert fp(bad) is None


def test_settings_defaults():
    assert settings.astrometry is False and settings.ast_cat is None
    assert settings.ast_cat_cols == ('RA', 'DEC', 'MAG') and settings.ast_cat_max == 2000000
    assert (settings.pixscale, settings.ast_rot, settings.ast_parity, settings.ast_max_shift, settings.ast_bin, settings.ast_poldeg,
            settings.ast_rounds, settings.ast_dist, settings.ast_mag_zp) == (0.564, 0.0, 1, 256.0, 4.0, 2, 3, None, 25.0)


def test_arguments():
    import blackbox
    ap = blackbox.build_parser()
    a = ap.parse_args([])
    assert a.astrometry is None and a.ast_cat is None and a.ast_ra is None and a.ast_dec is None
    kw = blackbox.astrometry_keywords(a, settings, 'ML1')
    assert kw == dict(astrometry=True, ast_poldeg=2, ast_max_shift=256.0, ast_bin=4.0, ast_rounds=3, ast_dist=settings.match_dist_pix, ast_rot=0.0,
                      ast_parity=1, ast_pixscale=0.564, ast_mag_zp=25.0)
    a = ap.parse_args('--astrometry True --ast_cat c.fits --ast_cat_cols ra,dec,phot_g --ast_ra 10.5 --ast_dec -3 --ast_poldeg 1 --ast_max_shift 100 '
                      '--ast_bin 2 --ast_rounds 2 --ast_dist 2.5 --ast_rot 90 --ast_parity -1 --ast_pixscale 0.5 --ast_mag_zp 20'.split())
    assert a.astrometry is True and a.ast_cat == 'c.fits' and a.ast_cat_cols == ('ra', 'dec', 'phot_g') and (a.ast_ra, a.ast_dec) == (10.5, -3.0)
    kw = blackbox.astrometry_keywords(a, settings, 'ML1')
    assert kw == dict(astrometry=True, ast_poldeg=1, ast_max_shift=100.0, ast_bin=2.0, ast_rounds=2, ast_dist=2.5, ast_rot=90.0, ast_parity=-1,
                      ast_pixscale=0.5, ast_mag_zp=20.0)
    assert 'ast_pointing' not in kw and 'ast_catalog' not in kw       # the frame's, and the run's object
    for bad in ('--ast_poldeg 3', '--ast_parity 0', '--ast_cat_cols RA,DEC'):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def fake_reducer(argv):
    import blackbox
    args = blackbox.build_parser().parse_args(argv)
    me = types.SimpleNamespace(args=args, tel='ML1', _load_psf=lambda path: None, ctx=None)
    return blackbox, me


def test_switch_off_the_subtraction_gets_todays_keywords():
    blackbox, me = fake_reducer(['--cat_extract', 'True'])
    sub = blackbox.Reducer._load_subtraction_inputs(me, lambda *a: None)
    assert sorted(sub) == sorted(['psf_new', 'psf_ref', 'ref', 'ref_mask', 'cat_extract', 'trans_extract', 'fratio', 'dx', 'dy', 'ref_is_bkgsub'])
    from blackbox_amd import zogy
    par = inspect.signature(zogy._optimal_subtraction).parameters
    assert par['astrometry'].default is False and par['ast_catalog'].default is None and par['ast_pointing'].default is None
    # switched on without a catalogue: an error before any frame runs
    blackbox, me = fake_reducer(['--cat_extract', 'True', '--astrometry', 'True'])
    with pytest.raises(ValueError, match='ast_cat'):
        blackbox.Reducer._load_subtraction_inputs(me, lambda *a: None)


def test_key_and_column_names(tmp_path):
    hdr = AST.ast_header(None)
    names = ['A-P'] + [k for k, _ in AST.AST_KEYS]
    assert list(hdr) == names and hdr['A-P'][0] is False
    assert all(hdr[k][0] == 'None' for k in names[1:])
    assert not any(k in hdr for k in AST.WCS_KEYS + AST.SIP_KEYS)
    for k in ('A-PSCALE', 'A-PSCALX', 'A-PSCALY', 'A-ROT', 'A-ROTX', 'A-ROTY', 'A-CAT-F', 'A-NAST', 'A-TNAST', 'A-DRA', 'A-DRASTD', 'A-DDEC',
              'A-DDESTD', 'RA-CNTR', 'DEC-CNTR', 'A-PLDG', 'A-NVOTE', 'A-MSHFT', 'A-FLAGS'):
        assert k in hdr and len(k) <= 8
    # the column lists as before, and the new groups behind them only where the table carries them
    assert [c[0] for c in catalogs.COLUMNS['new']] == ['NUMBER', 'X_POS', 'Y_POS', 'E_FLUX_PEAK', 'E_FLUX_OPT', 'E_FLUXERR_OPT', 'SNR_OPT']
    assert [c[0] for c in catalogs.COLUMNS['trans']] == ['NUMBER', 'X_PEAK', 'Y_PEAK', 'SNR_ZOGY', 'E_FLUX_ZOGY', 'E_FLUXERR_ZOGY']
    assert [c[0] for c in catalogs.AST_COLUMNS] == ['RA', 'DEC'] and [c[0] for c in catalogs.AST_TRANS_COLUMNS] == ['RA_PEAK', 'DEC_PEAK']
    assert [c[0] for c in catalogs.AST_TRANSFIT_COLUMNS] == ['RA_PSF_D', 'DEC_PSF_D']
    cat = dict(X_POS=np.array([1.5, 2.5], np.float32), Y_POS=np.array([3.0, 4.0], np.float32), E_FLUX_PEAK=np.ones(2, np.float32),
               E_FLUX_OPT=np.ones(2, np.float32), E_FLUXERR_OPT=np.ones(2, np.float32), SNR_OPT=np.ones(2, np.float32))
    p0, p1 = str(tmp_path / 'a.fits'), str(tmp_path / 'b.fits')
    catalogs.format_cat(cat, p0, 'new')
    assert list(fitsio.read_table(p0)[0]) == [c[0] for c in catalogs.COLUMNS['new']]
    sky = np.array([359.99999999999994, 1.2345678901234567e-5])
    catalogs.format_cat(dict(cat, RA=sky, DEC=-sky), p1, 'new')
    tab = fitsio.read_table(p1)[0]
    assert list(tab) == [c[0] for c in catalogs.COLUMNS['new']] + ['RA', 'DEC']
    assert tab['RA'].dtype == np.float64 and np.array_equal(tab['RA'], sky) and np.array_equal(tab['DEC'], -sky)
    t = [dict(y=3, x=4, scorr=7.0, fpsf=1.0, fpsferr=0.1), dict(y=5, x=6, scorr=8.0, fpsf=1.0, fpsferr=0.1)]
    assert 'RA_PEAK' not in catalogs.transient_table(t)
    for d in t:
        d.update(ra_peak=1.0, dec_peak=2.0)
    tt = catalogs.transient_table(t)
    assert tt['RA_PEAK'].dtype == np.float64 and tt['DEC_PEAK'].tolist() == [2.0, 2.0] and 'RA_PSF_D' not in tt
    catalogs.format_cat(tt, p1, 'trans')
    assert list(fitsio.read_table(p1)[0]) == [c[0] for c in catalogs.COLUMNS['trans']] + ['RA_PEAK', 'DEC_PEAK']


def test_header_cards_keep_the_digits(tmp_path):
    """the solution through a header file: 13 significant digits per card leave less than 1e-9 deg over the toy frame"""
    pointing, cd = W.POINTINGS[2], AST.cd0(PIXSCALE)
    coef, _ = W.fit_truth(SHAPE, pointing, cd, 2, truth_of(pointing))
    hdr = AST.wcs_header(coef, SHAPE, 2, cd, pointing)
    path = str(tmp_path / 'h.fits')
    fitsio.write_header(path, hdr)
    back = fitsio.read_hdus(path, headers_only=True)[0][0]
    x, y = np.array([1.0, 480.0, 1.0, 480.0, 200.3]), np.array([1.0, 1.0, 240.0, 240.0, 100.7])
    sep = W.separation(*AST.wcs_pix2sky(hdr, x, y), *AST.wcs_pix2sky(back, x, y)).max()
    print('through the file: %.3g deg' % sep)
    assert sep <= 1e-9
