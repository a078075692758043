"""CPU: the numpy restatement of bbx_aper_phot (aper_ref.py) against what aperture photometry must give -- the overlap weights
against pi r^2 and against supersampling, a constant frame, a noiseless Moffat star against its analytic encircled energy, the
error model against noise realisations -- and the host plumbing of the stage: flags, settings, switches, columns, header keys,
the library's argument checks."""
import ctypes

import numpy as np
import pytest

import aper_ref as A
import test_match_host as H

F = np.float32
RADII = (0.66, 1.5, 5.0)


def weights_on_grid(r, cy, cx):
    R = int(np.ceil(r + 2.5))
    j = np.arange(-R, R + 1)
    jy, jx = np.meshgrid(j, j, indexing='ij')
    return A.overlap_weights(jy - cy, jx - cx, r)


def test_weights_add_up_to_the_disc():
    rs = np.random.RandomState(1)
    worst = 0.0
    cases = [(r, tuple(rs.uniform(-0.5, 0.5, 2))) for r in (0.3, 0.5, 1 / np.sqrt(2), 1.0, 2.376, 5.4, 18.0, 25.2, 47.9) for _ in range(20)]
    # on a pixel centre, on a corner, on the two edge midpoints: tangent and corner-crossing circles
    cases += [(r, c) for r in (0.5, 1 / np.sqrt(2), 1.0, np.sqrt(2), 1.5) for c in ((0.0, 0.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5))]
    for r, (cy, cx) in cases:
        w = weights_on_grid(r, cy, cx)
        assert w.min() >= 0.0 and w.max() <= 1.0, (r, cy, cx)
        worst = max(worst, abs(w.sum() / (np.pi * r * r) - 1))
    print('sum of the weights against pi r^2: worst %.3g over %d discs' % (worst, len(cases)))
    assert worst <= 1e-12


def test_weights_against_supersampling():
    """64 x 64 point samples per pixel: the arc crosses at most about 3 N of the N^2 sub-cells, so every weight lies within 3 / 64"""
    r, cy, cx, N = 2.376, 0.31, -0.17, 64
    j = np.arange(-5, 6)
    jy, jx = np.meshgrid(j, j, indexing='ij')
    w = A.overlap_weights(jy - cy, jx - cx, r)
    s = (np.arange(N) + 0.5) / N - 0.5
    sy, sx = np.meshgrid(s, s, indexing='ij')
    ss = np.array([[(((y + sy - cy) ** 2 + (x + sx - cx) ** 2) <= r * r).mean() for x in j] for y in j])
    d = np.abs(ss - w).max()
    print('weights against 64 x 64 supersampling: largest difference %.3g (bound %.3g)' % (d, 3 / N))
    assert d <= 3.0 / N
    assert ((w > 0) & (w < 1)).sum() >= 12                           # (the comparison covers crossed pixels)


def run_ref(img, y, x, fwhm, sigma=1.0, mask=None, **kw):
    y, x = np.atleast_1d(np.asarray(y, np.float64)), np.atleast_1d(np.asarray(x, np.float64))
    ys, xs = np.rint(y).astype(np.int32), np.rint(x).astype(np.int32)
    off = np.stack([y - ys, x - xs], axis=1).astype(F)
    sg = np.full(img.shape, sigma, F) if np.isscalar(sigma) else sigma
    return A.aper_phot_ref(img, sg, mask, ys, xs, off, np.array([fwhm], F), max(img.shape), 1, 1, **dict(dict(radii=RADII), **kw))


def test_constant_frame():
    c, fw = 37.5, 3.6
    img = np.full((121, 131), c, F)
    rs = np.random.RandomState(2)
    y, x = 60 + rs.uniform(-0.5, 0.5, 6), 65 + rs.uniform(-0.5, 0.5, 6)
    raw, sub = run_ref(img, y, x, fw, sub_sky=False), run_ref(img, y, x, fw, sub_sky=True)
    area = np.pi * (np.asarray(RADII, F).astype(np.float64) * np.float64(F(fw))) ** 2
    assert not raw['flags'].any() and not sub['flags'].any()
    d_raw, d_sub = np.abs(raw['flux'] / (c * area) - 1).max(), (np.abs(sub['flux']) / (c * area)).max()
    print('constant frame: |F / (c pi r^2) - 1| <= %.3g without the sky, |F| / (c pi r^2) <= %.3g with it' % (d_raw, d_sub))
    assert d_raw <= 1e-12 and d_sub <= 1e-9
    assert np.array_equal(sub['sky'][:, 0], np.full(6, c)) and np.array_equal(sub['sky'][:, 1], np.zeros(6))


def moffat_ee(r, fwhm, beta=H.BETA):
    alpha = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / beta) - 1.0))
    return 1.0 - (1.0 + r * r / alpha ** 2) ** (1.0 - beta)


def moffat_cases():
    """one noiseless point-sampled Moffat star (beta 2.5) per FWHM and phase -> [(fwhm, flux ratios to f EE(r_k))]"""
    rs = np.random.RandomState(3)
    gy, gx = np.mgrid[0:111, 0:111].astype(np.float64)
    out = []
    for fw in (3.0, 3.6, 4.2):
        for _ in range(12):
            y, x = 55 + rs.uniform(-0.5, 0.5), 55 + rs.uniform(-0.5, 0.5)
            img = (1e5 * H.moffat(fw, gy - y, gx - x)).astype(F)
            res = run_ref(img, y, x, fw, sub_sky=False)
            assert res['flags'][0] == 0
            r = np.asarray(RADII, F).astype(np.float64) * np.float64(F(fw))
            out.append((fw, res['flux'][0] / (np.float64(1e5) * moffat_ee(r, fw))))
    return out


def test_moffat_star_against_its_encircled_energy():
    """the 5 x FWHM aperture of a point-sampled Moffat holds f EE(r) within 1e-4; the two small apertures differ from the analytic EE
    through pixelisation alone: printed for the README, nothing is asserted of them"""
    cases = moffat_cases()
    ratio = np.array([c[1] for c in cases])
    worst = np.abs(ratio[:, 2] - 1).max()
    print('Moffat truth, 5 x FWHM: worst |F / (f EE) - 1| = %.3g over %d stars' % (worst, len(cases)))
    for fw in (3.0, 3.6, 4.2):
        sel = np.array([c[0] == fw for c in cases])
        print('  FWHM %.1f: F / (f EE) of the 0.66 and 1.5 x FWHM apertures within [%.4f, %.4f] and [%.4f, %.4f]' %
              (fw, ratio[sel, 0].min(), ratio[sel, 0].max(), ratio[sel, 1].min(), ratio[sel, 1].max()))
    assert worst <= 1e-4


def noise_scene(seed):
    """240 x 480, 32 stars on a 60-pixel grid with random phases, flux 1e4 .. 2e5, sky sigma 14, a pedestal of 3 e-"""
    rs = np.random.RandomState(seed)
    gy, gx = np.meshgrid(30 + 60 * np.arange(4), 30 + 60 * np.arange(8), indexing='ij')
    y, x = gy.ravel() + rs.uniform(-0.5, 0.5, 32), gx.ravel() + rs.uniform(-0.5, 0.5, 32)
    flux = 10 ** rs.uniform(4.0, np.log10(2e5), 32)
    model = H.render(240, 480, y, x, flux, H.FWHM_NEW, half=60) + 3.0
    noisy = model + rs.normal(0, 1, model.shape) * np.sqrt(model + H.SKY_NEW ** 2)
    return y, x, model.astype(F), noisy.astype(F)


def test_errors_describe_the_noise():
    pulls, skyp = [], []
    for seed in range(5):
        y, x, model, noisy = noise_scene(seed)
        clean = run_ref(model, y, x, H.FWHM_NEW, sigma=H.SKY_NEW)
        got = run_ref(noisy, y, x, H.FWHM_NEW, sigma=H.SKY_NEW)
        assert not got['flags'].any() and not clean['flags'].any()
        pulls.append((got['flux'] - clean['flux']) / got['err'])
        skyp.append((got['sky'][:, 0] - clean['sky'][:, 0]) / (got['sky'][:, 1] * np.sqrt(np.pi / (2 * got['sky'][:, 2]))))
    pulls, skyp = np.concatenate(pulls), np.concatenate(skyp)
    rms = np.sqrt((pulls ** 2).mean(axis=0))
    print('noise: largest |pull| per aperture %s, rms %s, largest sky pull %.2f' %
          (np.round(np.abs(pulls).max(axis=0), 2).tolist(), np.round(rms, 2).tolist(), np.abs(skyp).max()))
    assert np.abs(pulls).max() <= 4.5 and np.abs(skyp).max() <= 4.5
    assert (rms >= 0.8).all() and (rms <= 1.2).all()


def test_float32_sums_follow_float64():
    """the float32 twin of the sums: what single precision would cost (the kernel sums in float64)"""
    y, x, model, noisy = noise_scene(0)
    a, b = run_ref(noisy, y, x, H.FWHM_NEW, sigma=H.SKY_NEW), run_ref(noisy, y, x, H.FWHM_NEW, sigma=H.SKY_NEW, dtype=np.float32)
    d = np.abs(b['flux'] - a['flux']) / a['sumabs']
    print('float32 sums against float64: largest |dF| / sum w |D| = %.3g' % d.max())
    assert np.array_equal(a['flags'], b['flags']) and d.max() <= 1e-5


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flags_of_hand_made_cases():
    rs = np.random.RandomState(4)
    img = (rs.normal(0, 5, (160, 160)) + 1e5 * H.moffat(3.6, *np.mgrid[-80:80, -80:80].astype(np.float64))).astype(F)
    fw, c = 3.0, 80
    clean = run_ref(img, c, c, fw)
    assert clean['flags'][0] == 0 and np.isfinite(clean['flux']).all() and clean['sky'][0, 2] > 500
    # 1: no centroid -- the peak alone
    nanoff = A.aper_phot_ref(img, np.ones_like(img), None, [c], [c], np.array([[np.nan, 0.2]], F), np.array([fw], F), 160, 1, 1)
    zero = A.aper_phot_ref(img, np.ones_like(img), None, [c], [c], None, np.array([fw], F), 160, 1, 1)
    assert nanoff['flags'][0] == A.NO_CENTROID and np.array_equal(nanoff['flux'], zero['flux']) and zero['flags'][0] == 0
    # 2: a masked pixel, or a NaN pixel, in the smallest aperture; 16: in the annulus only
    m = np.zeros(img.shape, np.uint8)
    m[c, c + 1] = 1
    hit = run_ref(img, c, c, fw, mask=m)
    assert hit['flags'][0] == A.MASKED and hit['flux'][0, 0] < clean['flux'][0, 0]
    bad = img.copy()
    bad[c + 1, c] = np.nan
    assert run_ref(bad, c, c, fw)['flags'][0] == A.MASKED
    m[:] = 0
    m[c, c + 18] = 4
    ann = run_ref(img, c, c, fw, mask=m)
    assert ann['flags'][0] == A.SKY_CUT and ann['sky'][0, 2] <= clean['sky'][0, 2] - 1
    assert np.allclose(run_ref(img, c, c, fw, mask=m, sub_sky=False)['flux'], run_ref(img, c, c, fw, sub_sky=False)['flux'], rtol=1e-13, atol=0)
    # 4 (and 16): the apertures and the annulus leave the frame
    edge = run_ref(img, 2, c, fw)
    assert edge['flags'][0] == A.OFF_FRAME | A.SKY_CUT
    # 8: the annulus masked down to fewer than sky_nmin pixels -- nothing is subtracted
    gy, gx = np.mgrid[0:160, 0:160]
    d = np.hypot(gy - c, gx - c)
    m[:] = 0
    m[(d >= 14) & (d < 22) & ~((gy == c) & (gx > c))] = 1
    few = run_ref(img, c, c, fw, mask=m)
    raw = run_ref(img, c, c, fw, sub_sky=False)
    assert few['flags'][0] & A.FEW_SKY and few['sky'][0, 2] < 20 and np.isnan(few['sky'][0, :2]).all()
    assert np.array_equal(few['flux'][0, :2], raw['flux'][0, :2])
    # A == 0: the smallest aperture masked entirely
    m[:] = 0
    m[c - 3:c + 4, c - 3:c + 4] = 1
    none = run_ref(img, c, c, fw, mask=m)
    assert np.isnan(none['flux'][0, 0]) and np.isnan(none['err'][0, 0]) and np.isfinite(none['flux'][0, 2]) and none['flags'][0] == A.MASKED
    # 32: too big -- a FWHM whose annulus passes 48 pixels, and one that is no number
    for f in (6.9, np.nan, 0.0, -1.0, np.inf):
        big = run_ref(img, c, c, f)
        assert big['flags'][0] == A.TOO_BIG and np.isnan(big['flux']).all() and np.isnan(big['err']).all(), f
        assert np.isnan(big['sky'][0, :2]).all() and big['sky'][0, 2] == 0
    assert run_ref(img, c, c, 6.8)['flags'][0] == 0                  # r_out = 47.6


# ---- plumbing ---------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_switches():
    from blackbox_amd import settings as S
    import test_cli_entry as CE
    assert S.cat_apphot is False and S.apphot_radii == (0.66, 1.5, 5.0) and S.apphot_sky_inout == (5.0, 7.0)
    assert S.apphot_local_sky is True and S.apphot_sky_nmin == 20
    ap = CE.load_cli().build_parser()
    a = ap.parse_args([])
    assert a.cat_apphot is None and a.apphot_radii is None and a.apphot_local_sky is None        # unset: settings
    a = ap.parse_args(['--cat_apphot', 'True', '--apphot_radii', '1,2', '--apphot_local_sky', 'False'])
    assert a.cat_apphot is True and a.apphot_radii == (1.0, 2.0) and a.apphot_local_sky is False
    with pytest.raises(SystemExit):
        ap.parse_args(['--apphot_radii', 'one,two'])


def test_column_names_and_columns():
    from blackbox_amd import aperphot as AP
    assert AP.aper_column_names() == ['E_FLUX_APER_R0.66xFWHM', 'E_FLUXERR_APER_R0.66xFWHM', 'E_FLUX_APER_R1.5xFWHM', 'E_FLUXERR_APER_R1.5xFWHM',
                                      'E_FLUX_APER_R5xFWHM', 'E_FLUXERR_APER_R5xFWHM', 'BKG_APER', 'BKGSTD_APER', 'NSKY_APER', 'FWHM_APER', 'FLAGS_APER']
    assert AP.aper_column_names((1, 2))[:4] == ['E_FLUX_APER_R1xFWHM', 'E_FLUXERR_APER_R1xFWHM', 'E_FLUX_APER_R2xFWHM', 'E_FLUXERR_APER_R2xFWHM']
    for bad in ((), tuple(range(1, 10)), (1.0, -2.0), (np.nan,)):
        with pytest.raises(ValueError):
            AP.aper_column_names(bad)
    assert (AP.APER_NO_CENTROID, AP.APER_MASKED, AP.APER_OFF_FRAME, AP.APER_FEW_SKY, AP.APER_SKY_CUT, AP.APER_TOO_BIG) == \
        (A.NO_CENTROID, A.MASKED, A.OFF_FRAME, A.FEW_SKY, A.SKY_CUT, A.TOO_BIG) == (1, 2, 4, 8, 16, 32)
    flux, err = np.arange(6, dtype=F).reshape(2, 3), np.arange(6, dtype=F).reshape(2, 3) + 10
    c = AP.aper_columns(flux, err, np.array([[1, 2, 30], [np.nan, np.nan, 4]], F), np.array([0, 8], np.uint8), 4.25)
    assert list(c) == AP.aper_column_names()
    assert c['E_FLUX_APER_R1.5xFWHM'].tolist() == [1, 4] and c['E_FLUXERR_APER_R5xFWHM'].tolist() == [12, 15]
    assert c['NSKY_APER'].tolist() == [30, 4] and c['NSKY_APER'].dtype == np.int32 and c['FWHM_APER'].tolist() == [4.25, 4.25]
    assert c['FLAGS_APER'].dtype == np.uint8 and np.isnan(c['BKG_APER'][1])


def test_format_cat_appends_the_aperture_columns(tmp_path):
    from blackbox_amd import aperphot as AP, catalogs, fitsio
    n = 3
    base = dict(X_POS=np.arange(n, dtype=F) + 1.25, Y_POS=np.arange(n, dtype=F) + 2.5, E_FLUX_PEAK=np.ones(n, F), E_FLUX_OPT=np.ones(n, F),
                E_FLUXERR_OPT=np.ones(n, F), SNR_OPT=np.ones(n, F))
    aper = AP.aper_columns(np.arange(3 * n, dtype=F).reshape(n, 3), np.ones((n, 3), F), np.ones((n, 3), F), np.array([0, 2, 32], np.uint8), 3.5)
    full = dict(base, FLAGS_OPT=np.zeros(n, np.uint8), **aper)
    catalogs.format_cat(full, str(tmp_path / 'a.fits'), 'new')
    cols, _ = fitsio.read_table(str(tmp_path / 'a.fits'))
    assert list(cols) == [c[0] for c in catalogs.COLUMNS['new']] + ['FLAGS_OPT'] + AP.aper_column_names()
    for k in aper:
        assert np.array_equal(cols[k], aper[k]), k
    assert cols['FLAGS_APER'].dtype == np.uint8 and cols['NSKY_APER'].dtype.kind == 'i'
    two = dict(base, **AP.aper_columns(np.ones((n, 2), F), np.ones((n, 2), F), np.ones((n, 3), F), np.zeros(n, np.uint8), 3.5, radii=(1, 2)))
    catalogs.format_cat(two, str(tmp_path / 'b.fits'), 'new')
    assert list(fitsio.read_table(str(tmp_path / 'b.fits'))[0]) == [c[0] for c in catalogs.COLUMNS['new']] + AP.aper_column_names((1, 2))
    catalogs.format_cat(base, str(tmp_path / 'c.fits'), 'new')       # a table without them, and the dummy catalogue: the seven
    catalogs.format_cat(None, str(tmp_path / 'd.fits'), 'new')
    for f in ('c.fits', 'd.fits'):
        assert list(fitsio.read_table(str(tmp_path / f))[0]) == [c[0] for c in catalogs.COLUMNS['new']]


def test_aper_header():
    from blackbox_amd import aperphot as AP, settings as S
    rs = np.random.RandomState(5)
    n = 40
    fo = 10 ** rs.uniform(4, 5, n)
    snr = np.full(n, 50.0)
    snr[:5] = 10.0                                                   # below shape_snr_min
    fl = np.zeros(n, np.uint8)
    fl[5:8] = 2
    flux = np.stack([0.3 * fo, 0.8 * fo, 1.02 * fo], axis=1) * (1 + rs.normal(0, 1e-3, (n, 3)))
    flux[10] *= 5.0                                                  # an outlier among the good ones: clipped
    cols = AP.aper_columns(flux, flux / 50, np.ones((n, 3), F), fl, 4.2)
    h = AP.aper_header(True, 4.2, None, None, None, cols, fo, snr)
    assert list(h) == ['AP-P', 'AP-FWHM', 'AP-NAPER', 'AP-R1', 'AP-R2', 'AP-R3', 'AP-SKYIN', 'AP-SKYOU', 'AP-LSKY', 'AP-NSTAR', 'AP-OPT1',
                       'AP-OPT2', 'AP-OPT3']
    assert all(isinstance(v, tuple) and len(v) == 2 and len(k) <= 8 for k, v in h.items())
    assert h['AP-P'][0] is True and h['AP-FWHM'][0] == 4.2 and h['AP-NAPER'][0] == 3 and h['AP-NSTAR'][0] == 32
    assert (h['AP-R1'][0], h['AP-R2'][0], h['AP-R3'][0], h['AP-SKYIN'][0], h['AP-SKYOU'][0], h['AP-LSKY'][0]) == (0.66, 1.5, 5.0, 5.0, 7.0, True)
    for key, want in (('AP-OPT1', 0.3), ('AP-OPT2', 0.8), ('AP-OPT3', 1.02)):
        assert abs(h[key][0] / want - 1) < 1e-3, key
    assert S.shape_nmin == 15
    few = AP.aper_header(True, 4.2, None, None, False, {k: v[:20] for k, v in cols.items()}, fo[:20], snr[:20])
    assert few['AP-NSTAR'][0] == 12 and [few['AP-OPT%d' % k][0] for k in (1, 2, 3)] == ['None'] * 3 and few['AP-LSKY'][0] is False
    assert AP.aper_header(False) == {'AP-P': (False, 'aperture photometry of the catalogue made?')}
    none = AP.aper_header(True, 4.2, (1, 2), None, None, AP.aper_columns(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0), 4.2, (1, 2)),
                          np.zeros(0), np.zeros(0))
    assert none['AP-NSTAR'][0] == 0 and none['AP-NAPER'][0] == 2 and none['AP-OPT2'][0] == 'None'


def test_wrapper_refuses_wrong_tensors_before_the_library():
    """dtypes, shapes and layouts are refused by the wrapper (a bare pointer with a bad extent would be a device fault): no library
    call is reached, so no GPU is needed"""
    torch = pytest.importorskip('torch')
    from blackbox_amd import aperphot as AP

    class Ctx:
        device, h = 'cpu', None

        def stream(self):
            raise AssertionError('the library was reached')
    D, sg = torch.zeros((40, 50)), torch.ones((40, 50))
    ys = xs = torch.zeros(3, dtype=torch.int32)
    off, fw = torch.zeros((3, 2)), torch.full((4,), 3.0)
    ok = dict(D=D, sigma=sg, mask=None, d_ys=ys, d_xs=xs, d_off=off, d_fwhm=fw, size=25, nsy=2, nsx=2)
    for change in (dict(D=D.double()), dict(D=D.t()), dict(sigma=sg[:, :40]), dict(sigma=sg.double()), dict(mask=torch.zeros((40, 50))),
                   dict(mask=torch.zeros((40, 49), dtype=torch.uint8)), dict(d_ys=ys.long()), dict(d_xs=xs[:2]), dict(d_off=off[:2]),
                   dict(d_off=off.double()), dict(d_fwhm=fw[:3]), dict(d_fwhm=fw.double()), dict(nsy=0), dict(size=0), dict(radii=()),
                   dict(radii=tuple(range(1, 10))), dict(sky_inout=(7.0, 5.0)), dict(sky_inout=(5.0, 5.0)), dict(sky_nmin=0)):
        with pytest.raises(ValueError):
            AP.aper_phot(Ctx(), **dict(ok, **change))


def test_library_rejects_bad_arguments_without_gpu():
    """BBX_ERR_ARG before anything touches the context or the device: the context of the calls below is a block of zeros"""
    from blackbox_amd import _lib
    L = _lib.lib
    fake = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rad = (ctypes.c_float * 9)(0.66, 1.5, 5.0, 6, 7, 8, 9, 10, 11)

    def call(c=ctx, ny=64, nx=64, D=p, sigma=p, mini=None, nsrc=1, ys=p, xs=p, fw=p, size=32, nsy=2, nsx=2, naper=3, radii=rad, sky_in=5.0,
             sky_out=7.0, nmin=20, flux=p, err=p, sky=p, flags=p):
        return L.bbx_aper_phot(c, ny, nx, D, sigma, mini, None, nsrc, ys, xs, None, fw, size, nsy, nsx, naper, radii, sky_in, sky_out, 1, nmin,
                               flux, err, sky, flags, None)
    assert call(c=None) == -1
    assert call(naper=0) == -1 and call(naper=9) == -1 and call(radii=None) == -1
    assert call(sky_in=7.0) == -1 and call(sky_in=8.0) == -1 and call(sky_in=-1.0) == -1 and call(sky_out=float('inf')) == -1
    assert call(radii=(ctypes.c_float * 3)(0.66, 0.0, 5.0)) == -1 and call(radii=(ctypes.c_float * 3)(0.66, float('nan'), 5.0)) == -1
    for name in ('flux', 'err', 'sky', 'flags', 'D', 'ys', 'xs', 'fw'):
        assert call(**{name: None}) == -1, name
    assert call(sigma=None) == -1                                    # neither form of the sigma map ... (both: a mini image is needed)
    assert call(ny=0) == -1 and call(nsrc=-1) == -1 and call(size=0) == -1 and call(nsx=0) == -1 and call(nmin=0) == -1
    assert call(nsrc=0, flux=None, err=None, sky=None, flags=None, D=None, ys=None, xs=None, fw=None) == 0      # nothing to do, nothing launched
