"""The candidate table's host functions (blackbox_amd/transients.py: candidate_rows, sky_columns, pd_columns, shapefit_columns,
drop_edge_rows, vet_rows) on three synthetic candidates: every key and value, and the rows that leave with the index lists
their thumbnails are cut by.  Numpy arrays and lists of dicts only: nothing here needs a device."""
import numpy as np

from blackbox_amd import transients as T

F = np.float32
YS, XS = np.array([5, 17, 40], np.int32), np.array([9, 3, 77], np.int32)
SCORR = np.array([7.5, -6.25, 12.0], F)
FE = np.array([[100.0, -50.0, 300.0], [10.0, 5.0, 20.0]], F)


def rows():
    return T.candidate_rows(YS, XS, SCORR, FE)


def test_candidate_rows():
    got = rows()
    assert got == [dict(y=5, x=9, scorr=7.5, fpsf=100.0, fpsferr=10.0), dict(y=17, x=3, scorr=-6.25, fpsf=-50.0, fpsferr=5.0),
                   dict(y=40, x=77, scorr=12.0, fpsf=300.0, fpsferr=20.0)]
    assert [list(d) for d in got] == [['y', 'x', 'scorr', 'fpsf', 'fpsferr']] * 3
    assert all(type(d['y']) is int and type(d['scorr']) is float for d in got)


def test_sky_columns_of_the_peaks_and_of_the_fitted_positions():
    sky = np.array([[10.0, -1.0], [10.5, -1.5], [11.0, -2.0], [20.0, 1.0], [20.5, 1.5], [21.0, 2.0]])
    r = rows()
    T.sky_columns(r, sky[:3])                                        # n rows: the peaks only
    assert [list(d)[5:] for d in r] == [['ra_peak', 'dec_peak']] * 3
    assert [(d['ra_peak'], d['dec_peak']) for d in r] == [(10.0, -1.0), (10.5, -1.5), (11.0, -2.0)]
    r = rows()
    T.sky_columns(r, sky)                                            # 2 n rows: the fitted positions follow
    assert [list(d)[5:] for d in r] == [['ra_peak', 'dec_peak', 'ra_psf_d', 'dec_psf_d']] * 3
    assert [(d['ra_peak'], d['dec_peak'], d['ra_psf_d'], d['dec_psf_d']) for d in r] == \
        [(10.0, -1.0, 20.0, 1.0), (10.5, -1.5, 20.5, 1.5), (11.0, -2.0, 21.0, 2.0)]
    assert all(type(v) is float for d in r for v in list(d.values())[5:])


def test_pd_columns():
    # six planes of n: flux, error, dy, dx, chi2, flags; then the fold of two sub-images
    planes = np.array([[1000.0, 2000.0, 3000.0], [11.0, 12.0, 13.0], [0.25, -0.5, 0.0], [-0.125, 0.75, 1.5], [0.9, 1.1, 30.0], [0, 1, 4]], F)
    tf = np.concatenate([planes.reshape(-1), np.array([0.001, 0.02], F)])
    r = rows()
    fold = T.pd_columns(r, tf)
    assert np.array_equal(fold, np.array([0.001, 0.02], F))
    assert [list(d)[5:] for d in r] == [['y_psf_d', 'x_psf_d', 'flux_psf_d', 'fluxerr_psf_d', 'chi2_psf_d', 'flags_psf_d']] * 3
    assert [d['y_psf_d'] for d in r] == [5.25, 16.5, 40.0] and [d['x_psf_d'] for d in r] == [8.875, 3.75, 78.5]
    assert [d['flux_psf_d'] for d in r] == [1000.0, 2000.0, 3000.0] and [d['fluxerr_psf_d'] for d in r] == [11.0, 12.0, 13.0]
    assert [d['chi2_psf_d'] for d in r] == [float(F(0.9)), float(F(1.1)), 30.0] and [d['flags_psf_d'] for d in r] == [0, 1, 4]
    assert all(type(d['flags_psf_d']) is int and type(d['y_psf_d']) is float for d in r)


def shape_vector():
    """two models x seven planes of n (dy, dx, yerr, xerr, fwhm, elongation, chi2), then two flag planes: the value of plane p of model m
    at row i is 100 m + 10 p + i + 0.5 (the offsets 1/8 of that, so that they stay small and exact)"""
    planes = np.zeros((2, 7, 3), F)
    for m in range(2):
        for p in range(7):
            for i in range(3):
                planes[m, p, i] = (100 * m + 10 * p + i + 0.5) * (0.125 if p < 2 else 1.0)
    flags = np.array([[0, 4, 8], [1, 0, 4]], F)
    return np.concatenate([planes.reshape(-1), flags.reshape(-1)]), planes, flags


def test_shapefit_columns():
    ts, planes, flags = shape_vector()
    r = rows()
    T.shapefit_columns(r, ts)
    names = ['x_%s_d', 'xerr_%s_d', 'y_%s_d', 'yerr_%s_d', 'fwhm_%s_d', 'elong_%s_d', 'chi2_%s_d', 'flags_%s_d']
    assert [list(d)[5:] for d in r] == [[n % 'gauss' for n in names] + [n % 'moffat' for n in names]] * 3        # the sixteen keys
    for m, name in enumerate(('gauss', 'moffat')):
        for i, d in enumerate(r):
            assert d['y_%s_d' % name] == float(YS[i]) + float(planes[m, 0, i]) and d['x_%s_d' % name] == float(XS[i]) + float(planes[m, 1, i])
            assert d['yerr_%s_d' % name] == float(planes[m, 2, i]) and d['xerr_%s_d' % name] == float(planes[m, 3, i])
            assert d['fwhm_%s_d' % name] == float(planes[m, 4, i]) and d['elong_%s_d' % name] == float(planes[m, 5, i])
            assert d['chi2_%s_d' % name] == float(planes[m, 6, i])
            assert d['flags_%s_d' % name] == int(flags[m, i]) and type(d['flags_%s_d' % name]) is int
    assert r[2]['y_moffat_d'] == 40 + 102.5 * 0.125 and r[1]['fwhm_gauss_d'] == 41.5 and r[0]['chi2_moffat_d'] == 160.5


def test_drop_edge_rows():
    r = rows()
    kept, keep = T.drop_edge_rows(r, np.array([0.0, 16.0, 0.0], F))
    assert keep == [0, 2] and kept == [r[0], r[2]] and kept[1] is r[2]
    kept, keep = T.drop_edge_rows(r, np.zeros(3, F))
    assert keep == [0, 1, 2] and kept == r
    kept, keep = T.drop_edge_rows(r, np.full(3, 16.0, F))
    assert keep == [] and kept == []


def vetted_rows():
    r = rows()
    for d, chi2, fl, fw, el, gfl in zip(r, (0.9, 1.1, 30.0), (0, T.TRANS_NO_FIT, 0), (3.0, 3.5, 9.0), (1.1, 1.2, 1.3), (0, 0, 0)):
        d.update(chi2_psf_d=chi2, flags_psf_d=fl, fwhm_gauss_d=fw, elong_gauss_d=el, flags_gauss_d=gfl)
    return r


def test_vet_rows():
    r = vetted_rows()
    # no bound given, or none that applies (the chi2 bound needs the fit of P_D, the Gauss bounds the shape fits): nothing is dropped
    assert T.vet_rows(r, True, True) == (r, None)
    assert T.vet_rows(r, False, True, chi2_max=2.0) == (r, None)
    assert T.vet_rows(r, True, False, fwhm_gauss_max=5.0, elong_gauss_max=1.0, fwhm_gauss_min=8.0) == (r, None)
    # chi2: row 1 has no fit, row 2 is above the bound
    kept, keep = T.vet_rows(r, True, False, chi2_max=2)
    assert keep == [0] and kept == [r[0]]
    # the Gauss bounds alone
    kept, keep = T.vet_rows(r, False, True, chi2_max=2.0, fwhm_gauss_max=5.0)
    assert keep == [0, 1] and kept == [r[0], r[1]]
    kept, keep = T.vet_rows(r, False, True, fwhm_gauss_min=3.2, elong_gauss_max=1.25)
    assert keep == [1] and kept == [r[1]]
    # both: what vet_transients gives with the same bounds
    kept, keep = T.vet_rows(r, True, True, chi2_max=50.0, fwhm_gauss_min=2.0, fwhm_gauss_max=10.0, elong_gauss_max=2.0)
    assert (kept, keep) == T.vet_transients(r, chi2_max=50.0, fwhm_gauss_min=2.0, fwhm_gauss_max=10.0, elong_gauss_max=2.0) and keep == [0, 2]
    # a bound under which every row leaves: an empty list, not None
    assert T.vet_rows(r, True, True, chi2_max=0.1) == ([], [])
