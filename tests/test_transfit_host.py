"""CPU: the transient vetting's definition (transfit_ref.py: the numpy restatement of bbx_zogy_pd_stamps and bbx_trans_psffit) measured
on the host, and the switches around it.

  P_D        the restatement on the small grid against numpy.fft on the full L = 1400 grid (oracle/zogy_core.run_zogy's PDh)
  recovery   a toy sub-image through oracle/zogy_core.run_zogy: positions and fluxes of injected point sources within K_SIGMA of
             the fit's own error estimates; the chi2 of spikes and dipoles against that of the point sources
  float32    the float32 restatement against the float64 one over the case table: the D32_* of transfit_ref.py
  switches   argparse and settings defaults, the table's columns, the chi2 filter, the header keys

zogy's PSF fit to D is not in the reference tree: the rules are this project's own, parity is unpinned."""
import functools
import os

import numpy as np
import pytest

import psfphot_ref as PR
import transfit_ref as T
import zogy_core as Z

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- P_D --------------------------------------------------------------------------------------------------------------------
L_FULL, S_PD = 1400, 49
SCAL_PD = np.array([10.0, 5.0, 1.0, 1.1, 0.1, 0.1], F)
SCAL_BOX = np.array([10.0, 0.2, 1.0, 1.1, 0.1, 0.1], F)              # a deep reference: nothing but |Pr^| in the denominator


def pd_full_grid(pn, pr, sc):
    """the stamp cut from P_D on the full sub-image grid, unit sum"""
    p = T.pd_grid(pn, pr, sc, L_FULL)
    i = (np.arange(S_PD) - S_PD // 2) % L_FULL
    st = p[np.ix_(i, i)]
    return st / st.sum()


def test_pd_on_the_small_grid_meets_the_full_grid():
    dev, fold = [], []
    for fn_, fr_ in T.PD_PAIRS:
        pn, pr = PR.moffat_stamp(S_PD, fn_).astype(F), PR.moffat_stamp(S_PD, fr_).astype(F)
        pd, fo = T.pd_stamps_ref(pn[None], pr[None], SCAL_PD[None], 256)
        full = pd_full_grid(pn, pr, SCAL_PD)
        dev.append(np.abs(pd[0] - full).max() / full.max())
        fold.append(fo[0])
        print('FWHM %.1f / %.1f: max |P_D(256) - P_D(1400)| / peak %.2e, fold %.3e' % (fn_, fr_, dev[-1], fold[-1]))
    point = np.zeros((S_PD, S_PD), F)
    point[S_PD // 2, S_PD // 2] = 1
    box = np.zeros((S_PD, S_PD), F)
    box[S_PD // 2 - 2:S_PD // 2 + 3, S_PD // 2 - 2:S_PD // 2 + 3] = 1 / 25.0
    fold_box = T.pd_stamps_ref(point[None], box[None], SCAL_BOX[None], 256)[1][0]
    print('largest deviation %.3e (module: %.1e), largest fold %.3e (module: %.1e), fold of point / box %.3e (module: %.1e)'
          % (max(dev), T.PD_GRID_DEV, max(fold), T.PD_FOLD_MOFFAT, fold_box, T.PD_FOLD_BOX))
    assert max(dev) <= T.PD_GRID_DEV and max(fold) <= T.PD_FOLD_MOFFAT and fold_box >= T.PD_FOLD_BOX
    # the threshold of a warning lies well between the two: a decade above the Moffat pairs, a factor 3 below the box pair
    assert 10 * T.PD_FOLD_MOFFAT <= T.PD_FOLD_WARN <= T.PD_FOLD_BOX / 3
    from blackbox_amd import zogy as G
    assert G.PD_FOLD_WARN == T.PD_FOLD_WARN


def test_pd_rules():
    c = T.make_pd_case(15, 64, 12)
    pd, fold = T.pd_stamps_ref(c['pn'], c['pr'], c['scal'], 64)
    dead = [11, 6]
    for k in range(12):
        if k in dead:
            assert not pd[k].any() and fold[k] == 1
        else:
            assert abs(pd[k].sum() - 1) < 1e-12 and 0 <= fold[k] < 0.05
    # equal PSFs and equal noise: P_D^ = P^ P^ / (sqrt(2) |P^|) is not P, but its centre stays put and it is symmetric
    p = PR.moffat_stamp(21, 3.5).astype(F)
    pd = T.pd_stamps_ref(p[None], p[None], np.array([[7, 7, 1, 1, 0, 0]], F), 128)[0][0]
    assert np.unravel_index(pd.argmax(), pd.shape) == (10, 10) and np.allclose(pd, pd[::-1, ::-1], atol=1e-9)


# ---- recovery ---------------------------------------------------------------------------------------------------------------
L_TOY, S_TOY, W_TOY, SEED_TOY = 128, 21, 11, 2
# positions and fluxes of the point sources within K_SIGMA of the fit's own errors.  Observed (seed 2, 64 sources, float64
# restatement): positions 2.55, flux 2.45; seeds 1 and 3: 3.04 / 2.15 and 2.60 / 3.32
K_SIGMA = 5.0
# chi2 of the point sources (seed 2): median 1.03, standard deviation 0.30, largest 1.79; the smallest of the spikes 36.4,
# of the dipoles 34.8
ARTEFACT_FACTOR = 3.0


def point_spectrum(pos, flux, L):
    """band-limited point sources at sub-pixel positions: the transform of shifted deltas"""
    ky, kx = np.meshgrid(np.fft.fftfreq(L), np.fft.fftfreq(L), indexing='ij')
    h = np.zeros((L, L), complex)
    for (y, x), f in zip(pos, flux):
        h += f * np.exp(-2j * np.pi * (ky * y + kx * x))
    return h


@functools.lru_cache(maxsize=4)
def toy(seed=SEED_TOY, artefacts=False):
    """one sub-image through oracle/zogy_core.run_zogy.  Point sources (artefacts False): 64 on a grid of 14 px, offsets over the
    half-pixel square, S/N 10 .. 300 against the background's noise, both signs (a negative one is a star of the reference that
    is gone).  Artefacts: 8 single-pixel spikes of 300 .. 1000 sigma in the new image only and 8 stars of 1 .. 3 10^5 e- that sit
    0.7 px apart in the new image and the reference, on a grid of 20 px.  Noise: Gaussian of variance max(image, 0) + sigma^2"""
    L, S = L_TOY, S_TOY
    rs = np.random.RandomState(seed + (1000 if artefacts else 0))
    Pn, Pr = PR.moffat_stamp(S, 3.2), PR.moffat_stamp(S, 3.8)
    sn, sr = 10.0, 5.0
    step = 20 if artefacts else 14
    gy, gx = np.mgrid[step:L - 10:step, step:L - 10:step]
    cells = np.stack([gy.ravel(), gx.ravel()], 1).astype(float)
    rs.shuffle(cells)
    npt, nsp, ndp = (0, 8, 8) if artefacts else (len(cells), 0, 0)
    ppos = cells[:npt] + rs.uniform(-0.5, 0.5, (npt, 2))
    snr = 10 ** rs.uniform(1, np.log10(300), npt)
    pflux = snr * 65.0 * np.where(np.arange(npt) % 2, -1, 1)
    spos, sflux = cells[npt:npt + nsp], rs.uniform(3000, 10000, nsp)
    dpos = cells[npt + nsp:npt + nsp + ndp] + rs.uniform(-0.5, 0.5, (ndp, 2))
    dflux = rs.uniform(1e5, 3e5, ndp)
    ang = rs.uniform(0, 2 * np.pi, ndp)
    dpos_n = dpos + 0.7 * np.stack([np.sin(ang), np.cos(ang)], 1)
    base = np.abs(pflux) * (pflux < 0)
    En, Er = T.embed(Pn, L), T.embed(Pr, L)
    Rt = np.fft.ifft2((point_spectrum(ppos, base, L) + point_spectrum(dpos, dflux, L)) * np.fft.fft2(Er)).real
    Nt = np.fft.ifft2((point_spectrum(ppos, base + pflux, L) + point_spectrum(dpos_n, dflux, L)) * np.fft.fft2(En)).real
    for (y, x), f in zip(spos, sflux):
        Nt[int(y), int(x)] += f
    N = (Nt + rs.normal(0, 1, Nt.shape) * np.sqrt(np.maximum(Nt, 0) + sn ** 2)).astype(F)
    R = (Rt + rs.normal(0, 1, Rt.shape) * np.sqrt(np.maximum(Rt, 0) + sr ** 2)).astype(F)
    Vn, Vr = (np.maximum(N, 0) + F(sn) ** 2).astype(F), (np.maximum(R, 0) + F(sr) ** 2).astype(F)
    D = Z.run_zogy(N, R, En, Er, sn, sr, 1.0, 1.0, Vn, Vr, 0.0, 0.0)[0]
    scal = np.array([[sn, sr, 1, 1, 0, 0]], F)
    pd, fold = T.pd_stamps_ref(Pn[None].astype(F), Pr[None].astype(F), scal, L)
    return dict(D=D, N=N, R=R, sn=sn, sr=sr, scal=scal, pd=pd.astype(F), fold=fold, ppos=ppos, pflux=pflux, spos=spos, dpos=(dpos + dpos_n) / 2)


def toy_fit(t, pos, dtype=np.float64):
    ys, xs = np.rint(pos[:, 0]).astype(int), np.rint(pos[:, 1]).astype(int)
    sgn, sgr = np.full((L_TOY, L_TOY), t['sn'], F), np.full((L_TOY, L_TOY), t['sr'], F)
    return ys, xs, T.trans_psffit_ref(t['D'], t['N'], t['R'], sgn, sgr, None, t['pd'], ys, xs, t['scal'], L_TOY, 1, W_TOY, T.NITER, T.MAXSHIFT, dtype)


def test_point_sources_are_recovered():
    t = toy()
    ys, xs, o = toy_fit(t, t['ppos'])
    assert not o['flags'].any()
    ey, ex = (ys + o['dy'] - t['ppos'][:, 0]) / o['dy_err'], (xs + o['dx'] - t['ppos'][:, 1]) / o['dx_err']
    ef = (o['flux'] - t['pflux']) / o['err']
    print('%d point sources, |S/N| %.0f .. %.0f: largest |dy| / err %.2f, |dx| / err %.2f, |dflux| / err %.2f (K_SIGMA %.1f); chi2 median %.3f std %.3f '
          'max %.3f' % (len(ys), np.abs(o['flux'] / o['err']).min(), np.abs(o['flux'] / o['err']).max(), np.abs(ey).max(), np.abs(ex).max(),
                        np.abs(ef).max(), K_SIGMA, np.median(o['chi2']), o['chi2'].std(), o['chi2'].max()))
    assert (t['pflux'] < 0).sum() >= 20 and (o['flux'] < 0).sum() == (t['pflux'] < 0).sum()
    assert max(np.abs(ey).max(), np.abs(ex).max(), np.abs(ef).max()) <= K_SIGMA
    assert 0.8 < np.median(o['chi2']) < 1.3


def test_artefacts_have_a_larger_chi2_than_any_point_source():
    top = toy_fit(toy(), toy()['ppos'])[2]['chi2'].max()
    a = toy(SEED_TOY, True)
    spikes, dipoles = toy_fit(a, a['spos'])[2], toy_fit(a, a['dpos'])[2]
    print('largest chi2 of a point source %.2f; spikes %s; dipoles %s' % (top, np.round(np.sort(spikes['chi2']), 1), np.round(np.sort(dipoles['chi2']), 1)))
    assert not (spikes['flags'] & T.NO_FIT).any() and not (dipoles['flags'] & T.NO_FIT).any()
    assert spikes['chi2'].min() >= ARTEFACT_FACTOR * top and dipoles['chi2'].min() >= ARTEFACT_FACTOR * top


# ---- float32 against float64 --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_runs(spec):
    case = T.make_case(*spec)
    sg = T.sigma_frames(case)
    return case, T.run_case(case, np.float64, sg), T.run_case(case, np.float32, sg)


def test_float32_follows_float64():
    worst = dict(flux=0.0, err=0.0, chi2=0.0, pos=0.0)
    seen = 0
    for spec in T.CASES:
        case, a, b = case_runs(spec)
        assert np.array_equal(a['flags'], b['flags']), spec
        ok = (a['flags'] & T.NO_FIT) == 0
        seen |= int(np.bitwise_or.reduce(a['flags']))
        for k in ('flux', 'err', 'chi2'):
            worst[k] = max(worst[k], float(np.abs(b[k][ok] / a[k][ok] - 1).max()))
        worst['pos'] = max(worst['pos'], float(np.abs(b['dy'] - a['dy']).max()), float(np.abs(b['dx'] - a['dx']).max()))
        # no fitted candidate's last step lies where rounding could flip bit 8
        for r in (a, b):
            last = r['last'][ok]
            assert not ((last >= 1e-3) & (last <= 1e-1)).any(), spec
        assert not a['flux'][~ok].any() and not a['chi2'][~ok].any() and not a['dy'][~ok].any()
    print('float32 against float64: flux %.2e (D32_FLUX %.1e) err %.2e (%.1e) chi2 %.2e (%.1e) dy, dx %.2e px (%.1e)'
          % (worst['flux'], T.D32_FLUX, worst['err'], T.D32_ERR, worst['chi2'], T.D32_CHI2, worst['pos'], T.D32_POS))
    assert seen == 15                                                # every flag bit occurs in the table
    assert worst['flux'] <= T.D32_FLUX and worst['err'] <= T.D32_ERR and worst['chi2'] <= T.D32_CHI2 and worst['pos'] <= T.D32_POS


def test_case_table_reaches_the_variants():
    case, a, _ = case_runs((21, 3, 300, 'frame', 'hits'))
    assert a['flags'][0] == T.NO_FIT | T.MASKED                      # the corner peak under W = 3 with its centre masked: 3 pixels left
    assert a['flags'][T.FAR] & T.AT_BOUND and a['flags'][T.FAR] & T.NOT_CONVERGED
    assert (a['flux'] < 0).sum() > 50 and np.isnan(case['D']).sum() == 1 and np.isnan(case['N']).sum() == 1
    ok = a['flags'] == 0
    err = np.abs(np.stack([a['dy'], a['dx']], 1)[ok] - case['off'][ok])
    assert ok.sum() > 200 and np.median(err) < 0.1


# ---- switches ---------------------------------------------------------------------------------------------------------------
ROWS = [dict(y=10, x=20, scorr=9.0, fpsf=100.0, fpsferr=10.0, y_psf_d=10.25, x_psf_d=19.5, flux_psf_d=101.0, fluxerr_psf_d=9.0, chi2_psf_d=1.1,
             flags_psf_d=0),
        dict(y=30, x=40, scorr=-7.0, fpsf=-80.0, fpsferr=10.0, y_psf_d=30.0, x_psf_d=40.0, flux_psf_d=0.0, fluxerr_psf_d=0.0, chi2_psf_d=0.0,
             flags_psf_d=4),
        dict(y=50, x=60, scorr=30.0, fpsf=900.0, fpsferr=10.0, y_psf_d=50.5, x_psf_d=60.1, flux_psf_d=700.0, fluxerr_psf_d=9.0, chi2_psf_d=25.0,
             flags_psf_d=8),
        dict(y=70, x=80, scorr=8.0, fpsf=90.0, fpsferr=10.0, y_psf_d=69.9, x_psf_d=80.2, flux_psf_d=95.0, fluxerr_psf_d=9.0, chi2_psf_d=0.9,
             flags_psf_d=2)]
BASE_KEYS = ('y', 'x', 'scorr', 'fpsf', 'fpsferr')


def test_settings_and_arguments_default_to_off():
    import importlib.util
    from blackbox_amd import settings
    assert settings.trans_psffit is False and settings.trans_chi2_max is None
    assert (settings.trans_fit_size, settings.trans_fit_niter, settings.trans_fit_maxshift, settings.trans_pd_grid) == (11, 8, 2.0, 256)
    spec = importlib.util.spec_from_file_location('blackbox_cli_transfit', os.path.join(ROOT, 'blackbox.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args([])
    assert a.trans_psffit is None and a.trans_fit_size is None and a.trans_chi2_max is None
    a = cli.build_parser().parse_args(['--trans_psffit', 'True', '--trans_fit_size', '7', '--trans_chi2_max', '4.5'])
    assert a.trans_psffit is True and a.trans_fit_size == 7 and a.trans_chi2_max == 4.5


def test_table_columns(tmp_path):
    from blackbox_amd import catalogs, fitsio
    plain = [{k: r[k] for k in BASE_KEYS} for r in ROWS]
    base = catalogs._transient_columns(plain)
    assert list(base) == ['X_PEAK', 'Y_PEAK', 'SNR_ZOGY', 'E_FLUX_ZOGY', 'E_FLUXERR_ZOGY']
    assert list(catalogs._transient_columns([])) == list(base)
    full = catalogs._transient_columns(ROWS)
    assert list(full) == list(base) + [c[0] for c in catalogs.TRANSFIT_COLUMNS]
    for k in base:
        assert full[k].tobytes() == base[k].tobytes()
    assert full['X_PSF_D'].tolist() == [20.5, 41.0, F(61.1), F(81.2)] and full['Y_PSF_D'][0] == 11.25 and full['FLAGS_PSF_D'].dtype == np.uint8
    # ... and in the file: the columns follow today's, which keep their bytes
    catalogs.format_cat(catalogs.transient_table(plain), str(tmp_path / 'a.fits'), cat_type='trans')
    catalogs.format_cat(catalogs.transient_table(ROWS), str(tmp_path / 'b.fits'), cat_type='trans')
    ta, tb = fitsio.read_table(str(tmp_path / 'a.fits'))[0], fitsio.read_table(str(tmp_path / 'b.fits'))[0]
    assert list(tb) == list(ta) + [c[0] for c in catalogs.TRANSFIT_COLUMNS]
    for k in ta:
        assert np.array_equal(ta[k], tb[k])
    assert tb['CHI2_PSF_D'].dtype.kind == 'f' and tb['FLAGS_PSF_D'].tolist() == [0, 4, 8, 2]


def test_chi2_filter_and_header_keys():
    from blackbox_amd import zogy as G
    kept, idx = G.vet_transients(ROWS, 5.0)
    assert idx == [0, 3] and kept == [ROWS[0], ROWS[3]]
    assert G.vet_transients(ROWS, 100.0)[1] == [0, 2, 3]             # the row without a fit goes whatever the bound
    h = G.trans_fit_header(True, 11, ROWS, np.array([0.001, 0.004, 0.002], F))
    assert list(h) == ['T-PSFD', 'T-FITSZ', 'T-NFIT', 'T-PDFOLD', 'T-CHI2MD']
    assert h['T-PSFD'][0] is True and h['T-FITSZ'][0] == 11 and h['T-NFIT'][0] == 2 and h['T-PDFOLD'][0] == pytest.approx(0.004)
    assert h['T-CHI2MD'][0] == pytest.approx(1.0)
    none = G.trans_fit_header(True, 11, ROWS[1:3], np.array([0.001], F))
    assert none['T-NFIT'][0] == 0 and none['T-CHI2MD'][0] == 'None'
    assert list(G.trans_fit_header(False)) == ['T-PSFD'] and G.trans_fit_header(False)['T-PSFD'][0] is False
