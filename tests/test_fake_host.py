"""CPU: the fake stars' definition (fake_ref.py: the numpy restatement of bbx_fake_inject and bbx_fake_recover) measured on the host,
and the host stage around the kernels.

  layout     deterministic, the stars' distances, the sizes that do not fit, the S/N cycle
  root       S/N(F) = s on stamps with negative wings under a sigma gradient
  float32    the float32 restatement against the float64 one over the case table: the D32_* of fake_ref.py
  generator  moments and correlations of the deviates, no word shared between two stars' streams, a known answer of Philox4x32-10
  recovery   a toy sub-image through oracle/zogy_core.run_zogy: stars of S/N 2 and 30, found or not, the flux pulls
  forms      the table, the header keys with their 'None' rules, the switches, the entry points' argument checks

zogy's fake stars are not in the reference tree: the rules are this project's own, parity is unpinned."""
import ctypes
import functools

import numpy as np
import pytest
from scipy import ndimage

import fake_ref as FR
import psfphot_ref as PR
import zogy_core as Z
from blackbox_amd import fakestars as K

F = np.float32


# ---- layout -----------------------------------------------------------------------------------------------------------------
def min_chebyshev(ys, xs):
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    best = np.inf
    for i in range(0, len(ys), 512):
        d = np.maximum(np.abs(ys[i:i + 512, None] - ys[None]), np.abs(xs[i:i + 512, None] - xs[None]))
        d[np.arange(d.shape[0]), np.arange(i, i + d.shape[0])] = 1 << 40
        best = min(best, d.min())
    return best


@pytest.mark.parametrize('size,S,nper,nsy,nsx', [(120, 21, 1, 3, 4), (120, 21, 4, 3, 4), (120, 21, 9, 3, 4), (120, 21, 16, 3, 4), (1320, 49, 16, 2, 2),
                                                  (1320, 49, 529, 2, 2)])
def test_layout(size, S, nper, nsy, nsx):
    ny, nx = nsy * size, nsx * size
    a = K.fake_layout(ny, nx, size, nsy, nsx, S, nper, (3, 5, 7), 11)
    b = K.fake_layout(ny, nx, size, nsy, nsx, S, nper, (3, 5, 7), 11)
    c = K.fake_layout(ny, nx, size, nsy, nsx, S, nper, (3, 5, 7), 12)
    for k in ('ys', 'xs', 'off', 's2n', 'sub'):
        assert a[k].tobytes() == b[k].tobytes()
    assert a['ys'].tobytes() != c['ys'].tobytes() or a['xs'].tobytes() != c['xs'].tobytes()
    n = nsy * nsx * nper
    assert a['ys'].shape == (n,) and a['off'].shape == (n, 2) and a['ys'].dtype == np.int32 and a['off'].dtype == F
    assert min_chebyshev(a['ys'], a['xs']) >= S + 7
    assert np.abs(a['off']).max() <= 0.5
    h = S // 2
    assert a['ys'].min() >= h and a['xs'].min() >= h and a['ys'].max() + h < ny and a['xs'].max() + h < nx
    assert (a['sub'] == (a['ys'] // size) * nsx + a['xs'] // size).all() and np.bincount(a['sub'], minlength=nsy * nsx).tolist() == [nper] * (nsy * nsx)
    assert a['s2n'].tolist() == [(3.0, 5.0, 7.0)[i % 3] for i in range(n)]                  # the S/N list cycles
    K.check_apart(a['ys'], a['xs'], S)


@pytest.mark.parametrize('size,S,nper', [(120, 21, 17), (1320, 49, 530)])
def test_layout_refuses_what_does_not_fit(size, S, nper):
    with pytest.raises(ValueError):
        K.fake_layout(size, size, size, 1, 1, S, nper, (10,), 0)


def test_layout_and_distance_rules():
    with pytest.raises(ValueError):
        K.fake_layout(120, 120, 120, 1, 1, 21, 4, tuple(range(1, 10)), 0)                  # nine S/N values
    with pytest.raises(ValueError):
        K.check_apart([10, 30], [10, 30], 21)
    K.check_apart([10, 31], [10, 10], 21)                                                   # touching stamps are apart
    assert K.fake_s2n_list('3,5.5') == (3.0, 5.5) and K.fake_s2n_list(10) == (10.0,)


# ---- root -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fwhm', [3.0, 4.2])
@pytest.mark.parametrize('s', [1e-3, 2.0, 20.0, 1e4])
def test_root(fwhm, s):
    S = 25
    p = FR.wing_stamp(S, fwhm, 0.3, -0.2)
    assert p.min() < 0
    gy, gx = np.mgrid[0:S, 0:S]
    v = (8.0 + 0.15 * gy - 0.1 * gx) ** 2
    lo, hi, _, _ = FR.brackets(s, p, v)
    assert FR.snr(lo, p, v) <= s * (1 + 1e-14) and FR.snr(hi, p, v) >= s * (1 - 1e-14)      # the bracket holds
    Fl = FR.flux_root(s, p, v)
    # within 1e-12 wherever float64 can hold it; relative at s = 1e4, where one ulp is 1.8e-12 already
    assert abs(FR.snr(Fl, p, v) - s) <= 1e-12 * max(1.0, s / 20.0)
    assert FR.snr(Fl * (1 + 1e-6), p, v) > FR.snr(Fl, p, v)                                 # increasing


# ---- float32 against float64 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(i):
    return FR.make_case(*FR.CASES[i])


def test_float32_follows_float64():
    d_f = d_add = d_noise = 0.0
    for i in range(len(FR.CASES)):
        c = case(i)
        for g in c['groups']:
            r64, r32 = FR.run_group(c, g, np.float64), FR.run_group(c, g, np.float32)
            n64, n32 = FR.run_group(c, g, np.float64, noise=True, seed=31), FR.run_group(c, g, np.float32, noise=True, seed=31)
            assert r64['flags'].tolist() == r32['flags'].tolist() == n64['flags'].tolist() == n32['flags'].tolist() == [s['want'] for s in g['stars']]
            for k in np.nonzero(r64['flags'] == 0)[0]:
                d_f = max(d_f, abs(r32['flux'][k] / r64['flux'][k] - 1))
                d_add = max(d_add, np.abs(r32['add'][k] - r64['add'][k]).max() / (r64['flux'][k] * r64['pmax'][k]))
                # the part of the add that the deviates bring, in units of its own scale sqrt(F max P)
                dn = (n32['add'][k] - r32['add'][k]) - (n64['add'][k] - r64['add'][k])
                d_noise = max(d_noise, np.abs(dn).max() / np.sqrt(r64['flux'][k] * r64['pmax'][k]))
    print('largest |F32 / F64 - 1| %.3e (module: %.1e), largest |add32 - add64| / (F max P) %.3e (module: %.1e), largest |n32 - n64| / sqrt(F max P) '
          '%.3e (module: %.1e)' % (d_f, FR.D32_F, d_add, FR.D32_ADD, d_noise, FR.D32_NOISE))
    assert d_f <= FR.D32_F and d_add <= FR.D32_ADD and d_noise <= FR.D32_NOISE
    # the recorded figures are the measured ones, rounded up in their last digit: nothing to spare in them
    assert d_f >= 0.9 * FR.D32_F and d_add >= 0.9 * FR.D32_ADD and d_noise >= 0.9 * FR.D32_NOISE


def test_cases_cover_what_they_name():
    """every case holds every tag; the touching pair shares a launch; the flagged stars leave their frame alone"""
    for i in (0, 5):
        c = case(i)
        tags = [s['tag'] for g in c['groups'] for s in g['stars']]
        assert len(set(tags)) == len(tags) >= 24 and 'sigma_zero' in tags
        assert any({'corner_tl', 'touching'} <= {s['tag'] for s in g['stars']} for g in c['groups'])
        for g in c['groups']:
            r = FR.run_group(c, g)
            inside = np.zeros((c['ny'], c['nx']), bool)
            h = c['S'] // 2
            for s, fl in zip(g['stars'], r['flags']):
                if fl == 0:
                    inside[s['y'] - h:s['y'] + h + 1, s['x'] - h:s['x'] + h + 1] = True
            assert r['out'][~inside].tobytes() == g['frame'][~inside].tobytes()


# ---- generator --------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32-10
    assert [int(v) for v in FR.philox4x32(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    m = 0xffffffff
    assert [int(v) for v in FR.philox4x32(m, m, m, m, m, m)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(v) for v in FR.philox4x32(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_generator_moments():
    nstar, npx = 64, 49 * 49
    g = np.stack([FR.normals(12345, s, npx) for s in range(nstar)])
    n = g.size
    assert n >= 100000 and np.isfinite(g).all()
    assert abs(g.mean()) <= 5 / np.sqrt(n) and abs(g.var() - 1) <= 5 * np.sqrt(2.0 / n)
    assert abs((g[:, 1:] * g[:, :-1]).mean()) <= 5 / np.sqrt(n)                              # lag 1 inside a star
    assert abs((g[1:] * g[:-1]).mean()) <= 5 / np.sqrt(n)                                    # the same pixel of two stars
    words = np.stack([np.stack(FR.star_words(12345, s, npx)) for s in range(nstar)])
    assert len(np.unique(words[:, 0] .astype(np.uint64) << np.uint64(32) | words[:, 1].astype(np.uint64))) == n      # no (r0, r1) pair twice
    assert FR.normals(12345, 3, 50).tobytes() == FR.normals(12345, 3, 50).tobytes()
    assert FR.normals(12346, 3, 50).tobytes() != FR.normals(12345, 3, 50).tobytes()
    assert FR.normals(1 << 32, 3, 50).tobytes() != FR.normals(0, 3, 50).tobytes()            # the high word is part of the key


def test_noise_bound_of_the_flat_stamp():
    """the float32 frame of a flat stamp on zeros against the float64 deviates: the NOISE_TOL the GPU test uses"""
    S = 49
    cube = np.full((1, S, S), 1.0 / (S * S), F)
    sigma = np.ones((60, 60), F)
    s2n = F(FR.snr(4.0 * S * S, cube[0].astype(np.float64) / cube[0].astype(np.float64).sum(), np.ones(S * S)))
    r = FR.inject_ref(np.zeros((60, 60), F), None, sigma, None, None, cube, None, [0], [30], [30], np.zeros((1, 2), F), [s2n], noise=True, seed=7,
                      dtype=np.float32)
    assert r['flags'][0] == 0
    fp = r['flux'][0] / (S * S)
    dev = np.abs((r['out'][6:55, 6:55].astype(np.float64) - fp) / np.sqrt(fp) - FR.normals(7, 0, S * S).reshape(S, S)).max()
    print('F P = %.6f, largest |(out - F P) / sqrt(F P) - g| %.3e (module: %.1e)' % (fp, dev, FR.NOISE_TOL))
    assert abs(fp - 4.0) < 1e-3 and dev <= FR.NOISE_TOL


# ---- recovery ---------------------------------------------------------------------------------------------------------------
L_TOY, S_TOY, NSIG_TOY, RADIUS = 256, 21, 6.0, 2


def embed(Pm, L):
    out = np.zeros((L, L))
    S = Pm.shape[0]
    i = (np.arange(S) - S // 2) % L
    out[np.ix_(i, i)] = Pm
    return out


@functools.lru_cache(maxsize=2)
def toy(noise):
    """one sub-image through oracle/zogy_core.run_zogy: 64 stars of S/N 2 and 30 in turn, injected by the restatement into a new frame
    of pure sky noise; the reference has the same PSF and the same sky noise"""
    rs = np.random.RandomState(4)
    L, S, sky = L_TOY, S_TOY, 10.0
    Pm = PR.moffat_stamp(S, 3.4)
    lay = K.fake_layout(L, L, L, 1, 1, S, 64, (2, 30), 9)
    N0 = (rs.normal(0, sky, (L, L))).astype(F)
    R = (rs.normal(0, sky, (L, L))).astype(F)
    sig = np.full((L, L), sky, F)
    inj = FR.inject_ref(N0, R, sig, None, None, Pm[None].astype(F), None, np.zeros(64, np.int32), lay['ys'], lay['xs'], lay['off'], lay['s2n'],
                        3, 5.0, noise, lay['seed'])
    N = inj['out']
    Vn, Vr = (np.maximum(N, 0) + F(sky) ** 2).astype(F), (np.maximum(R, 0) + F(sky) ** 2).astype(F)
    E = embed(Pm, L)
    _, _, Scorr, Fpsf, Fpsferr = Z.run_zogy(N, R, E, E, sky, sky, 1.0, 1.0, Vn, Vr, 0.0, 0.0)
    rec = FR.recover_ref(Scorr, Fpsf, Fpsferr, lay['ys'], lay['xs'], RADIUS)
    peak = (Scorr == ndimage.maximum_filter(Scorr, size=3)) & (Scorr >= NSIG_TOY)
    ty, tx = np.nonzero(peak)
    order = np.argsort(-Scorr[ty, tx], kind='stable')
    trans = [dict(y=int(ty[k]), x=int(tx[k]), scorr=float(Scorr[ty[k], tx[k]]), fpsf=float(Fpsf[ty[k], tx[k]]), fpsferr=float(Fpsferr[ty[k], tx[k]]))
             for k in order]
    first = K.fake_match(trans, lay, RADIUS, flags=inj['flags'])
    tab = K.fake_table(lay, (inj['flux'], inj['real'], inj['snr_sky'], inj['flags']), rec, NSIG_TOY, first, first)
    hdr = K.fake_header(True, tab, lay, noise, RADIUS, int((first > 0).sum()))
    return dict(lay=lay, inj=inj, tab=tab, hdr=hdr, trans=trans, first=first)


@pytest.mark.parametrize('noise', [False, True])
def test_stars_are_recovered(noise):
    t = toy(noise)
    tab, hdr = t['tab'], t['hdr']
    ok = tab['FLAGS_IN'] == 0
    print('noise %s: flagged %d, T-FKFRAT %s, T-FKFSTD %s, T-FKPULL %s, T-FKSCRT %s, T-FKEF1 %s, T-FKEF2 %s' % (
        noise, int((~ok).sum()), hdr['T-FKFRAT'][0], hdr['T-FKFSTD'][0], hdr['T-FKPULL'][0], hdr['T-FKSCRT'][0], hdr['T-FKEF1'][0], hdr['T-FKEF2'][0]))
    assert ok.sum() >= 60
    bright, faint = ok & (tab['SNR_IN'] == 30), ok & (tab['SNR_IN'] == 2)
    # equal sky noise and PSFs: Scorr ~ S/N / sqrt(2) = 21 at S/N 30, 15 sigma above the threshold; 1.4 at S/N 2
    assert ((tab['FOUND'][bright] & 3) == 3).all() and (tab['NUMBER_TRANS'][bright] > 0).all()
    assert int(((tab['FOUND'][faint] & 3) != 0).sum()) <= 1
    for k in np.nonzero(bright)[0]:
        row = t['trans'][tab['NUMBER_TRANS'][k] - 1]
        assert max(abs(row['y'] - t['lay']['ys'][k]), abs(row['x'] - t['lay']['xs'][k])) <= RADIUS and t['first'][tab['NUMBER_TRANS'][k] - 1] == k + 1
    pull = ((tab['E_FLUX_OUT'] - tab['E_FLUX_REAL']) / tab['E_FLUXERR_OUT'])[bright].astype(np.float64)
    print('median pull of the %d S/N 30 stars %.3f (bound %.3f)' % (pull.size, np.median(pull), 5 * 1.2533 / np.sqrt(pull.size)))
    assert abs(np.median(pull)) <= 5 * 1.2533 / np.sqrt(pull.size)
    assert hdr['T-NFAKE'][0] == int(ok.sum()) and hdr['T-FAKESN'][0] == 2.0 and hdr['T-FKEF2'][0] == 1.0


# ---- forms ------------------------------------------------------------------------------------------------------------------
KEYS_ON = ['T-FKP', 'T-NFAKE', 'T-FAKESN', 'T-FKNASK', 'T-FKNREJ', 'T-FKSEED', 'T-FKNOIS', 'T-FKRAD', 'T-NFKTR', 'T-FKSN1', 'T-FKN1', 'T-FKEF1',
           'T-FKVT1', 'T-FKSN2', 'T-FKN2', 'T-FKEF2', 'T-FKVT2', 'T-FKFRAT', 'T-FKFSTD', 'T-FKPULL', 'T-FKSCRT']


def small_table(n, flags=None, snr=10.0):
    lay = dict(ys=np.arange(n, dtype=np.int32) * 30 + 20, xs=np.full(n, 40, np.int32), off=np.zeros((n, 2), F), s2n=np.full(n, snr, F),
               s2n_list=(snr, 50.0), seed=3)
    flags = np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    flux = np.where(flags == 0, 1000.0, 0).astype(F)
    rec = np.zeros((n, 6), F)
    rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = 8.0, 1010.0, 100.0, 990.0
    first = np.arange(1, n + 1)
    return lay, K.fake_table(lay, (flux, flux, flux / 100, flags), rec, 6.0, first, first[::2])


def test_header_and_table_forms():
    from blackbox_amd import catalogs
    assert K.FAKE_COLS == tuple(c[0] for c in catalogs.FAKESTAR_TABLE)
    lay, tab = small_table(4)
    assert tuple(tab) == K.FAKE_COLS and all(len(v) == 4 for v in tab.values())
    assert tab['FOUND'].tolist() == [7, 3, 7, 3] and tab['NUMBER_TRANS'].tolist() == [1, 0, 2, 0]
    assert tab['X_IN'].tolist() == [41.0] * 4 and tab['Y_IN'].tolist() == [21.0, 51.0, 81.0, 111.0] and tab['Y_PEAK'].tolist() == tab['Y_IN'].tolist()
    h = K.fake_header(True, tab, lay, True, 2, 4)
    assert list(h) == KEYS_ON
    assert [h[k][0] for k in ('T-FKFRAT', 'T-FKFSTD', 'T-FKPULL', 'T-FKSCRT')] == ['None'] * 4          # four stars: no statistics
    assert h['T-NFAKE'][0] == 4 and h['T-FAKESN'][0] == 10.0 and h['T-FKN1'][0] == 2 and h['T-FKEF1'][0] == 1.0 and h['T-FKVT1'][0] == 1.0
    assert h['T-FKVT2'][0] == 0.0 and h['T-NFKTR'][0] == 4 and h['T-FKP'][0] is True
    lay, tab = small_table(5)
    h = K.fake_header(True, tab, lay, False, 2, 5)
    assert abs(h['T-FKFRAT'][0] - 1.01) < 1e-6 and h['T-FKFSTD'][0] < 1e-6 and h['T-FKPULL'][0] == 0.0 and abs(h['T-FKSCRT'][0] - 0.8) < 1e-6
    lay, tab = small_table(6, flags=[0, 4, 0, 0, 0, 1])                  # two rejected: four left
    h = K.fake_header(True, tab, lay, False, 2, 4)
    assert h['T-FKFRAT'][0] == 'None' and h['T-NFAKE'][0] == 4 and h['T-FKNREJ'][0] == 2 and h['T-FKNASK'][0] == 6
    assert tab['FOUND'][1] & 1 == 0
    lay, tab = small_table(8, snr=9.0)                                   # below S/N 10: no statistics either
    assert K.fake_header(True, tab, lay, False, 2, 8)['T-FKPULL'][0] == 'None'
    # an S/N of the list without a star: its shares are 'None'
    lay, tab = small_table(1)
    assert K.fake_header(True, tab, lay, False, 2, 1)['T-FKEF2'][0] == 'None'
    off = K.fake_header(False)
    assert list(off) == ['T-FKP', 'T-NFAKE', 'T-FAKESN'] and off['T-FKP'][0] is False and off['T-NFAKE'][0] == 0


def test_match_rules():
    lay = dict(ys=np.array([20, 60], np.int32), xs=np.array([20, 60], np.int32))
    rows = [dict(y=22, x=18, scorr=7.0), dict(y=23, x=20, scorr=9.0), dict(y=60, x=60, scorr=-8.0), dict(y=59, x=61, scorr=6.5), dict(y=100, x=5, scorr=50.0)]
    assert K.fake_match(rows, lay, 2).tolist() == [1, 0, 0, 2, 0]
    assert K.fake_match(rows, lay, 2, flags=[2, 0]).tolist() == [0, 0, 0, 2, 0]             # a star that was not injected has no rows
    assert K.fake_match([], lay, 2).shape == (0,)


def test_switches_and_columns(tmp_path):
    import blackbox as cli
    from blackbox_amd import catalogs, fitsio, settings
    assert settings.nfakestars == 0 and settings.fakestar_s2n == 10.0 and settings.fakestar_seed == 0 and settings.fakestar_noise is True
    assert settings.fakestar_radius == 2 and settings.fake_clear_half == 3 and settings.fake_clear_nsigma == 5.0
    a = cli.build_parser().parse_args([])
    assert a.fake_stars is None and a.fake_s2n is None and a.fake_seed is None and a.fake_noise is None and a.fake_radius is None
    a = cli.build_parser().parse_args(['--fake_stars', '4', '--fake_s2n', '3,5,30', '--fake_seed', '7', '--fake_noise', 'False', '--fake_radius', '3',
                                       '--fake_clear_nsigma', '4.5'])
    assert (a.fake_stars, a.fake_s2n, a.fake_seed, a.fake_noise, a.fake_radius, a.fake_clear_nsigma) == (4, (3.0, 5.0, 30.0), 7, False, 3, 4.5)
    rows = [dict(y=1, x=2, scorr=7.0, fpsf=100.0, fpsferr=10.0)]
    assert 'FAKE_STAR' not in catalogs.transient_table(rows) and 'FAKE_STAR' not in catalogs.transient_table([])
    empty = catalogs.transient_table([], fake_star=True)                 # a frame with fake stars and no candidate: the column is there
    assert empty['FAKE_STAR'].shape == (0,) and empty['FAKE_STAR'].dtype == np.int16
    assert catalogs.transient_table(rows, fake_star=True)['FAKE_STAR'].tolist() == [0]
    tab = catalogs.transient_table([dict(rows[0], fake_star=3)])
    assert tab['FAKE_STAR'].tolist() == [3] and tab['FAKE_STAR'].dtype == np.int16
    _, t4 = small_table(4)
    done = catalogs.write_small_products([('fakestars', (t4, str(tmp_path / 'f.fits'), {'T-NFAKE': (4, 'n')})),
                                          ('trans', ([dict(rows[0], fake_star=3)], str(tmp_path / 't.fits'), {})),
                                          ('trans', ([], str(tmp_path / 'e.fits'), {}, dict(fake_star=True)))])
    assert done == [str(tmp_path / 'f.fits'), str(tmp_path / 't.fits'), str(tmp_path / 'e.fits')]
    assert 'FAKE_STAR' in fitsio.read_table(str(tmp_path / 'e.fits'))[0]
    got, hdr = fitsio.read_table(str(tmp_path / 'f.fits'))
    assert tuple(got) == K.FAKE_COLS and got['FOUND'].tolist() == [7, 3, 7, 3]
    assert 'FAKE_STAR' in fitsio.read_table(str(tmp_path / 't.fits'))[0]
    from blackbox_amd import zogy as G
    import inspect
    p = inspect.signature(G._optimal_subtraction).parameters
    assert p['fake_stars'].default == 0 and all(p[k].default is None for k in ('fake_s2n', 'fake_seed', 'fake_noise', 'fake_radius', 'fake_clear_nsigma'))
    assert G.fake_inject is K.fake_inject and G._fake_launch is K.fake_launch and G._fake_recover is K.fake_recover


def test_fake_inject_refuses_first():
    import torch
    from blackbox_amd import zogy as G
    lay = dict(ys=[10, 12], xs=[10, 12], off=np.zeros((2, 2), F), s2n=np.ones(2, F))
    fr = torch.zeros((40, 40))
    cube = torch.zeros((1, 9, 9))
    with pytest.raises(ValueError):                                      # overlapping stamps
        G.fake_inject(None, fr, None, fr, None, None, None, cube, lay, 1, 40)
    with pytest.raises(ValueError):                                      # a frame of another type
        G.fake_inject(None, fr.double(), None, fr, None, None, None, cube, lay, 1, 40)
    with pytest.raises(ValueError):                                      # a mask of another shape
        G.fake_inject(None, fr, None, fr, torch.zeros((40, 41), dtype=torch.uint8), None, None, cube, lay, 1, 40)
    with pytest.raises(ValueError):
        G.fake_recover(None, fr, fr, fr.double(), lay, 2)
    with pytest.raises(ValueError):
        G.fake_recover(None, fr, fr, fr, lay, 5)


def test_library_rejects_bad_arguments_without_gpu():
    from blackbox_amd import _lib
    L = _lib.lib
    n = None
    assert L.bbx_fake_inject(n, 96, 128, n, n, n, n, n, n, 9, 1, n, n, n, 1, n, n, n, n, 3, 5.0, 0, 0, n, n, n, n, n) == -1
    assert L.bbx_fake_recover(n, 96, 128, n, n, n, 1, n, n, 2, n, n) == -1
    # with a context that is never dereferenced before the checks: shapes, forms, null pointers
    ctx_buf, buf = ctypes.create_string_buffer(1 << 20), ctypes.create_string_buffer(4096)
    fake, one = ctypes.cast(ctx_buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p)
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 8, 1, one, n, one, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1      # S even
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 51, 1, one, n, one, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1     # S > 49
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, one, one, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1     # both PSF forms
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, n, n, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1         # neither
    assert L.bbx_fake_inject(fake, 96, 128, one, n, n, n, n, n, 9, 1, one, n, one, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1         # no sigma
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, n, one, 1, one, one, one, one, 5, 5.0, 0, 0, one, one, one, one, n) == -1       # clear_half > S / 2
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, n, one, 1, one, one, one, one, 3, 5.0, 2, 0, one, one, one, one, n) == -1       # noise not 0 / 1
    assert L.bbx_fake_inject(fake, 96, 128, n, n, one, n, n, n, 9, 1, one, n, one, 1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1         # no frame
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, n, one, 1, one, one, one, n, 3, 5.0, 0, 0, one, one, one, one, n) == -1         # no s2n
    assert L.bbx_fake_inject(fake, 96, 128, one, n, one, n, n, n, 9, 1, one, n, one, -1, one, one, one, one, 3, 5.0, 0, 0, one, one, one, one, n) == -1
    assert L.bbx_fake_inject(fake, 96, 128, n, n, one, n, n, n, 9, 1, n, n, one, 0, n, n, n, n, 3, 5.0, 0, 0, n, n, n, n, n) == 0                           # no star: nothing to do
    assert L.bbx_fake_recover(fake, 96, 128, one, one, one, 1, one, one, 5, one, n) == -1                                                                # radius > 4
    assert L.bbx_fake_recover(fake, 96, 128, one, n, one, 1, one, one, 2, one, n) == -1
    assert L.bbx_fake_recover(fake, 96, 128, n, n, n, 0, n, n, 2, n, n) == 0
