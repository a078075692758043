"""Catalogue photometry with the PSF on the centroid, host side (no GPU): the restatement of psfphot_ref.py (the definition the
GPU tests compare bbx_psf_optflux_shift with) against conditions on noise-free stars -- the bias of the unshifted estimator, what
the shift leaves of it, what the mask does -- its float32 run against its float64 run on the cases of the kernel tests; the
setting, the command-line switch, the catalogue column and the library's argument checks.

Every bound below that is not set by the issue is 2 x what the float64 restatement itself gives on the very inputs of the test
(measured on a CPU with numpy; the margin covers nothing but a change of the scene), and says so."""
import numpy as np
import pytest

import psfphot_ref as R
import test_psfbuild_host as P

F = np.float32
S = P.V                                                              # 21
OFFS = ((0.5, 0.5), (0.25, -0.4), (-0.5, 0.1), (0.0, 0.5), (0.33, 0.33))
XS = (0, 240, 480)                                                   # FWHM 3.0, 3.6, 4.2 (test_psfbuild_host.fwhm_at)
# the restatement's worst |flux / truth - 1| with the shifted PSF over XS x OFFS: 0.00416 (FWHM 3.0 at (0.5, 0.5)); FWHM 3.6:
# 0.00309, FWHM 4.2: 0.00263.  What is left is LANCZOS3's interpolation error of a critically sampled profile
SHIFT_BOUND = 2 * 0.00416
# there and back, FWHM 3.5: the worst |difference| / peak over OFFS is 1.145e-2 (at (0.5, 0.5))
ROUND_TRIP_BOUND = 2 * 1.145e-2


def star(x, dy, dx, flux=1000.0, n=41):
    """a noise-free, point-sampled star of truth_stamp's profile at (20 + dy, 20 + dx) of an n x n frame, sigma = 10: V = max(D,
    0) + 100"""
    D = np.zeros((n, n))
    c = n // 2
    D[c - S // 2:c + S // 2 + 1, c - S // 2:c + S // 2 + 1] = flux * P.truth_stamp(x, S, dy, dx)
    return D.astype(F), np.full((n, n), 10.0, F), c


def measure(D, sig, c, cube, off, mask=None, dtype=np.float64):
    f, e, g = R.optflux_shift_ref(D, sig, mask, cube, None, [0], [c], [c], np.asarray([off], F), dtype)
    return f[0], e[0], int(g[0])


def test_zero_offset_is_the_plain_optimal_flux():
    sc = P.make_scene()
    img = np.nan_to_num(sc['img'])
    sig = np.full(img.shape, P.SKY, F)
    ys, xs = np.round(sc['sy'][:40]).astype(int), np.round(sc['sx'][:40]).astype(int)
    cube = np.stack([P.truth_stamp(x).astype(F) for x in xs])
    f, e, g = R.optflux_shift_ref(img, sig, None, cube, None, np.arange(40), ys, xs, np.zeros((40, 2), F))
    for k in range(40):
        p = cube[k].astype(np.float64)
        fp, ep = R.plain_optflux(img, sig, p / p.sum(), int(ys[k]), int(xs[k]))
        assert abs(f[k] / fp - 1) < 1e-12 and abs(e[k] / ep - 1) < 1e-12
    assert not g.any()
    # ... and the stamp itself keeps its bits, in either arithmetic, also where an integer shift is asked for
    st = cube[0]
    assert R.shift_stamp(st, 0.0, 0.0, np.float32).tobytes() == st.tobytes()
    moved = R.shift_stamp(st, 2.0, -3.0, np.float32)
    assert moved[2:, :-3].tobytes() == st[:-2, 3:].tobytes() and not moved[:2].any() and not moved[:, -3:].any()


def test_shift_there_and_back():
    st = R.moffat_stamp(S, 3.5)
    worst = 0.0
    for dy, dx in OFFS:
        back = R.shift_stamp(R.shift_stamp(st, dy, dx), -dy, -dx)
        d = float(np.abs(back - st).max() / st.max())
        print('(%+.2f, %+.2f): |there and back - stamp| / peak %.3e' % (dy, dx, d))
        worst = max(worst, d)
    assert worst <= ROUND_TRIP_BOUND
    # one shift against the profile sampled at the shifted position
    for dy, dx in OFFS:
        d = float(np.abs(R.shift_stamp(st, dy, dx) - R.moffat_stamp(S, 3.5, dy, dx)).max() / st.max())
        print('(%+.2f, %+.2f): |shifted - sampled there| / peak %.3e' % (dy, dx, d))
        assert d <= ROUND_TRIP_BOUND


def test_bias_table():
    worst = 0.0
    for x in XS:
        cube = P.truth_stamp(x, S)[None].astype(F)
        row = []
        for dy, dx in OFFS:
            D, sig, c = star(x, dy, dx)
            f0 = measure(D, sig, c, cube, (0.0, 0.0))[0] / 1000.0 - 1.0
            f1 = measure(D, sig, c, cube, (dy, dx))[0] / 1000.0 - 1.0
            row.append((f0, f1))
            worst = max(worst, abs(f1))
            assert abs(f1) <= SHIFT_BOUND, (x, dy, dx, f1)
        print('FWHM %.1f  unshifted / shifted: ' % P.fwhm_at(x) + '  '.join('%+.4f / %+.5f' % t for t in row))
        assert row[0][0] < -0.03, (x, row[0][0])                     # the integer-peak PSF at (0.5, 0.5): low by more than 3 %
    print('worst shifted error %.5f, bound %.5f' % (worst, SHIFT_BOUND))


def test_masked_spike():
    """a 10^4 e- spike at (+2, +1) of the peak, 2.2 px from the centroid of a FWHM 3.6 star: outside the half-maximum radius;
    further out the estimator protects itself, V = max(D, 0) + sigma^2 carries the spike (at 4.6 px it moves the flux by 2 %)"""
    x, off = 240, (0.25, -0.4)
    cube = P.truth_stamp(x, S)[None].astype(F)
    D, sig, c = star(x, *off)
    clean = measure(D, sig, c, cube, off)
    D[c + 2, c + 1] += F(1e4)
    mask = np.zeros(D.shape, np.uint8)
    mask[c + 2, c + 1] = 16
    with_mask, without = measure(D, sig, c, cube, off, mask), measure(D, sig, c, cube, off)
    print('flux / clean - 1: masked %+.2e, unmasked %+.4f; bound %.5f' % (with_mask[0] / clean[0] - 1, without[0] / clean[0] - 1, SHIFT_BOUND))
    assert abs(with_mask[0] / clean[0] - 1) < SHIFT_BOUND and abs(with_mask[0] / 1000.0 - 1) < SHIFT_BOUND
    assert with_mask[2] == R.MASKED and without[2] == 0 and clean[2] == 0
    assert abs(without[0] / clean[0] - 1) > 10 * SHIFT_BOUND
    assert with_mask[1] > clean[1]                                   # fewer pixels: a larger error


def test_no_centroid_and_no_sum():
    x = 240
    cube = P.truth_stamp(x, S)[None].astype(F)
    D, sig, c = star(x, 0.3, 0.2)
    ref = measure(D, sig, c, cube, (0.0, 0.0))
    for off in ((np.nan, 0.1), (0.1, np.inf), (16.5, 0.0), (0.0, -17.0)):
        got = measure(D, sig, c, cube, off)
        assert got[2] == R.NO_CENTROID and got[:2] == ref[:2]
    assert measure(D, sig, c, cube, (16.0, -16.0))[2] == 0            # 16 px is still a centroid (the stamp is then shifted out: flux 0)
    assert measure(D, sig, c, 0 * cube, (0.0, 0.0)) == (0.0, 0.0, R.NO_SUM)
    D[c, c] = np.nan                                                 # a dead pixel is skipped, the flux stays finite
    assert np.isfinite(measure(D, sig, c, cube, (0.3, 0.2))[0])


@pytest.fixture(scope='module')
def case_runs():
    out = []
    for c in R.CASES:
        case = R.make_case(*c)
        sg = R.sigma_frame(case)
        out.append((c, R.run_case(case, np.float64, sg), R.run_case(case, np.float32, sg)))
    return out


def test_float32_follows_float64(case_runs):
    worst = 0.0
    for c, (f64, e64, g64), (f32, e32, g32) in case_runs:
        assert np.array_equal(g64, g32)
        ok = e64 > 0
        assert ok.all() and (f64 > 5 * e64).all(), c                # every source is a star: a relative flux difference means something
        d = max(float(np.abs(f32 / f64 - 1).max()), float(np.abs(e32 / e64 - 1).max()))
        print(c, 'd32 %.2e' % d)
        worst = max(worst, d)
    print('worst %.3e; D32 %.1e, tolerance of the GPU tests %.2e' % (worst, R.D32, R.TOL))
    assert worst <= R.D32 and R.TOL == 4 * R.D32


def test_cases_cover_what_they_should(case_runs):
    flags = np.concatenate([r[1][2] for r in case_runs])
    assert (flags & R.NO_CENTROID).any() and (flags & R.MASKED).any() and (flags == 0).any()
    hits = [r for r in case_runs if r[0][4] == 'hits']
    assert all((r[1][2] & R.MASKED).any() and not (r[1][2] & R.MASKED).all() for r in hits if r[0][3] > 1)
    assert {c[0] for c in R.CASES} == {5, 21, 49} and {c[1] for c in R.CASES} == {'plane', 1, 6, 10}
    assert {c[2] for c in R.CASES} == {'frame', 'mini_x', 'mini_c'} and {c[3] for c in R.CASES} == {1, 65, 300}
    assert {c[4] for c in R.CASES} == {None, 'zero', 'hits'}


def test_setting_switch_and_column(tmp_path):
    from blackbox_amd import settings as ST, catalogs, fitsio
    assert ST.phot_centroid is False
    import test_cli_entry as CE
    ap = CE.load_cli().build_parser()
    assert ap.parse_args(['--image', 'x.fits']).phot_centroid is None
    assert ap.parse_args(['--image', 'x.fits', '--phot_centroid', 'True']).phot_centroid is True
    assert ap.parse_args(['--image', 'x.fits', '--phot_centroid', 'False']).phot_centroid is False
    base = dict(X_POS=np.array([1.5, 2.5], F), Y_POS=np.array([3.0, 4.0], F), E_FLUX_PEAK=np.ones(2, F), E_FLUX_OPT=np.ones(2, F),
                E_FLUXERR_OPT=np.ones(2, F), SNR_OPT=np.ones(2, F))
    names = [c[0] for c in catalogs.COLUMNS['new']]
    a, _ = fitsio.read_table(catalogs.format_cat(dict(base), str(tmp_path / 'a.fits')))
    assert list(a) == names
    b, _ = fitsio.read_table(catalogs.format_cat(dict(base, FLAGS_OPT=np.array([0, 3], np.uint8)), str(tmp_path / 'b.fits')))
    assert list(b) == names + ['FLAGS_OPT'] and b['FLAGS_OPT'].dtype == np.uint8 and b['FLAGS_OPT'].tolist() == [0, 3]
    sh = {k[0]: np.zeros(2, k[1]) for k in catalogs.SHAPE_COLUMNS}
    c, _ = fitsio.read_table(catalogs.format_cat(dict(base, FLAGS_OPT=np.array([0, 3], np.uint8), **sh), str(tmp_path / 'c.fits')))
    assert list(c) == names + [k[0] for k in catalogs.SHAPE_COLUMNS] + ['FLAGS_OPT']
    d, _ = fitsio.read_table(catalogs.format_cat(None, str(tmp_path / 'd.fits')))
    assert list(d) == names                                          # the dummy catalogue keeps its seven


def test_ref_catalog_tells_the_two_photometries_apart():
    from blackbox_amd import zogy as G
    rc = object.__new__(G.RefCatalog)
    ref = __import__('torch').zeros((4, 4))
    rc.ref, rc.sig_ref, rc.geom = ref, ref, (4, 4, 2, 1)
    for made_with in (False, True):
        rc.phot_centroid = made_with
        assert rc.matches(ref, ref, 2, 1, phot_centroid=made_with) and not rc.matches(ref, ref, 2, 1, phot_centroid=not made_with)
    rc.phot_centroid = False
    assert rc.matches(ref, ref, 2, 1)                                # the call of before


def test_library_rejects_bad_arguments_without_gpu():
    import ctypes
    from blackbox_amd._lib import lib, SplineImage
    n = None
    c = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)      # in the context's place: never dereferenced before the checks
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)

    def call(ctx=c, ny=96, nx=128, D=p, sigma=p, mini=n, mask=n, S=21, nplane=6, cube=p, terms=p, idx=n, nsrc=3, ys=p, xs=p, off=p, flux=p,
             err=p, flags=p):
        return lib.bbx_psf_optflux_shift(ctx, ny, nx, D, sigma, mini, mask, S, nplane, cube, terms, idx, nsrc, ys, xs, off, flux, err, flags, n)
    assert call(ctx=n) == -1
    for S_ in (20, 0, 51, -3):                                       # even, empty, above the LDS maximum
        assert call(S=S_) == -1
    assert call(nplane=65) == -1 and call(nplane=0) == -1            # ncoef > 64
    assert call(nsrc=-1) == -1 and call(ny=0) == -1 and call(nx=0) == -1
    assert call(terms=n) == -1 and call(idx=p) == -1                 # neither form, both forms
    assert call(sigma=n) == -1                                       # neither sigma
    mini = SplineImage(p.value, 6, 8, 6, 8, 16, 6)
    assert call(mini=ctypes.byref(mini)) == -1                       # both
    bad = SplineImage(p.value, 6, 7, 6, 7, 16, 6)                    # does not tile the frame
    assert call(sigma=n, mini=ctypes.byref(bad)) == -1
    for k in ('D', 'cube', 'ys', 'xs', 'off', 'flux', 'err', 'flags'):
        assert call(**{k: n}) == -1, k
    # nothing to do: no launch, whatever the pointers; a plane form may have more than 64 planes
    assert call(nsrc=0, D=n, cube=n, ys=n, xs=n, off=n, flux=n, err=n, flags=n) == 0
    assert call(nsrc=0, terms=n, idx=p, nplane=500) == 0
    assert call(nsrc=0, sigma=n, mini=ctypes.byref(mini), mask=p) == 0
