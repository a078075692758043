"""CPU: the rules of bbx_limflux_image as restated in limflux_ref.py (analytic value, window, mask), the host logic of
blackbox_amd/limflux.py (header, parameters, refusals), the command line's switches and the magnitude conversion that `_trans_limmag`
and `_red_limmag` share."""
import ctypes

import numpy as np
import pytest

import limflux_ref as L

F = np.float32
GPU_S, GPU_FRAC = (9, 25, 49), (0.0, 1e-4, 0.5)                       # the stamps and fractions of tests/test_gpu_limflux.py


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1.5, 2.5])
def test_gaussian_meets_the_analytic_limit(s):
    """uniform sigma, no mask, a Gaussian stamp: sum P^2 = 1 / (4 pi s^2), so lim = nsigma sigma sqrt(4 pi) s away from the edge"""
    S, n, sg, nsigma = 49, 60, 7.5, 5.0
    r = L.limflux_ref(np.full((n, n), sg, F), None, L.gauss(S, s)[None], n, 1, 1, nsigma=nsigma, frac=0.0)
    want = nsigma * sg * np.sqrt(4.0 * np.pi) * s
    inner = r['lim'][S // 2:n - S // 2, S // 2:n - S // 2]
    assert inner.size and np.abs(inner / want - 1.0).max() <= 1e-6, np.abs(inner / want - 1.0).max()
    assert 1.3 * want < r['lim'][0, 0] < 2.0 * want                   # (in the corner a quarter of the stamp, with its centre lines, is on the frame)
    assert list(r['win']) == [S]


@pytest.mark.parametrize('fwhm, T', [(3.0, 15), (3.6, 19), (4.2, 21), (5.68, 29)])
def test_window_of_a_moffat(fwhm, T):
    Q, ok = L.q_stamp(L.moffat(49, fwhm))
    assert ok and L.window(Q, 1e-4)[0] == T
    assert L.window(Q, 0.0) == (49, np.inf)
    ts = [L.window(Q, f)[0] for f in (0.0, 1e-8, 1e-6, 1e-4, 1e-2, 0.1, 0.5, 0.9, 0.999999)]
    assert all(a >= b for a, b in zip(ts, ts[1:])) and ts[-1] == 1 and all(t % 2 == 1 for t in ts)
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            L.window(Q, bad)


def test_windows_of_the_gpu_tests_are_decided_by_a_margin():
    """every PSF of tests/test_gpu_limflux.py keeps its threshold at least 1e-9 (relative) away from the sums at T and at T - 2: the
    kernel's float64 summation order cannot move T"""
    for S in GPU_S:
        for fw in (2.0, 5.68):
            Q, ok = L.q_stamp(L.moffat(S, fw))
            assert ok
            for frac in GPU_FRAC:
                T, margin = L.window(Q, frac)
                assert margin >= 1e-9, (S, fw, frac, T, margin)
                assert 1 <= T <= S
    # a window smaller than the stamp leaves at most frac of Q out: the limit is high by at most frac / 2
    Q, _ = L.q_stamp(L.moffat(49, 3.6))
    cs = L.central_sums(Q)
    assert 0 <= 1.0 - cs[19 // 2] / cs[-1] <= 1e-4


def test_a_stamp_without_a_sum_gives_zeros():
    planes = np.stack([L.moffat(9, 3.0), np.zeros((9, 9), F), -L.moffat(9, 3.0), np.full((9, 9), np.nan, F)])
    r = L.limflux_ref(np.full((40, 40), 2.0, F), None, planes, 20, 2, 2, frac=1e-4)
    assert list(r['win'][1:]) == [0, 0, 0] and r['win'][0] > 0
    assert (r['lim'][:20, :20] > 0).all() and not r['lim'][20:].any() and not r['lim'][:20, 20:].any()


def test_one_masked_pixel_lowers_den_by_its_term():
    S, n = 25, 64
    P = L.moffat(S, 4.0)
    Q, _ = L.q_stamp(P)
    sg = np.full((n, n), 3.0, F)
    W = F(1.0) / (F(3.0) * F(3.0))
    free = L.limflux_ref(sg, None, P[None], n, 1, 1, frac=0.0)['den']
    mask = np.zeros((n, n), np.uint8)
    mask[30, 33] = 4
    got = L.limflux_ref(sg, mask, P[None], n, 1, 1, frac=0.0)['den']
    for (y, x) in ((30, 33), (28, 30), (20, 40), (32, 33), (40, 23)):
        j, i = 30 - y, 33 - x                                         # the masked pixel sits at (j, i) of the stamp centred on (y, x)
        assert got[y, x] == pytest.approx(free[y, x] - float(Q[S // 2 + j, S // 2 + i]) * float(W), rel=1e-13)
    assert got[30, 33] < free[30, 33] and got[30, 33] > 0              # the masked pixel itself gets the limit of a source centred on it
    assert got[10, 10] == free[10, 10]                                 # out of the stamp's reach: untouched


def test_a_masked_block_wider_than_the_window_gives_zero_inside():
    S, n = 9, 64
    P = L.moffat(S, 3.0)
    mask = np.zeros((n, n), np.uint8)
    mask[20:40, 20:45] = 1
    sg = np.full((n, n), 3.0, F)
    sg[5, 5], sg[6, 6], sg[7, 7] = np.nan, 0.0, -1.0
    r = L.limflux_ref(sg, mask, P[None], n, 1, 1, frac=0.0)
    assert not r['lim'][24:36, 24:41].any() and (r['lim'][23, 24:41] > 0).all() and (r['lim'][24:36, 41] > 0).all()
    assert r['lim'][6, 6] > r['lim'][50, 50] > 0                       # sigma that is not positive and finite carries no weight
    # a sigma whose square underflows: W is the largest float32, the pixels in its reach get a tiny finite limit, the others their own
    sg2 = np.full((n, n), 3.0, F)
    sg2[50, 12] = 1e-25
    assert L.weights(sg2, None)[50, 12] == np.finfo(F).max
    r2 = L.limflux_ref(sg2, None, P[None], n, 1, 1, frac=0.0)
    assert np.isfinite(r2['lim']).all() and 0 < r2['lim'][50, 12] < 1e-15 and 0 < r2['lim'][54, 16] < 1e-12
    assert r2['lim'][55, 12] == r2['lim'][50, 30] == r2['lim'][30, 30] > 1.0


# ---- the host layer ------------------------------------------------------------------------------------------------------
KEYS = ['LIMMAG-P', 'LIMNSIG', 'LIMEFLUX', 'LIMMAG', 'LIMFNU', 'LIMPFRAC', 'LIMWIN', 'LIMNPIX']


def test_header_with_and_without_a_zeropoint():
    from blackbox_amd import limflux as LF
    stat = np.array([12345.0, 600.0, 610.0, 30.0, 0, 0, 0, 0])
    win = np.array([19, 19, 21, 17, 19, 0], np.int32)
    h = LF.limflux_header(True, stat, win, 5.0, 1e-4, exptime=60.0, zp=22.5, ext=0.1)
    assert list(h) == KEYS and all(len(k) <= 8 for k in h)
    mag = 22.5 - 2.5 * np.log10(10.0) - 0.1
    assert h['LIMMAG-P'][0] is True and h['LIMNSIG'][0] == 5.0 and h['LIMEFLUX'][0] == pytest.approx(10.0, rel=1e-15)
    assert h['LIMMAG'][0] == pytest.approx(mag, rel=1e-15) and h['LIMFNU'][0] == pytest.approx(10 ** (-0.4 * (mag - 23.9)), rel=1e-14)
    assert h['LIMPFRAC'][0] == 1e-4 and h['LIMWIN'][0] == 19 and h['LIMNPIX'][0] == 12345
    # LIMWIN is a window side: the lower median of the tiles that have a window
    assert LF.limflux_header(True, stat, [19, 21], 5.0, 1e-4)['LIMWIN'][0] == 19
    assert LF.limflux_header(True, stat, [0, 0, 23, 0], 5.0, 1e-4)['LIMWIN'][0] == 23
    assert LF.limflux_header(True, stat, [0, 0], 5.0, 1e-4)['LIMWIN'][0] == 'None'
    h = LF.limflux_header(True, stat, win, None, None, exptime=60.0)
    assert h['LIMMAG-P'][0] is True and h['LIMEFLUX'][0] == pytest.approx(10.0) and h['LIMMAG'][0] == 'None' and h['LIMFNU'][0] == 'None'
    assert h['LIMNSIG'][0] == 5.0 and h['LIMPFRAC'][0] == 1e-4            # the settings
    h = LF.limflux_header(True, stat, win, 5.0, 1e-4)                   # no exposure time: the tensor-level call
    assert h['LIMMAG-P'][0] is True and h['LIMEFLUX'][0] == 'None' and h['LIMNPIX'][0] == 12345
    for bad in (LF.limflux_header(False), LF.limflux_header(True, None, None), LF.limflux_header(True, np.zeros(8), win, 5.0, 1e-4, exptime=60.0),
                LF.limflux_header(True, np.array([5, np.nan, 0, 0, 0, 0, 0, 0.0]), win, 5.0, 1e-4, exptime=60.0, zp=22.5)):
        assert list(bad) == KEYS and bad['LIMMAG-P'][0] is False and all(bad[k][0] == 'None' for k in KEYS[1:])


def test_settings_parser_and_parameters():
    from blackbox_amd import limflux as LF, settings as S
    import test_cli_entry as CE
    assert S.limmag is False and S.limmag_nsigma == 5.0 and S.limmag_psf_frac == 1e-4
    ap = CE.load_cli().build_parser()
    a = ap.parse_args([])
    assert a.limmag is None and a.limmag_nsigma is None and a.limmag_psf_frac is None          # unset: the settings apply
    a = ap.parse_args(['--limmag', 'True', '--limmag_nsigma', '3', '--limmag_psf_frac', '0'])
    assert a.limmag is True and a.limmag_nsigma == 3.0 and a.limmag_psf_frac == 0.0
    assert LF.check_parameters() == (5.0, 1e-4) and LF.check_parameters(3, 0) == (3.0, 0.0)
    for frac in (1.0, -1e-9, 2.0, float('nan')):
        with pytest.raises(ValueError):
            LF.check_parameters(None, frac)
    for nsig in (0.0, -5.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            LF.check_parameters(nsig, None)


def test_wrapper_refuses_before_the_library():
    torch = pytest.importorskip('torch')
    from blackbox_amd import limflux as LF

    class Ctx:
        device, h = 'cpu', None

        def stream(self):
            raise AssertionError('the library was reached')
    sg, planes = torch.ones((40, 50)), torch.ones((4, 9, 9))
    ok = dict(sigma=sg, mask=None, sub_psfs=planes, size=25, nsy=2, nsx=2)
    for change in (dict(sigma=sg.double()), dict(sigma=sg.t()), dict(sigma=sg[0]), dict(mask=torch.zeros((40, 50))),
                   dict(mask=torch.zeros((40, 49), dtype=torch.uint8)), dict(sub_psfs=planes.double()), dict(sub_psfs=planes[:3]),
                   dict(sub_psfs=planes[:, :, :8]), dict(sub_psfs=torch.ones((4, 8, 8))), dict(sub_psfs=torch.ones((4, 51, 51))),
                   dict(sub_psfs=torch.ones((9, 9, 4)).permute(2, 0, 1)),dict(sub_psfs=torch.ones((4, 81))), dict(nsy=0), dict(size=0),
                   dict(frac=1.0), dict(frac=-0.5), dict(nsigma=0.0)):
        with pytest.raises(ValueError):
            LF.limflux_image(Ctx(), **dict(ok, **change))


def test_library_rejects_bad_arguments_without_gpu():
    """BBX_ERR_ARG before anything touches the context or the device (the context below is a block of zeros); an empty frame is done
    without a launch"""
    from blackbox_amd import _lib
    lib = _lib.lib
    fake = ctypes.create_string_buffer(1 << 20)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    mini = ctypes.byref(_lib.SplineImage())

    def call(c=ctx, ny=64, nx=64, sigma=p, mini=None, S=9, planes=p, size=32, nsy=2, nsx=2, nsigma=5.0, frac=1e-4, lim=p):
        return lib.bbx_limflux_image(c, ny, nx, sigma, mini, None, S, planes, size, nsy, nsx, nsigma, frac, lim, None, None)
    assert call(c=None) == -1
    assert call(sigma=None) == -1 and call(mini=mini) == -1           # neither form of the sigma map, both
    assert call(S=8) == -1 and call(S=51) == -1 and call(S=0) == -1 and call(S=-3) == -1
    assert call(frac=1.0) == -1 and call(frac=-1e-9) == -1 and call(frac=float('nan')) == -1
    assert call(nsigma=0.0) == -1 and call(nsigma=float('nan')) == -1
    assert call(size=0) == -1 and call(nsy=0) == -1 and call(nsx=0) == -1 and call(ny=-1) == -1
    assert call(planes=None) == -1 and call(lim=None) == -1
    assert call(sigma=None, mini=mini) == -1                          # a mini image that tiles no frame
    assert call(ny=0) == 0 and call(nx=0, planes=None, lim=None) == 0  # nothing to do, nothing launched


def test_the_shared_magnitude_conversion_is_write_limmags():
    """limit_magnitudes, which `_trans_limmag` and `_red_limmag` go through, against the expression write_limmag carried before"""
    torch = pytest.importorskip('torch')
    from blackbox_amd import limflux as LF
    lim = torch.tensor([[0.0, 1.0, 37.5, 6.0e4], [-2.0, 1e-35, 812.25, 3.3e9]], dtype=torch.float32)
    zp, exptime, ext = 22.5, 60.0, 0.0675
    got = LF.limit_magnitudes(lim, zp, exptime, ext)
    old = torch.where(lim > 0, zp - 2.5 * torch.log10(lim.clamp(min=1e-30) / exptime) - ext, torch.zeros_like(lim))
    assert got.dtype == torch.float32 and torch.equal(got, old)
    v = lim.numpy().astype(np.float64)
    want = np.where(v > 0, zp - 2.5 * np.log10(np.maximum(v, 1e-30) / exptime) - ext, 0.0)
    assert np.abs(got.numpy() - want).max() <= 4e-6 * np.abs(want).max()
    assert got[0, 0] == 0 and got[1, 0] == 0 and got[0, 2] == pytest.approx(22.5 - 2.5 * np.log10(37.5 / 60.0) - 0.0675, rel=1e-6)
    assert torch.equal(LF.limit_magnitudes(lim, zp, exptime), torch.where(lim > 0, zp - 2.5 * torch.log10(lim.clamp(min=1e-30) / exptime) - 0.0,
                                                                          torch.zeros_like(lim)))
