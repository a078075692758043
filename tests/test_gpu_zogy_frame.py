"""GPU: bbx_zogy_frame -- the hand-written 2-D FFT path of the ZOGY stage (bbx_zogy3.hip) -- against
the oracle's run_zogy on every sub-image (cut with zero padding, per-sub-image PSFs and
scalars, stitched), for each sub-image side the path is built for (64 = 8*8, 128 = 8*16,
100 = 5*5*4, 140 = 5*7*4; 1400 = 5*7*5*8 is covered at full size in test_gpu_fullsize_zogy.py), with and
without a border (the finite differences then wrap around like np.roll), and against the
rocFFT path (bbx_zogy_subimages) on the same inputs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import zogy_core as Z                       # noqa: E402
from blackbox_amd import reduce as R       # noqa: E402
from blackbox_amd import zogy as G          # noqa: E402
from blackbox_amd._lib import lib, BBX_OPT_ZOGY_KWIN_OFF          # noqa: E402

F = np.float32


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def moffat(S, fwhm, dy=0.0, dx=0.0):
    a = fwhm / (2 * np.sqrt(2 ** (1 / 2.5) - 1))
    y, x = np.mgrid[0:S, 0:S] - S // 2
    p = (1 + ((y - dy) ** 2 + (x - dx) ** 2) / (a * a)) ** -2.5
    return (p / p.sum()).astype(F)


def embed(p, L):
    k = np.zeros((L, L), F); S = p.shape[0]; h = S // 2
    for j in range(S):
        for i in range(S):
            k[(j - h) % L, (i - h) % L] = p[j, i]
    return k


def make(size, border, nsy, nsx, S, seed):
    rs = np.random.RandomState(seed)
    ny, nx = nsy * size, nsx * size
    truth = np.zeros((ny, nx))
    for _ in range(6 * nsy * nsx):
        truth[rs.randint(0, ny), rs.randint(0, nx)] += 10 ** rs.uniform(3, 5)
    from scipy import ndimage
    new = (ndimage.gaussian_filter(truth, 1.6) + rs.normal(0, 14, (ny, nx))).astype(F)
    ref = (ndimage.gaussian_filter(truth, 1.3) + rs.normal(0, 6, (ny, nx))).astype(F)
    new[rs.randint(0, ny), rs.randint(0, nx)] += 4000.0                      # a transient
    sig_n = (14 + 2 * rs.random_sample((ny, nx))).astype(F)
    sig_r = (6 + rs.random_sample((ny, nx))).astype(F)
    nsub = nsy * nsx
    pn = np.stack([moffat(S, 3.4 + 0.1 * k, 0.1 * k, -0.05 * k) for k in range(nsub)])
    pr = np.stack([moffat(S, 2.9 + 0.05 * k) for k in range(nsub)])
    scal = np.stack([[14 + 0.3 * k, 6 + 0.1 * k, 1.0, 0.9 + 0.02 * k, 0.03, 0.02] for k in range(nsub)]).astype(F)
    return new, ref, sig_n, sig_r, pn, pr, scal


def oracle(new, ref, sig_n, sig_r, pn, pr, scal, size, border):
    ny, nx = new.shape
    L = size + 2 * border
    Vn = (np.maximum(new, 0) + sig_n * sig_n).astype(F)
    Vr = (np.maximum(ref, 0) + sig_r * sig_r).astype(F)
    subs = [Z.cut_subimages(a, size, border) for a in (new, ref, Vn, Vr)]
    outs = [[] for _ in range(5)]
    for k in range(subs[0].shape[0]):
        sn, sr, fn, fr, dx, dy = scal[k]
        r = Z.run_zogy(subs[0][k], subs[1][k], embed(pn[k], L), embed(pr[k], L), sn, sr, fn, fr, subs[2][k], subs[3][k], dx, dy)
        for o, a in zip(outs, r):
            o.append(a)
    return [Z.stitch_subimages(np.stack(o), ny, nx, size, border) for o in outs]


@pytest.mark.parametrize('size,border,nsy,nsx,S', [(48, 8, 2, 3, 11), (64, 0, 2, 2, 9), (100, 14, 2, 3, 15), (120, 10, 2, 4, 15), (100, 0, 2, 2, 9),
                                                  (128, 0, 1, 2, 13)])
def test_frame_path_vs_oracle(ctx, size, border, nsy, nsx, S):
    L = size + 2 * border
    assert lib.bbx_zogy_frame_supported(L)
    new, ref, sig_n, sig_r, pn, pr, scal = make(size, border, nsy, nsx, S, seed=L + border)
    want = oracle(new, ref, sig_n, sig_r, pn, pr, scal, size, border)
    got = G.run_zogy_frame(ctx, dev(ctx, new), dev(ctx, ref), dev(ctx, sig_n), dev(ctx, sig_r), dev(ctx, pn), dev(ctx, pr), scal,
                           size, border, want_S=True)
    ctx.sync()
    for name, g, w in zip(('D', 'S', 'Scorr', 'Fpsf', 'Fpsferr'), got, want):
        g = g.cpu().numpy()
        ok = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), ok), name
        # toy frames (a few 10^4 e- peaks over 15 e- of noise): 2e-5 of the image scale, i.e. ~1e-3 of the noise
        scale = np.abs(w[ok]).max()
        assert np.abs(g[ok] - w[ok]).max() <= 2e-5 * scale, (name, np.abs(g[ok] - w[ok]).max(), scale)


def test_frame_path_vs_rocfft_path(ctx):
    """the two device implementations on the same inputs (L = 140: radices 2, 5, 7 like 1400)"""
    size, border, nsy, nsx, S = 120, 10, 2, 4, 15
    L = size + 2 * border
    new, ref, sig_n, sig_r, pn, pr, scal = make(size, border, nsy, nsx, S, seed=5)
    a = G.run_zogy_frame(ctx, dev(ctx, new), dev(ctx, ref), dev(ctx, sig_n), dev(ctx, sig_r), dev(ctx, pn), dev(ctx, pr), scal,
                         size, border, want_S=True)
    dn, dr = dev(ctx, new), dev(ctx, ref)
    Vn, Vr = G.variance(ctx, dn, dev(ctx, sig_n)), G.variance(ctx, dr, dev(ctx, sig_r))
    subs = [G.cut_subimages(ctx, t, size, border) for t in (dn, dr, Vn, Vr)]
    b = G.run_zogy(ctx, subs[0], subs[1], G.embed_psfs(ctx, dev(ctx, pn), L), G.embed_psfs(ctx, dev(ctx, pr), L), subs[2], subs[3], scal)
    b = [G.stitch_subimages(ctx, t, new.shape, size, border) for t in b]
    ctx.sync()
    for name, x, y in zip(('D', 'S', 'Scorr', 'Fpsf', 'Fpsferr'), a, b):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.abs(x - y).max() <= 2e-5 * np.abs(y).max(), name


def test_kernel_row_window_equals_full_transforms(ctx):
    """bbx_zogy_frame takes the matched-filter kernels k_n, k_r through the inverse row pass / squares / forward row pass
    on a window of 2 wh >= 4 S + 32 rows only (they are as compact as the PSF stamps).  With the window switched off
    (BBX_OPT_ZOGY_KWIN_OFF = 1: all L rows, the textbook evaluation) the images agree to float32 rounding --
    far inside the tolerance either holds against the oracle."""
    size, border, nsy, nsx, S = 128, 0, 2, 2, 13               # L = 128: window of 96 rows
    new, ref, sig_n, sig_r, pn, pr, scal = make(size, border, nsy, nsx, S, seed=77)
    args = [dev(ctx, a) for a in (new, ref, sig_n, sig_r, pn, pr)]
    a = [t.cpu().numpy() for t in G.run_zogy_frame(ctx, *args, scal, size, border, want_S=True)]
    assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 1) == 0
    try:
        b = [t.cpu().numpy() for t in G.run_zogy_frame(ctx, *args, scal, size, border, want_S=True)]
    finally:
        assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 0) == 0
    ctx.sync()
    for name, x, y in zip(('D', 'S', 'Scorr', 'Fpsf', 'Fpsferr'), a, b):
        ok = np.isfinite(y)
        assert np.array_equal(np.isfinite(x), ok)
        if name in ('S', 'Fpsf'):
            assert np.array_equal(x[ok], y[ok]), name             # the window only touches V(S) (and D, which shares a transform with it)
        else:
            assert np.abs(x[ok] - y[ok]).max() <= 2e-6 * np.abs(y[ok]).max(), (name, np.abs(x[ok] - y[ok]).max())


def test_kernel_row_window_is_checked_on_the_device(ctx):
    """PSFs whose matched-filter kernel is NOT compact: a point-like new PSF against a 5 x 5 box reference at very low
    reference noise -- k_n^ = |Pr^|^2 / (sn^2 |Pr^|^2 + sr^2) has sharp notches at the zeros of the box's spectrum,
    k_n rings across the whole sub-image.  The energy outside the window is measured in k_psf_cols: the call's step
    is flagged (BBX_ERR_PSFWIN at the next synchronisation) instead of returning a wrong V(S); with the window off the
    same inputs pass."""
    from blackbox_amd._lib import BBXError
    size, border, nsy, nsx, S = 128, 0, 1, 2, 5
    new, ref, sig_n, sig_r, _, _, scal = make(size, border, nsy, nsx, S, seed=3)
    pn = np.zeros((2, S, S), F); pn[:, 2, 2] = 1.0
    pr = np.full((2, S, S), 1.0 / 25, F)
    scal[:, 0], scal[:, 1] = 10.0, 0.01
    args = [dev(ctx, a) for a in (new, ref, sig_n, sig_r, pn, pr)]
    ctx.sync()
    G.run_zogy_frame(ctx, *args, scal, size, border)
    with pytest.raises(BBXError) as ei:
        ctx.sync()
    assert ei.value.code == -6
    ctx.sync()                                                   # the flag was cleared
    assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 1) == 0
    try:
        out = G.run_zogy_frame(ctx, *args, scal, size, border)
        ctx.sync()
        assert torch.isfinite(out[0]).all()
    finally:
        assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 0) == 0


def test_frame_path_rejects_bad_arguments(ctx):
    z = torch.zeros((96, 96), dtype=torch.float32, device=ctx.device)
    p = torch.zeros((4, 9, 9), dtype=torch.float32, device=ctx.device)
    sc = (C.c_float * 24)()
    args = [z.data_ptr()] * 4 + [p.data_ptr()] * 2

    def call(ny, nx, size, border, S=9):
        return lib.bbx_zogy_frame(ctx.h, ny, nx, size, border, *[C.c_void_p(a) for a in args], S, sc,
                                  *[C.c_void_p(z.data_ptr())] * 5, ctx.stream())
    assert call(96, 96, 50, 7) != 0          # frame not a multiple of the sub-image size
    assert call(96, 96, 48, 9) != 0          # L = 66: not a supported side
    assert call(96, 96, 48, 8, S=0) != 0
    assert not lib.bbx_zogy_frame_supported(66) and lib.bbx_zogy_frame_supported(1400)


@pytest.mark.parametrize('size,border,nsy,nsx,S,thr', [(100, 14, 2, 3, 15, 6.0), (64, 0, 2, 2, 9, 3.0), (120, 10, 2, 4, 15, 2.5)])
def test_candidates_listed_by_the_final_kernel_equal_the_peak_search_pass(ctx, size, border, nsy, nsx, S, thr):
    """bbx_zogy_candidates: the pixels with |Scorr| >= thr listed by the kernel that writes Scorr, picked up by bbx_find_peaks on
    that frame -- the same regions and peaks as bbx_find_peaks' own pass over (a copy of) the frame; one-shot and bound to
    the frame and the threshold"""
    from blackbox_amd._lib import check
    new, ref, sig_n, sig_r, pn, pr, scal = make(size, border, nsy, nsx, S, seed=size + 3)
    args = [dev(ctx, a) for a in (new, ref, sig_n, sig_r, pn, pr)]
    check(lib.bbx_zogy_candidates(ctx.h, thr), 'bbx_zogy_candidates')
    try:
        sc = G.run_zogy_frame(ctx, *args, scal, size, border)[2]
        a = G.find_peaks_arrays(ctx, sc, thr)                       # from the list
        b = G.find_peaks_arrays(ctx, sc.clone(), thr)               # another frame: its own pass
        c = G.find_peaks_arrays(ctx, sc, thr)                       # the list is spent: its own pass
        assert a[0].size > 0 and (thr > 3 or a[0].size > 20)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        sc = G.run_zogy_frame(ctx, *args, scal, size, border)[2]
        d = G.find_peaks_arrays(ctx, sc, thr + 1.0)                 # another threshold: its own pass
        e = G.find_peaks_arrays(ctx, sc.clone(), thr + 1.0)
        for x, y in zip(d, e):
            assert np.array_equal(x, y)
    finally:
        check(lib.bbx_zogy_candidates(ctx.h, 0.0), 'bbx_zogy_candidates')


def test_sigma_maps_read_off_their_mini_images(ctx):
    """bbx_zogy_frame_mini / bbx_psf_optflux_mini: the sigma images of the two sides as mini images (new frame: one patch
    per channel, interp_Xchan False; reference: one patch) against the same calls on the full-frame images that
    bbx_spline_zoom makes of the same coefficients -- what rounds 1-4 fed bbx_zogy_frame.  The kernels evaluate the spline
    as a float32 cubic per box interval: the sigma values agree to 3e-7 (relative), the images that come out of the
    transforms to 2e-6 of their scale; and the zoom itself against scipy (the oracle's mini2back) as before."""
    size, border, box, S = 100, 20, 20, 13
    nsy, nsx = 4, 8
    ny, nx = nsy * size, nsx * size
    new, ref, _, _, pn, pr, scal = make(size, border, nsy, nsx, S, 11)
    rs = np.random.RandomState(5)
    nby, nbx = ny // box, nx // box
    yy, xx = np.mgrid[0:nby, 0:nbx]
    mini_n = (14 + 2 * np.sin(yy / 5.0) * np.cos(xx / 7.0) + 0.3 * rs.random_sample((nby, nbx))
              + 1.5 * ((yy // (nby // 2)) * 8 + xx // (nbx // 8)) / 16).astype(F)            # steps between the 16 channels
    mini_r = (6 + np.cos(yy / 6.0 + xx / 9.0) + 0.2 * rs.random_sample((nby, nbx))).astype(F)
    mn = G.MiniImage(ctx, mini_n, box, interp_Xchan=False)
    mr = G.MiniImage(ctx, mini_r, box, interp_Xchan=True)
    assert G.mini_path_supported((ny, nx), size, border, box, mn, mr)
    sig_n, sig_r = mn.frame(ctx), mr.frame(ctx)
    np.testing.assert_allclose(sig_n.cpu().numpy(), Z.mini2back(mini_n, (ny, nx), box, channels=(nby // 2, nbx // 8)), rtol=2.4e-7)
    np.testing.assert_allclose(sig_r.cpu().numpy(), Z.mini2back(mini_r, (ny, nx), box), rtol=2.4e-7)
    d_new, d_ref, d_pn, d_pr = dev(ctx, new), dev(ctx, ref), dev(ctx, pn), dev(ctx, pr)
    want = [o.cpu().numpy() for o in G.run_zogy_frame(ctx, d_new, d_ref, sig_n, sig_r, d_pn, d_pr, scal, size, border, want_S=True)]
    got = [o.cpu().numpy() for o in G.run_zogy_frame(ctx, d_new, d_ref, mn, mr, d_pn, d_pr, scal, size, border, want_S=True)]
    ctx.sync()
    for name, g, w in zip(('D', 'S', 'Scorr', 'Fpsf', 'Fpsferr'), got, want):
        assert np.isfinite(g).all() and np.isfinite(w).all(), name
        scale = np.abs(w).max()
        assert np.abs(g - w).max() <= 2e-6 * scale, (name, float(np.abs(g - w).max() / scale))
    # D does not see the variance images at all: the same transforms of the same pixels (another instantiation of the row
    # kernel: the compiler contracts a few multiply-adds differently, nothing else)
    assert np.abs(got[0] - want[0]).max() <= 1e-6 * np.abs(want[0]).max()
    # the photometry at 300 positions, some at the frame edge (stamps cut) and on channel borders
    ys = np.concatenate([rs.randint(0, ny, 280), [0, 1, ny - 1, ny // 2, ny // 2 - 1] * 4]).astype(np.int32)
    xs = np.concatenate([rs.randint(0, nx, 280), [0, nx - 1, 3, size, size - 1] * 4]).astype(np.int32)
    stamps = dev(ctx, np.stack([moffat(S, 3.0 + 0.01 * (k % 50)) for k in range(ys.size)]))
    f0, e0 = G.psf_optflux(ctx, d_new, sig_n, stamps, ys, xs, v_is_sigma=True)
    f1, e1 = G.psf_optflux(ctx, d_new, mn, stamps, ys, xs, v_is_sigma=True)
    np.testing.assert_allclose(f1.cpu().numpy(), f0.cpu().numpy(), rtol=3e-6, atol=1e-4)
    np.testing.assert_allclose(e1.cpu().numpy(), e0.cpu().numpy(), rtol=1e-6)
    # a geometry the mini path does not take (groups of four pixels not aligned) is refused, not mis-evaluated
    bad = G.MiniImage(ctx, mini_r[:, :-1].copy(), box, interp_Xchan=True)
    assert not G.mini_path_supported((ny, nx), size, border, box, bad)
    rc = lib.bbx_zogy_frame_mini(ctx.h, ny, nx, size, border, G._p(d_new), G._p(d_ref), bad.ref(), mr.ref(), G._p(d_pn), G._p(d_pr), S,
                                 scal.ctypes.data_as(C.POINTER(C.c_float)), *[G._p(dev(ctx, w)) for w in want], ctx.stream())
    assert rc == -1
