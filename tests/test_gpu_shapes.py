"""GPU: source shapes of the catalogue (bbx_shapes.hip; include/bbx.h: bbx_src_shapes, bbx_shape_stats) against the numpy
restatements of test_shapes_host.py; optimal_subtraction(cat_extract=True, shapes=True) end to end on the scene of
test_match_host.py; the command line and the frames-in-flight list run with --cat_shapes.

Tolerance of the moments (TOL below): max(16 d32, 2e-5) relative, d32 = the float32 restatement's own distance from the float64
one on the very inputs of the test; 2e-5 is the project's centroid bound, the factor 16 covers expf and a sum order other than
numpy's.  What is derived from the moments is bounded by propagating that (see derived_bounds)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import test_match_host as H                   # noqa: E402  (the scene, the centroid restatement)
import test_shapes_host as S                  # noqa: E402  (the shape restatements)
import test_gpu_match as M                    # noqa: E402  (the special cases of the centroid test, the subtraction's inputs)
from test_gpu_match import ctx, scene, centroid_case          # noqa: E402,F401  (fixtures)
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402
from blackbox_amd._lib import lib             # noqa: E402

F = np.float32
NSUB = H.NSY * H.NSX
dev = M.dev
GAUSS = ((30.3, 440.8, 0.5), (120.6, 225.2, 2.2), (215.1, 331.5, -0.9))          # added elliptical Gaussians (y, x, theta)


@pytest.fixture(scope='module')
def shape_case(centroid_case):
    """the centroid test's frame and sources (stars in the corners and on the edges, a patch of zeros, one of negatives, a NaN
    pixel) + three bright elliptical Gaussians (sigma 2.0 x 1.4) + one source whose d_off is NaN; a mask with set bits under
    some windows, one of them partly off the frame; the centroids (float64 restatement, as float32) per window radius"""
    img, ys, xs, sigw, knan = centroid_case
    img = img.astype(np.float64)
    ny, nx = img.shape
    for y, x, th in GAUSS:
        img += S.gaussian(ny, nx, y, x, 2.0, 1.4, th, flux=3e5)[0]
    ys = np.concatenate([ys, [int(round(g[0])) for g in GAUSS]]).astype(np.int32)
    xs = np.concatenate([xs, [int(round(g[1])) for g in GAUSS]]).astype(np.int32)
    img = img.astype(F)
    mask = np.zeros(img.shape, np.uint8)
    mask[0, 3], mask[ny - 1, nx - 2], mask[100, 5] = 1, 4, 32                    # under the windows of the corner / edge stars
    mask[ys[-2] + 10, xs[-2] - 10] = 64                              # the corner pixel of a radius-10 window: outside a radius-6 one
    mask[ys[7] - 2, xs[7] + 1] |= 2
    mask[ys[7] + 1, xs[7]] |= 16
    mask[62, 38] = 8                                                 # in the window of the source in the patch of zeros, which fails
    knanoff = 3                                                      # an ordinary source that is given a NaN offset
    offs = {}
    for radius in (6, 10):
        off = H.win_centroid_ref(img, ys, xs, sigw, H.SIZE, H.NSY, H.NSX, radius, 8).astype(F)
        off[knanoff] = np.nan, 0.1
        offs[radius] = off
    n = len(ys)
    first = [knanoff, n - 13, n - 5, n - 4, n - 1]                   # NaN offset, a corner, zeros, negatives, a Gaussian
    order = np.array(first + [k for k in range(n) if k not in first])
    return dict(img=img, ys=ys, xs=xs, sigw=sigw, knan=knan, knanoff=knanoff, mask=mask, offs=offs, order=order, n=n)


def gpu_shapes(ctx, c, radius, niter, sel=None, mask=True):
    sel = np.arange(c['n']) if sel is None else sel
    out, fl = G.src_shapes(ctx, dev(ctx, c['img']), dev(ctx, c['mask']) if mask else None, dev(ctx, c['ys'][sel]), dev(ctx, c['xs'][sel]),
                           dev(ctx, c['offs'][radius][sel]), dev(ctx, c['sigw']), H.SIZE, H.NSY, H.NSX, radius, niter)
    ctx.sync()
    return out.cpu().numpy(), fl.cpu().numpy()


def derived_bounds(want, tol):
    """bounds on FWHM, ELONGATION (relative) and THETA (degrees) that follow from |d Tyy|, |d Txx| <= tol T, |d Txy| <= tol T,
    T = max(Tyy, Txx): tr = Tyy + Txx and df = Txx - Tyy move by <= 2 tol T; rad = sqrt(df^2 + 4 Txy^2) is 1-Lipschitz in
    (df, 2 Txy): <= 2 sqrt(2) tol T; A^2, B^2 = (tr +- rad) / 2 by <= 2.42 tol T, T <= A^2 = e^2 B^2.
    FWHM ~ sqrt(tr): relative tol.  e = sqrt(A^2 / B^2): relative <= 1.21 tol (1 + e^2).  THETA = 1/2 atan2(2 Txy, df):
    <= 1/2 * 2 sqrt(2) tol T / rad radians"""
    Tyy, Txx, Txy, e = want[:, 2], want[:, 3], want[:, 4], want[:, 6]
    T = np.maximum(Tyy, Txx)
    rad = np.sqrt((Txx - Tyy) ** 2 + 4 * Txy ** 2)
    with np.errstate(divide='ignore'):
        return tol, 1.25 * tol * (1 + e * e), np.degrees(np.sqrt(2.0) * tol * T / rad)


def compare_shapes(got, want, tol, label):
    """rows of bbx_src_shapes against the float64 restatement -> the largest relative difference of Tyy, Txx"""
    nan = np.isnan(want[:, 0])
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    g, w = got[~nan].astype(np.float64), want[~nan]
    T = np.maximum(w[:, 2], w[:, 3])
    dT = np.abs(g[:, 2:4] / w[:, 2:4] - 1).max()
    dxy = (np.abs(g[:, 4] - w[:, 4]) / T).max()
    dc = np.abs(g[:, 0:2] - w[:, 0:2]).max()
    b_fw, b_el, b_th = derived_bounds(w, tol)
    d_fw, d_el = np.abs(g[:, 5] / w[:, 5] - 1), np.abs(g[:, 6] / w[:, 6] - 1)
    print('%s: %d sources, %d NaN rows; gpu against float64: Tyy, Txx %.3g relative, Txy %.3g of T, centre %.3g px, FWHM %.3g, '
          'ELONGATION %.3g (tolerance %.3g)' % (label, len(want), nan.sum(), dT, dxy, dc, d_fw.max(), d_el.max(), tol))
    assert dT <= tol and dxy <= tol, label
    assert dc <= 2e-5, label
    assert (d_fw <= b_fw).all() and (d_el <= b_el).all(), label
    return dT, g, w, b_th


# ---- bbx_src_shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius,niter', [(6, 8), (10, 8), (6, 1), (10, 1)])
def test_shapes_meet_the_float64_restatement(ctx, shape_case, radius, niter):
    c = shape_case
    n = c['n']
    args = (c['img'], c['ys'], c['xs'], c['offs'][radius], c['sigw'], H.SIZE, H.NSY, H.NSX, radius, niter)
    want = S.shapes_ref(*args, np.float64)
    w32 = S.shapes_ref(*args, np.float32)
    assert np.array_equal(np.isnan(w32), np.isnan(want))             # (else the comparison below would not be decisive)
    d32 = np.nanmax(np.abs(w32[:, 2:4].astype(np.float64) / want[:, 2:4] - 1))
    tol = max(16 * d32, 2e-5)
    got, fl = gpu_shapes(ctx, c, radius, niter)
    again, fl2 = gpu_shapes(ctx, c, radius, niter)
    assert got.tobytes() == again.tobytes() and fl.tobytes() == fl2.tobytes()                  # two runs: the same bits
    print('R %d niter %d: float32 restatement against float64 d32 = %.3g' % (radius, niter, d32))
    dT, g, w, b_th = compare_shapes(got, want, tol, 'R %d niter %d' % (radius, niter))
    nan = np.isnan(want[:, 0])
    assert nan[c['knanoff']] and nan[c['knan']] and nan[n - 4] and nan[n - 5]                  # NaN offset, NaN pixel, negatives, zeros
    assert not nan[n - 13:n - 5].any()                               # corners and edges: the window partly off the frame
    assert not nan[n - 3:].any()
    # the added Gaussians: elongation 2.0 / 1.4 >= 1.2 and their angle
    isg = np.isin(np.nonzero(~nan)[0], np.arange(n - 3, n))         # (rows of g, w: the sources with a shape)
    assert isg.sum() == 3 and (w[isg, 6] >= 1.2).all()
    dth = np.abs((g[:, 7] - w[:, 7] + 90.0) % 180.0 - 90.0)
    print('THETA of the Gaussians: max difference %.3g deg (bound %.3g); elongation %s, theta %s (made with %s)' %
          (dth[isg].max(), b_th[isg].min(), np.round(g[isg, 6], 4).tolist(), np.round(g[isg, 7], 3).tolist(),
           [round(float(np.degrees(t[2])), 3) for t in GAUSS]))
    assert (dth[isg] <= b_th[isg] + 1e-5).all()
    if niter == 8:                                                   # converged: the covariance the Gaussians were made with
        for k, (_, _, th) in zip(np.nonzero(isg)[0], GAUSS):
            assert abs(g[k, 6] / (2.0 / 1.4) - 1) < 0.02 and abs((g[k, 7] - np.degrees(th) + 90.0) % 180.0 - 90.0) < 1.0
    # flags: the OR over the window on the frame, for failed sources too; a NULL mask gives 0
    assert np.array_equal(fl, S.flags_ref(c['mask'], c['ys'], c['xs'], radius))
    assert fl[n - 13] & 1 and fl[n - 10] & 4 and fl[7] & 18 == 18 and (fl[n - 2] & 64 != 0) == (radius == 10)
    assert nan[n - 5] and fl[n - 5] == 8                             # (a failed source carries its flags)
    got0, fl0 = gpu_shapes(ctx, c, radius, niter, mask=False)
    assert got0.tobytes() == got.tobytes() and not fl0.any()
    # any number of sources: the same rows (1, 3, 5: part of a workgroup of four waves, and one wave into the next)
    for nsrc in (1, 3, 5):
        sel = c['order'][:nsrc]
        part, pfl = gpu_shapes(ctx, c, radius, niter, sel=sel)
        assert part.tobytes() == got[sel].tobytes() and np.array_equal(pfl, fl[sel]), nsrc


def test_shapes_arguments(ctx):
    t = torch.zeros(64, dtype=torch.float32, device=ctx.device)
    p = t.data_ptr()

    def call(ny=4, nx=4, img=p, mask=None, n=1, ys=p, xs=p, off=p, sw=p, size=5, nsy=1, nsx=1, radius=6, niter=8, out=p, fl=p, c=ctx.h):
        return lib.bbx_src_shapes(c, ny, nx, img, mask, n, ys, xs, off, sw, size, nsy, nsx, radius, niter, out, fl, None)
    assert call(n=0, img=None, ys=None, xs=None, off=None, sw=None, out=None, fl=None) == 0        # nothing to do
    assert call(radius=11) == -1 and call(radius=0) == -1 and call(niter=0) == -1
    for name in ('img', 'ys', 'xs', 'off', 'sw', 'out', 'fl'):
        assert call(**{name: None}) == -1, name
    assert call(c=None) == -1 and call(n=-1) == -1 and call(size=0) == -1
    assert call() == 0                                               # (a 4 x 4 frame of zeros, peak (0, 0): a NaN row)
    ctx.sync()

    def stats(n=1, ys=p, xs=p, sh=p, fl=p, f=p, e=p, size=5, nsy=1, nsx=1, out=p, c=ctx.h):
        return lib.bbx_shape_stats(c, n, ys, xs, sh, fl, f, e, size, nsy, nsx, 20.0, out, None)
    assert stats(n=0, ys=None, xs=None, sh=None, fl=None, f=None, e=None, out=None) == 0
    for name in ('ys', 'xs', 'sh', 'fl', 'f', 'e', 'out'):
        assert stats(**{name: None}) == -1, name
    assert stats(c=None) == -1 and stats(n=-1) == -1 and stats(size=0) == -1 and stats(nsy=0) == -1
    assert stats() == 0
    ctx.sync()


# ---- bbx_shape_stats -----------------------------------------------------------------------------------------------
def shape_lists(rs, counts, size, nsx, bad=4):
    """a (y, x)-sorted list with counts[k] qualifying sources in tile k, 10 % of them outliers, + [bad] sources per tile failing
    each rule: a flag, S/N below 20, err <= 0, a NaN FWHM, an infinite ELONGATION"""
    ys, xs, fw, el, fl, f, e = [], [], [], [], [], [], []
    for k, n in enumerate(counts):
        ty, tx = divmod(k, nsx)
        m = n + 5 * bad if n else 5 * bad
        y, x = rs.randint(ty * size, (ty + 1) * size, m), rs.randint(tx * size, (tx + 1) * size, m)
        out = rs.rand(m) < 0.1
        w = rs.normal(4.0 + 0.1 * k, 0.15, m) + np.where(out, 2.5, 0.0)
        l = 1.0 + np.abs(rs.normal(0, 0.04, m)) + np.where(out, 0.8, 0.0)
        g, fx = np.zeros(m, np.uint8), 10 ** rs.uniform(3, 5, m)
        ex = fx / rs.uniform(25, 80, m)
        for j in range(5):
            sl = slice(n + j * bad, n + (j + 1) * bad)
            if j == 0:
                g[sl] = [1, 2, 64, 255][:bad]
            elif j == 1:
                ex[sl] = fx[sl] / 19.5
            elif j == 2:
                ex[sl] = [0.0, -1.0, 0.0, -5.0][:bad]
            elif j == 3:
                w[sl] = np.nan
            else:
                l[sl] = np.inf
        ys.append(y); xs.append(x); fw.append(w); el.append(l); fl.append(g); f.append(fx); e.append(ex)
    ys, xs, fw, el, fl, f, e = [np.concatenate(t) for t in (ys, xs, fw, el, fl, f, e)]
    o = np.lexsort((xs, ys))
    sh = np.zeros((o.size, 8), F)
    sh[:, 5], sh[:, 6] = fw[o], el[o]
    return ys[o].astype(np.int32), xs[o].astype(np.int32), sh, fl[o], f[o].astype(F), e[o].astype(F)


def gpu_stats(ctx, lst, size, nsy, nsx, snr=20.0):
    t = G.shape_stats(ctx, *[dev(ctx, a) for a in lst], size, nsy, nsx, snr)
    ctx.sync()
    return t.cpu().numpy()


def compare_tables(got, want):
    exact = [0, 1, 2, 3, 5, 6]                                       # counts, stride, medians
    assert np.array_equal(got[:, exact], want[:, exact], equal_nan=True), (got[:, exact], want[:, exact])
    assert np.array_equal(np.isnan(got[:, [4, 7]]), np.isnan(want[:, [4, 7]]))
    ok = ~np.isnan(want[:, [4, 7]])
    rel = np.abs(got[:, [4, 7]][ok] / want[:, [4, 7]][ok] - 1)
    print('shape statistics: largest relative difference of the stds %.3g' % rel.max())
    assert rel.max() <= 1e-12


def test_stats_meet_the_restatement(ctx):
    rs = np.random.RandomState(6)
    nmin = 15
    counts = [0, nmin - 1, nmin, 300, 200, 1000, 50, 64]             # 8 tiles, one of them without a qualifying source
    lst = shape_lists(rs, counts, 100, 4)
    want = S.shape_stats_ref(*lst, 100, 2, 4, 20.0)
    assert want[:8, 0].astype(int).tolist() == counts and want[8, 0] == sum(counts)          # only those meant to qualify do
    assert (want[3:6, 2] < want[3:6, 0]).all()                       # the outliers are clipped
    assert np.array_equal(want[0], G.empty_shape_table(8)[0], equal_nan=True)
    got = gpu_stats(ctx, lst, 100, 2, 4)
    compare_tables(got, want)
    assert np.array_equal(gpu_stats(ctx, lst, 100, 2, 4), got, equal_nan=True)               # the same bits
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 8), F), np.zeros(0, np.uint8), np.zeros(0, F), np.zeros(0, F))
    assert np.array_equal(gpu_stats(ctx, e, 100, 2, 4), G.empty_shape_table(8), equal_nan=True)
    none = (lst[0], lst[1], lst[2], np.ones_like(lst[3]), lst[4], lst[5])                    # every source flagged
    assert np.array_equal(gpu_stats(ctx, none, 100, 2, 4), G.empty_shape_table(8), equal_nan=True)


def test_stats_stride_path(ctx):
    """20000 qualifying sources in one tile: every third enters the statistics, and the stride slot says so"""
    rs = np.random.RandomState(9)
    lst = shape_lists(rs, [20000], 1000, 1, bad=3)
    want = S.shape_stats_ref(*lst, 1000, 1, 1, 20.0)
    assert want[0, 0] == 20000 and want[0, 1] == 3 and want[1, 1] == 3 and want[0, 2] <= 6667
    compare_tables(gpu_stats(ctx, lst, 1000, 1, 1), want)


# ---- optimal_subtraction -------------------------------------------------------------------------------------------
CATBASE = ['Y_POS', 'X_POS', 'E_FLUX_PEAK', 'E_FLUX_OPT', 'E_FLUXERR_OPT', 'SNR_OPT']      # (+ NUMBER, which format_cat adds: the seven columns)
SHAPE9 = ['FWHM', 'ELONGATION', 'A', 'B', 'THETA', 'X2', 'Y2', 'XY', 'FLAGS_MASK']
SKEYS = ['S-NOBJ', 'S-FWHM', 'S-FWSTD', 'S-SEEING', 'S-SEESTD', 'S-ELONG', 'S-ELOSTD']


@pytest.fixture(scope='module')
def e2e(ctx, scene):
    k = int(np.argmax(scene['f_new'] * (scene['tile'] == 5)))         # a bright star of tile 5, masked
    masked = (int(round(scene['ny'][k])), int(round(scene['nx'][k])))
    new, new_mask, ref, kw = M.subtraction_inputs(ctx, scene, masked)
    kw = dict(kw, cat_extract=True, fratio=1.0)
    runs = dict(on=M.run_sub(ctx, new, new_mask, ref, kw, shapes=True), off=M.run_sub(ctx, new, new_mask, ref, kw, shapes=False),
                both=M.run_sub(ctx, new, new_mask, ref, kw, shapes=True, match=True), match=M.run_sub(ctx, new, new_mask, ref, kw, match=True))
    return dict(runs, masked=masked, new_mask=new_mask.cpu().numpy())


def test_subtraction_with_shapes(ctx, scene, e2e):
    on = e2e['on']
    cat, hn = on['catalog'], on['header_new']
    assert list(cat) == CATBASE + SHAPE9 and [k for k in hn if k.startswith('S-') and k not in ('S-BKG', 'S-BKGSTD')] == SKEYS
    assert sorted(on['shapes']) == ['n_good', 'table'] and on['shapes']['table'].shape == (NSUB + 1, 8)
    # the restatement chain on the frame the subtraction saw
    work = on['data_bkgsub'].cpu().numpy()
    ys, xs = H.host_peaks(work, 5.0 * hn['S-BKGSTD'][0])
    free = e2e['new_mask'][ys, xs] == 0
    assert (~free).sum() == 1 and (ys[~free][0], xs[~free][0]) == e2e['masked']
    ys, xs = ys[free], xs[free]
    n = len(ys)
    assert hn['S-NOBJ'][0] == n == len(cat['X_POS']) == hn['NOBJECTS'][0]
    sub_pn = G.subimage_psfs(ctx, dev(ctx, scene['psf_new']), H.NSY, H.NSX, H.SIZE)
    sigw = G.window_sigma(sub_pn).cpu().numpy()
    off = H.win_centroid_ref(work, ys, xs, sigw, H.SIZE, H.NSY, H.NSX, H.RAD, H.NITER).astype(F)
    args = (work, ys, xs, off, sigw, H.SIZE, H.NSY, H.NSX, H.RAD, H.NITER)
    want, w32 = S.shapes_ref(*args, np.float64), S.shapes_ref(*args, np.float32)
    assert np.array_equal(np.isnan(w32), np.isnan(want))
    tol = max(16 * np.nanmax(np.abs(w32[:, 2:4].astype(np.float64) / want[:, 2:4] - 1)), 2e-5)
    rows = np.stack([np.zeros(n, F), np.zeros(n, F), cat['Y2'], cat['X2'], cat['XY'], cat['FWHM'], cat['ELONGATION'], cat['THETA']], axis=1)
    nan = np.isnan(want[:, 0])
    rows[:, 0], rows[:, 1] = np.where(nan, np.nan, 0), np.where(nan, np.nan, 0)
    w0 = want.copy()
    w0[~nan, 0:2] = 0.0                                              # (the centres are compared through X_POS / Y_POS below)
    compare_shapes(rows, w0, tol, 'catalogue')
    # positions: peak + 1 + offset, the integer peak where there is no shape; float32 near 480 has an ulp of 3.1e-5
    for col, p, k in (('Y_POS', ys, 0), ('X_POS', xs, 1)):
        assert np.abs(cat[col] - (p + 1 + np.where(nan, 0, want[:, k]))).max() <= 2e-5 + 3.1e-5, col
        assert np.array_equal(cat[col][nan], (p[nan] + 1).astype(F))
    assert (np.abs(cat['X_POS'] - np.rint(cat['X_POS'])) > 1e-3).sum() > 100
    ok = ~nan
    T = np.maximum(want[ok, 2], want[ok, 3])
    tr, rad = want[ok, 2] + want[ok, 3], np.sqrt((want[ok, 3] - want[ok, 2]) ** 2 + 4 * want[ok, 4] ** 2)
    for col, w in (('A', np.sqrt((tr + rad) / 2)), ('B', np.sqrt((tr - rad) / 2))):
        assert (np.abs(cat[col][ok] / w - 1) <= 1.25 * tol * T / w ** 2).all(), col          # A^2, B^2 move by <= 2.42 tol T
    # flags: the masked star's neighbours see its mask
    assert np.array_equal(cat['FLAGS_MASK'], S.flags_ref(e2e['new_mask'], ys, xs, H.RAD)) and cat['FLAGS_MASK'].dtype == np.uint8
    # the table: the statistics of the catalogue's own columns, exactly; the header from its frame row
    f, e = cat['E_FLUX_OPT'], cat['E_FLUXERR_OPT']
    tab = on['shapes']['table']
    twant = S.shape_stats_ref(ys, xs, rows, cat['FLAGS_MASK'], f, e, H.SIZE, H.NSY, H.NSX, 20.0)
    compare_tables(tab, twant)
    assert on['shapes']['n_good'] == tab[NSUB, 2] >= 15
    assert (hn['S-FWHM'][0], hn['S-FWSTD'][0], hn['S-ELONG'][0], hn['S-ELOSTD'][0]) == tuple(tab[NSUB, [3, 4, 6, 7]])
    assert hn['S-SEEING'][0] == hn['S-FWHM'][0] * 0.564 and hn['S-SEESTD'][0] == hn['S-FWSTD'][0] * 0.564
    # ... and they are the restatement chain's within the tolerance (medians of values that each agree within it)
    t64 = S.shape_stats_ref(ys, xs, want, cat['FLAGS_MASK'], f, e, H.SIZE, H.NSY, H.NSX, 20.0)
    print('header:', {k: hn[k][0] for k in SKEYS}, '; restatement chain: FWHM %.6f elongation %.6f' % (t64[NSUB, 3], t64[NSUB, 6]))
    assert t64[NSUB, 0] == tab[NSUB, 0]
    assert abs(hn['S-FWHM'][0] / t64[NSUB, 3] - 1) <= tol and abs(hn['S-ELONG'][0] / t64[NSUB, 6] - 1) <= 1.25 * tol * (1 + t64[NSUB, 6] ** 2)
    assert H.FWHM_NEW < hn['S-FWHM'][0] < 1.5 * H.FWHM_NEW           # (test_shapes_host: the Gaussian-equivalent width of the Moffat)


def test_shapes_leave_the_match_and_the_rest_alone(ctx, e2e):
    on, off, both, match = e2e['on'], e2e['off'], e2e['both'], e2e['match']
    # with the star match as well: its results bit for bit, the shapes bit for bit
    assert np.array_equal(both['match']['table'], match['match']['table'], equal_nan=True)
    assert {k: v for k, v in both['match'].items() if k != 'table'}.keys() == match['match'].keys() - {'table'}
    for k in ('n_new', 'n_ref', 'n_pairs', 'success'):
        assert both['match'][k] == match['match'][k]
    assert np.array_equal(both['scal'], match['scal']) and torch.equal(both['D'], match['D']) and torch.equal(both['Scorr'], match['Scorr'])
    assert both['header_trans'] == match['header_trans']
    for k in CATBASE + SHAPE9:
        assert np.array_equal(both['catalog'][k], on['catalog'][k], equal_nan=True), k
    assert np.array_equal(both['shapes']['table'], on['shapes']['table'], equal_nan=True)
    # switched off: no key, the seven columns, no S-SEEING; the products are those of the run with the switch on
    assert 'shapes' not in off and 'shapes' not in match
    assert list(off['catalog']) == CATBASE and list(match['catalog']) == CATBASE
    assert not any(k in off['header_new'] for k in SKEYS) and not any(k in off['header_trans'] for k in SKEYS)
    assert np.array_equal(off['catalog']['X_POS'], np.rint(off['catalog']['X_POS']))
    for k in CATBASE[2:]:
        assert np.array_equal(off['catalog'][k], on['catalog'][k]), k
    assert torch.equal(off['D'], on['D']) and torch.equal(off['Scorr'], on['Scorr'])
    assert {k: v for k, v in on['header_new'].items() if k not in SKEYS} == off['header_new']


def test_too_few_stars_give_none(ctx):
    sc = H.make_scene(seed=9, nstars=5)
    new, new_mask, ref, kw = M.subtraction_inputs(ctx, sc)
    res = M.run_sub(ctx, new, new_mask, ref, dict(kw, cat_extract=True, fratio=1.0), shapes=True)
    hn = res['header_new']
    assert res['shapes']['n_good'] < 15 and hn['S-NOBJ'][0] == len(res['catalog']['X_POS'])
    assert [hn[k][0] for k in SKEYS[1:]] == ['None'] * 6


# ---- command line --------------------------------------------------------------------------------------------------
def test_cli_writes_columns_and_keys(tmp_path, ctx):
    """blackbox.py --cat_extract True --cat_shapes True on a small frame (the 2 x 8 channels of 120 x 330 pixels of the
    operator tests: the subtraction stage needs a whole number of background boxes per channel): `_cat.fits` with the new columns,
    S-SEEING in `_cat_hdr.fits`; without the switch neither; two frames through the frames-in-flight list run give the serial
    path's catalogue"""
    import logging
    import bbx_oracle as O
    import test_gpu_operator as OP
    from blackbox_amd import catalogs, fitsio, synth
    cli = OP.load_cli()
    case = synth.make_case(OP.YS, OP.XS, 77, tel=OP.TEL, os_y=20, os_x=45, n_stars=60, n_sat=2, n_cr=40)
    raws = []
    for k in range(2):
        raws.append(str(tmp_path / ('ML1_raw%d.fits' % k)))
        fitsio.write_image(raws[-1], case['raw'], {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q', 'DATE-OBS': '2024-01-02T03:04:0%d' % k})
    fitsio.write_image(str(tmp_path / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp_path / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp_path / 'xtalk.dat'), case['xtalk'])
    d0 = R.reduce_object(ctx, dev(ctx, case['raw']), {}, OP.TEL, mflat=dev(ctx, case['flat']), bpm=dev(ctx, case['bpm']),
                         xtalk_coeffs=O.xtalk_coeffs(case['xtalk']), exptime=60.0, ysize_chan=OP.YS, xsize_chan=OP.XS,
                         log=logging.getLogger('t'))[0]
    rs = np.random.RandomState(3)
    fitsio.write_image(str(tmp_path / 'ref.fits'), (d0.cpu().numpy() - 100.0 + rs.normal(0, 4, d0.shape)).astype(F))
    fitsio.write_image(str(tmp_path / 'psf.fits'), OP.moffat(15, 3.5))
    common = ['--telescope', OP.TEL, '--mflat', str(tmp_path / 'flat.fits'), '--bpm', str(tmp_path / 'bpm.fits'),
              '--crosstalk', str(tmp_path / 'xtalk.dat'), '--ysize_chan', str(OP.YS), '--xsize_chan', str(OP.XS),
              '--cat_extract', 'True', '--trans_extract', 'True', '--ref', str(tmp_path / 'ref.fits'), '--psf_new', str(tmp_path / 'psf.fits'),
              '--psf_ref', str(tmp_path / 'psf.fits'), '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30']
    base_cols = [c[0] for c in catalogs.COLUMNS['new']]
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'on'), '--cat_shapes', 'True'])
    cat, _ = fitsio.read_table(str(tmp_path / 'on' / 'ML1_20240102_030400_red_cat.fits'))
    assert list(cat) == base_cols + SHAPE9 and len(cat['X_POS']) > 10
    assert np.isfinite(cat['FWHM']).sum() > 10 and (np.abs(cat['X_POS'] - np.rint(cat['X_POS'])) > 1e-3).any()
    h = fitsio.read_hdus(str(tmp_path / 'on' / 'ML1_20240102_030400_red_cat_hdr.fits'))[0][0]
    for k in SKEYS:
        assert k in h, k
    print('command line, switch on:', {k: R.hval(h, k) for k in SKEYS + ['QC-FLAG']})
    assert R.hval(h, 'S-NOBJ') == len(cat['X_POS'])
    if not isinstance(R.hval(h, 'S-SEEING'), str):
        assert R.hval(h, 'S-SEEING') == pytest.approx(R.hval(h, 'S-FWHM') * 0.564, rel=1e-9)
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'off')])
    cat_off, _ = fitsio.read_table(str(tmp_path / 'off' / 'ML1_20240102_030400_red_cat.fits'))
    h = fitsio.read_hdus(str(tmp_path / 'off' / 'ML1_20240102_030400_red_cat_hdr.fits'))[0][0]
    assert list(cat_off) == base_cols and not any(k in h for k in SKEYS)
    assert np.array_equal(cat_off['E_FLUX_OPT'], cat['E_FLUX_OPT'])
    # the list run (FramePipeline) of two frames: the serial path's catalogue and keys
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(raws) + '\n')
    outs = cli.main(common + ['--image_list', lst, '--red_dir', str(tmp_path / 'lst'), '--cat_shapes', 'True'])
    assert len(outs) == 2 and all(outs)
    h_on = fitsio.read_hdus(str(tmp_path / 'on' / 'ML1_20240102_030400_red_cat_hdr.fits'))[0][0]
    for k in range(2):
        got, _ = fitsio.read_table(str(tmp_path / 'lst' / ('ML1_20240102_03040%d_red_cat.fits' % k)))
        assert list(got) == list(cat)
        for name in cat:
            assert np.array_equal(got[name], cat[name], equal_nan=True), (k, name)
        hk = fitsio.read_hdus(str(tmp_path / 'lst' / ('ML1_20240102_03040%d_red_cat_hdr.fits' % k)))[0][0]
        assert [R.hval(hk, s) for s in SKEYS] == [R.hval(h_on, s) for s in SKEYS], k
