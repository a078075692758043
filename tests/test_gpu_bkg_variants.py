"""GPU: every fill, zoom and prefilter variant of the background mesh (bbx_bkg.hip) at small shapes.

bbx_spline_zoom / bbx_spline_zoom_sub choose between two kernels by row width and pointer alignment, and each kernel
between two or three code paths by the number of coefficient columns a workgroup touches; bbx_mini_fill_filter chooses by
the size of the mini image.  tests/test_bkg_shapes.py restates those choices and lists the geometries (held to their
regimes on the CPU); every launch here asserts the regime of its actual pointers first.

Bars: the background against the oracle's mini2back (scipy's zoom: float64, rounded to float32) rtol 2.4e-7, the bar of
test_background_mesh; the subtracted frame against `data - bkg_gpu` exactly (one float32 operation on the kernel's own
value); the kernels against each other bit for bit where they do the same operations in the same order; fill + filter
and the prefilter bit for bit (order statistics and one float64 mean; scipy's operations one by one)."""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import zogy_core as Z                                   # noqa: E402
import test_bkg_shapes as S                             # noqa: E402
from blackbox_amd import reduce as R                    # noqa: E402
from blackbox_amd import zogy as G                      # noqa: E402
from blackbox_amd._lib import lib, check, BBXError      # noqa: E402

F = np.float32
RTOL_BKG = 2.4e-7                  # two float32 ulps of a float64 16-tap sum (test_background_mesh)
GUARD = -777.0                     # what the floats around a frame tensor hold before and after a launch
KINDS = ('sky', 'sigma')


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


# ---- zoom -------------------------------------------------------------------------------------------------------------
def _seed(g, kind):
    return zlib.crc32(repr((g.nby, g.nbx, g.box, g.channels, kind)).encode()) & 0x7fffffff


@functools.lru_cache(maxsize=None)
def _mini(key, kind):
    """values well away from zero: a 300 +- 20 sky with a gradient, a sigma map between 8 and 30.  Keyed by what twins
    share (mini shape, box, channels), so that both launches of a twin pair zoom the same image."""
    nby, nbx, box, channels = key
    rs = np.random.RandomState(zlib.crc32(repr((key, kind)).encode()) & 0x7fffffff)
    yy, xx = np.mgrid[0:nby, 0:nbx]
    if kind == 'sky':
        m = 300 + 10 * (xx / nbx - 0.5) + 6 * (yy / nby - 0.5) + np.clip(rs.normal(0, 4, (nby, nbx)), -12, 12)
    else:
        m = 19 + 6 * np.sin(xx / 3.0 + yy / 5.0) + rs.uniform(-4, 4, (nby, nbx))
    m = m.astype(F)
    m.setflags(write=False)
    return m


def mini_of(g, kind):
    return _mini((g.nby, g.nbx, g.box, g.channels), kind)


@functools.lru_cache(maxsize=None)
def _oracle(key, kind):
    nby, nbx, box, channels = key
    out = Z.mini2back(_mini(key, kind), (nby * box, nbx * box), box, channels)
    assert out.dtype == F
    out.setflags(write=False)
    return out


def oracle_of(g, kind):
    return _oracle((g.nby, g.nbx, g.box, g.channels), kind)


def frame_of(g, kind):
    rs = np.random.RandomState(_seed(g, kind) ^ 0x5a5a)
    return (oracle_of(g, kind) + rs.normal(0, 15, g.shape)).astype(F)


class Frame:
    """a [ny, nx] float32 device tensor g.off floats behind a 16-byte boundary, with guard floats on both sides"""

    def __init__(self, ctx, g, values=None):
        ny, nx = g.shape
        self.buf = torch.full((ny * nx + 8,), GUARD, dtype=torch.float32, device=ctx.device)
        self.t = self.buf[g.off:g.off + ny * nx].view(ny, nx)
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * g.off
        if values is None:
            self.t.fill_(float('nan'))                              # a pixel the kernel leaves out stays NaN
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values)))
        self.off, self.n = g.off, ny * nx

    def get(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:self.off] == F(GUARD)) and np.all(b[self.off + self.n:] == F(GUARD)), 'a write outside the frame'
        return b[self.off:self.off + self.n].reshape(self.t.shape).copy()


def coefficients(ctx, g, kind):
    return G.device_zoom_coefficients(ctx, dev(ctx, mini_of(g, kind)), g.channels)


def _zoom_args(ctx, g, coef):
    ny, nx = g.shape
    fy, wy, fx, wx = G._device_taps(ctx, g.nby, g.nbx, g.box, *g.blocks)
    return (ctx.h, ny, nx, G._p(coef), coef.shape[0], coef.shape[1], G._p(fy), G._p(wy), G._p(fx), G._p(wx))


def _assert_launch(g, *frames):
    """the launch condition of bbx_spline_zoom(_sub) on the pointers that are passed, and the regime of every workgroup"""
    ptrs = [f.t.data_ptr() if f is not None else 0 for f in frames]
    assert g.launch(*ptrs) == (g.kernel, g.regimes), (g.name, ptrs)


def zoom(ctx, g, coef, data=None, bkg=None):
    _assert_launch(g, data, bkg)
    check(lib.bbx_spline_zoom(*_zoom_args(ctx, g, coef), G._p(data.t if data else None), G._p(bkg.t if bkg else None), ctx.stream()),
          'bbx_spline_zoom', ctx.h)
    ctx.sync()


def zoom_sub(ctx, g, coef, src, out):
    _assert_launch(g, src, out)
    check(lib.bbx_spline_zoom_sub(*_zoom_args(ctx, g, coef), G._p(src.t), G._p(out.t), ctx.stream()), 'bbx_spline_zoom_sub', ctx.h)
    ctx.sync()


def four_call_shapes(ctx, g, kind):
    """-> bkg alone, (data, bkg) of the in-place call with bkg, data of the in-place call without, out of zoom_sub"""
    coef = coefficients(ctx, g, kind)
    data = frame_of(g, kind)
    b0 = Frame(ctx, g)
    zoom(ctx, g, coef, bkg=b0)
    d1, b1 = Frame(ctx, g, data), Frame(ctx, g)
    zoom(ctx, g, coef, data=d1, bkg=b1)
    d2 = Frame(ctx, g, data)
    zoom(ctx, g, coef, data=d2)
    src, out = Frame(ctx, g, data), Frame(ctx, g)
    zoom_sub(ctx, g, coef, src, out)
    assert np.array_equal(src.get().view(np.uint32), data.view(np.uint32)), 'zoom_sub changed its source'
    return data, b0.get(), d1.get(), b1.get(), d2.get(), out.get()


def block_columns(g):
    width = 256 if g.kernel == 'scalar' else 1024
    return [(r, slice(x0, min(x0 + width, g.shape[1]))) for r, x0 in zip(g.regimes, range(0, g.shape[1], width))]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('g', S.GEOMETRIES, ids=lambda g: g.name)
def test_zoom_regime_against_scipy(ctx, g, kind):
    """bkg only; data -= bkg in place with and without bkg written; zoom_sub from an untouched source: the same background
    bits from all of them, within 2.4e-7 of scipy's zoom, and the subtraction exact"""
    want = oracle_of(g, kind)
    data, b0, d1, b1, d2, out = four_call_shapes(ctx, g, kind)
    assert not np.isnan(b0).any() and np.abs(want).min() > 5
    for r, cols in block_columns(g):
        rel = np.abs(b0[:, cols].astype(np.float64) - want[:, cols]) / np.abs(want[:, cols])
        print('BKGVAR %s %s %s %s maxrel %.3e' % (g.kernel, r, g.name, kind, rel.max()))
    np.testing.assert_allclose(b0, want, rtol=RTOL_BKG, atol=0)
    assert np.array_equal(b1, b0)
    sub = data - b0                                                  # float32 - float32
    assert np.array_equal(d1, sub) and np.array_equal(d2, sub) and np.array_equal(out, sub)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('v, s', S.TWINS)
def test_zoom_scalar_and_vector_kernels_give_the_same_bits(ctx, v, s, kind):
    """the folded regimes (scalar span <= 32, scalar span <= 512, vector span <= 64) fold the four coefficient rows with the
    same association and add the four column taps in the same order; the two 16-tap branches add the same 16 products in
    the same order.  The same mini image through a vector launch and through a scalar one (pointers one float off)"""
    gv, gs = S.BY_NAME[v], S.BY_NAME[s]
    assert gv.family() == gs.family() and mini_of(gv, kind) is mini_of(gs, kind)
    rv, rs_ = four_call_shapes(ctx, gv, kind), four_call_shapes(ctx, gs, kind)
    assert np.array_equal(rv[0], rs_[0])                             # the same frame to subtract from
    for a, b in zip(rv[1:], rs_[1:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def star_frame(g, seed):
    """noise about a sky of 100 with ~40 3 x 3 stars and one dense block that lies inside one workgroup of the vector kernel
    (32 rows x 1024 pixels) and holds more pixels than its queue of 2048"""
    ny, nx = g.shape
    rs = np.random.RandomState(seed)
    img = rs.normal(100, 5, (ny, nx)).astype(F)
    for _ in range(40):
        y, x = rs.randint(34, ny - 3), rs.randint(3, nx - 3)
        img[y - 1:y + 2, x - 1:x + 2] += F(rs.uniform(60, 3000))
    img[1:32, 600:680] += F(500.0)                                   # 31 x 80 = 2480 pixels; crosses x = 640
    return img


@pytest.mark.parametrize('name', ['vector_taps16_frame', 'vector_fold64_border'])
def test_candidates_listed_by_the_zoom(ctx, name):
    """bbx_zoom_candidates on the 16-tap branch of k_spline_zoom4 (a reservation per pixel) and on the folded branch where
    the span crosses a channel border: the peaks found from the list equal those of bbx_find_peaks' own pass, the frame
    equals src - bkg, and another threshold than the list's is refused"""
    g = S.BY_NAME[name]
    ny, nx = g.shape
    rs = np.random.RandomState(5 + ny)
    yy, xx = np.mgrid[0:g.nby, 0:g.nbx]
    mini = (100 + 3 * xx / g.nbx - 2 * yy / g.nby + rs.normal(0, 0.3, (g.nby, g.nbx))).astype(F)
    mstd = rs.uniform(5, 7, (g.nby, g.nbx)).astype(F)
    img = star_frame(g, 11 + nx)
    coef = G.device_zoom_coefficients(ctx, dev(ctx, mini), g.channels)
    d_mstd = dev(ctx, mstd)
    d_med = torch.empty(1, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_mini_median(ctx.h, mstd.size, G._p(d_mstd), G._p(d_med), ctx.stream()), 'bbx_mini_median', ctx.h)
    ctx.sync()
    assert d_med.item() == np.median(mstd)
    nsig = 5.0
    thr = float(nsig) * float(np.median(mstd))
    bkg = Frame(ctx, g)
    zoom(ctx, g, coef, bkg=bkg)
    want = img - bkg.get()
    assert (np.abs(want[1:32, 600:680]) >= F(thr)).all() and (np.abs(want) >= F(thr)).sum() >= 2480 + 200

    src, work = Frame(ctx, g, img), Frame(ctx, g)
    check(lib.bbx_zoom_candidates(ctx.h, G._p(d_med), nsig), 'bbx_zoom_candidates', ctx.h)
    zoom_sub(ctx, g, coef, src, work)
    assert np.array_equal(work.get(), want)
    a = G.find_peaks_arrays(ctx, work.t, thr, max_out=20000)         # from the list
    b = G.find_peaks_arrays(ctx, work.t.clone(), thr, max_out=20000)  # own pass
    c = G.find_peaks_arrays(ctx, work.t, thr, max_out=20000)         # the list is spent: own pass
    assert 30 <= a[0].size <= 41
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # the peaks are those of the frame: every one at or above the threshold, the block's among them
    assert (np.abs(a[2]) >= F(thr)).all() and np.array_equal(a[2], want[a[0], a[1]])
    assert ((a[0] < 32) & (a[1] >= 600) & (a[1] < 680)).sum() == 1
    # another threshold on a listed frame: refused, and the flag is gone with the refusal
    check(lib.bbx_zoom_candidates(ctx.h, G._p(d_med), nsig), 'bbx_zoom_candidates', ctx.h)
    zoom_sub(ctx, g, coef, src, work)
    with pytest.raises(BBXError):
        G.find_peaks_arrays(ctx, work.t, thr * 1.5, max_out=20000)
    ctx.sync()


# ---- fill and filter ----------------------------------------------------------------------------------------------------
HOLES = ('none', 'isolated', 'block', 'corner', 'row_col', 'pair', 'inf')
PAIRS = ((16777216.0, 3.0), (3.0e38, 3.2e38))      # (sum exact in float64 only; float32 sum overflows, float64 mean does not)


def fill_input(shape, holes):
    """float32 values of both signs, quarter-unit rounding on the left half (ties), one value planted many times; then the
    hole pattern.  None: the shape cannot hold it."""
    nby, nbx = shape
    rs = np.random.RandomState(zlib.crc32(repr((shape, holes)).encode()) & 0x7fffffff)
    a = rs.normal(0, 50, shape)
    a[:, :nbx // 2] = np.round(a[:, :nbx // 2] * 4) / 4
    a[rs.random_sample(shape) < 0.05] = 12.25
    a = a.astype(F)
    nan = F(np.nan)
    if holes == 'none':                                              # the median filter alone
        pass
    elif holes == 'isolated':
        if nby * nbx < 2:
            return None
        a[rs.random_sample(shape) < 0.03] = nan
        a[rs.randint(nby), rs.randint(nbx)] = nan
        if np.isnan(a).all():
            a[0, 0] = F(1.5)
    elif holes == 'block':                                           # 7 x 9: four sweeps deep
        if nby < 20 or nbx < 24:
            return None
        a[10:17, 12:21] = nan
    elif holes == 'corner':                                          # the same block in two corners: seven sweeps from inside
        if nby < 20 or nbx < 24:
            return None
        a[:7, :9] = nan
        a[-7:, -9:] = nan
    elif holes == 'row_col':
        if nby < 2 or nbx < 2:
            return None
        a[0, :] = nan
        a[:, -1] = nan
    elif holes == 'pair':                                            # a corner whose only valid neighbours are two values
        if nby < 5 or nbx < 7:
            return None
        a[0, 0], a[1, 1], a[0, 1], a[1, 0] = nan, nan, F(PAIRS[0][0]), F(PAIRS[0][1])
        a[-1, -1], a[-2, -2], a[-1, -2], a[-2, -1] = nan, nan, F(PAIRS[1][0]), F(PAIRS[1][1])
    elif holes == 'inf':
        if nby < 5 or nbx < 7:
            return None
        a[rs.random_sample(shape) < 0.04] = nan
        a[2, 2:5] = nan
        a[1, 3], a[3, 2] = F(np.inf), F(np.inf)
        a[rs.random_sample(shape) < 0.02] = F(np.inf)
    return a


_fill_cache = {}


def fill_case(shape, holes):
    """(input, oracle), computed once and shared by both orders"""
    key = (shape, holes)
    if key not in _fill_cache:
        a = fill_input(shape, holes)
        _fill_cache[key] = None if a is None else (a, Z.fill_filter_mini(a))
    return _fill_cache[key]


def gpu_fill(ctx, a):
    nby, nbx = a.shape
    n = a.size
    buf = torch.full((n + 16,), GUARD, dtype=torch.float32, device=ctx.device)
    t = buf[8:8 + n].view(nby, nbx)
    t.copy_(torch.from_numpy(a))
    check(lib.bbx_mini_fill_filter(ctx.h, nby, nbx, G._p(t), ctx.stream()), 'bbx_mini_fill_filter', ctx.h)
    ctx.sync()                                                       # (a device error flag fails here)
    b = buf.cpu().numpy()
    assert np.all(b[:8] == F(GUARD)) and np.all(b[8 + n:] == F(GUARD)), 'a write outside the mini image'
    return b[8:8 + n].reshape(nby, nbx).copy()


def test_fill_pairs_are_what_they_are_meant_to_be():
    """the planted pairs: the float64 mean of the first needs more than float32's 24 bits before it is rounded; the float32 sum
    of the second overflows.  (For two float32 values the float64 sum is exact or the smaller one is below half an ulp
    of the larger in both formats, so only the overflow makes a float32 mean differ from the rounded float64 mean.)"""
    a, b = F(PAIRS[0][0]), F(PAIRS[0][1])
    assert (np.float64(a) + np.float64(b)) * 0.5 == 8388609.5 and F((np.float64(a) + np.float64(b)) * 0.5) == F(8388610.0)
    a, b = F(PAIRS[1][0]), F(PAIRS[1][1])
    with np.errstate(over='ignore'):
        assert np.isinf((a + b) * F(0.5)) and np.isfinite(F((np.float64(a) + np.float64(b)) * 0.5))
    x = fill_input((31, 33), 'pair')
    want = Z.fill_filter_mini(x)
    assert np.isfinite(want).all()


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_fill_filter_shapes_and_holes(ctx, order):
    """both kernels of bbx_mini_fill_filter (the LDS one up to 36864 entries, with one and with up to 36 entries per thread;
    the two-buffer one above) on every hole pattern the shape can hold, bit for bit against the oracle.  Forward and
    reversed: the LDS attribute is set once per process, the global kernel alternates between two buffers."""
    shapes = S.FILL_SHAPES if order == 'forward' else S.FILL_SHAPES[::-1]
    ran = {k: 0 for k in ('k_mini_fill_filter_lds', 'k_mini_fill_filter')}
    per_pattern = {h: 0 for h in HOLES}
    for shape in shapes:
        kernel = S.fill_kernel(*shape)
        assert (kernel == 'k_mini_fill_filter_lds') == (shape[0] * shape[1] <= 36864)
        for holes in HOLES:
            case = fill_case(shape, holes)
            if case is None:
                continue
            a, want = case
            got = gpu_fill(ctx, a)
            assert np.array_equal(got, want, equal_nan=True), (shape, holes, kernel, int((got != want).sum()))
            assert not np.isnan(got).any()
            ran[kernel] += 1
            per_pattern[holes] += 1
    assert ran['k_mini_fill_filter'] >= 2 * len(HOLES) and ran['k_mini_fill_filter_lds'] >= 30
    assert min(per_pattern.values()) >= 8


@pytest.mark.parametrize('shape', [(9, 13), (192, 193)])
def test_fill_filter_all_nan_and_one_finite_entry(ctx, shape):
    """an image without a finite entry stays NaN and raises no device error; one finite entry fills the whole image"""
    a = np.full(shape, np.nan, F)
    got = gpu_fill(ctx, a)
    assert np.isnan(got).all()
    if a.size < 1000:
        assert np.isnan(Z.fill_filter_mini(a)).all()
    a[2, 5] = F(-37.125)
    got = gpu_fill(ctx, a)
    assert np.array_equal(got, np.full(shape, F(-37.125)))
    if a.size < 1000:
        assert np.array_equal(Z.fill_filter_mini(a), got)            # (the oracle's Python sweeps: the small shape only)


# ---- prefilter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape, channels', [((2, 8), (1, 1)), ((3, 40), (3, 1))])
def test_prefilter_blocks_of_a_single_box(ctx, shape, channels):
    """channel blocks one box high and / or wide: a padded line is 25 copies of one value"""
    assert not S.prefilter_refused(*shape, channels)
    rs = np.random.RandomState(shape[1])
    mini = (rs.normal(300.0, 20.0, shape) + 50 * np.sin(np.arange(shape[1]) / 7.0)).astype(F)
    ref = G.zoom_coefficients(mini, channels)
    got = G.device_zoom_coefficients(ctx, dev(ctx, mini), channels)
    ctx.sync()
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), np.abs(got - ref).max()


def test_prefilter_refuses_a_line_longer_than_512(ctx):
    """py = 500 + 24 > SPF_MAXLEN: BBX_ERR_ARG, and nothing is written"""
    import math
    nby, nbx = 500, 3
    assert S.prefilter_refused(nby, nbx)
    py, px = nby + 2 * G.NPAD, nbx + 2 * G.NPAD
    mini = dev(ctx, np.full((nby, nbx), 300, F))
    coef = torch.full((py, px), GUARD, dtype=torch.float64, device=ctx.device)
    rc = lib.bbx_spline_prefilter(ctx.h, nby, nbx, nby, nbx, G.NPAD, math.pow(G.SPLINE_POLE, py), math.pow(G.SPLINE_POLE, px),
                                  G._p(mini), G._p(coef), ctx.stream())
    assert rc == S.BBX_ERR_ARG
    ctx.sync()
    assert bool((coef == GUARD).all())
    with pytest.raises(BBXError) as e:
        G.device_zoom_coefficients(ctx, mini)
    assert e.value.code == S.BBX_ERR_ARG
    # the transposed image: px is the long one
    rc = lib.bbx_spline_prefilter(ctx.h, nbx, nby, nbx, nby, G.NPAD, math.pow(G.SPLINE_POLE, px), math.pow(G.SPLINE_POLE, py),
                                  G._p(mini), G._p(coef), ctx.stream())
    assert rc == S.BBX_ERR_ARG
    ctx.sync()
    assert bool((coef == GUARD).all())


# ---- box statistics and the median of a mini image --------------------------------------------------------------------------
@pytest.mark.parametrize('full_sort', [0, 1])
@pytest.mark.parametrize('box, nby, nbx', [(8, 6, 7), (60, 3, 4)])
def test_box_statistics_kernels(ctx, box, nby, nbx, full_sort):
    """the three box kernels at small shapes: k_bkg_boxstats (BBX_OPT_BKG_FULL_SORT), k_bkg_boxstats_fast (boxes whose sample
    has 128 pixels and more) and k_bkg_boxstats_list (what the fast kernel leaves: every box of 8 x 8).  Medians bit for
    bit, std to the 2e-6 of test_background_mesh"""
    launched, stats_from = S.boxstats_kernels(box, full_sort)
    assert stats_from == ('k_bkg_boxstats' if full_sort else 'k_bkg_boxstats_list' if box == 8 else 'k_bkg_boxstats_fast')
    ny, nx = nby * box, nbx * box
    rs = np.random.RandomState(box + full_sort)
    data = rs.normal(300, 12, (ny, nx))
    data[rs.random_sample((ny, nx)) < 0.01] += 4000
    data[rs.random_sample((ny, nx)) < 0.005] -= 500
    data = data.astype(F)
    mask = (rs.random_sample((ny, nx)) < 0.04).astype(np.uint8)
    mask[box:2 * box, box:2 * box] = 4                               # a box below limfrac: NaN
    med_o, std_o = Z.get_back_mini(data, mask, None, box=box)
    m = torch.full((nby, nbx), -1.0, dtype=torch.float32, device=ctx.device)
    s = torch.full((nby, nbx), -1.0, dtype=torch.float32, device=ctx.device)
    t_data, t_mask = dev(ctx, data), dev(ctx, mask)
    try:
        check(lib.bbx_set_option(ctx.h, 8, full_sort), 'bbx_set_option', ctx.h)
        check(lib.bbx_bkg_boxstats(ctx.h, ny, nx, box, G._p(t_data), G._p(t_mask), G._p(None), 0.5, G._p(m), G._p(s), ctx.stream()),
              'bbx_bkg_boxstats', ctx.h)
        ctx.sync()
    finally:
        check(lib.bbx_set_option(ctx.h, 8, 0), 'bbx_set_option', ctx.h)
    mh, sh = m.cpu().numpy(), s.cpu().numpy()
    ok = ~np.isnan(med_o)
    assert np.array_equal(np.isnan(mh), ~ok) and np.array_equal(np.isnan(sh), ~ok) and (~ok).sum() == 1
    assert np.array_equal(mh[ok], med_o[ok])
    np.testing.assert_allclose(sh[ok], std_o[ok], rtol=2e-6, atol=0)


def test_box_statistics_wide_bracket(ctx):
    """the 16-register bracket sort of k_bkg_boxstats_fast (a bracket of 513 to 1024 keys): 24 boxes of 60 x 60 integer-valued
    pixels.  Medians bit for bit from the default path, from BBX_OPT_BKG_FULL_SORT and from the oracle; std to 2e-6"""
    box, nbx = 60, 24
    data = S.wide_bracket_frame(box, nbx)
    counts = [S.box_bracket_counts(data[:, box * b:box * b + box]) for b in range(nbx)]
    print('BOXVAR (nb, nt) per box:', counts)
    assert sum(512 < nb <= 1024 and nt <= 1024 for nb, nt in counts) >= 12
    ny, nx = data.shape
    mask = np.zeros((ny, nx), np.uint8)
    med_o, std_o = Z.get_back_mini(data, mask, None, box=box)
    assert med_o.shape == (1, nbx) and not np.isnan(med_o).any()
    t_data, t_mask = dev(ctx, data), dev(ctx, mask)
    got = {}
    try:
        for full_sort in (0, 1):
            m = torch.full((1, nbx), -1.0, dtype=torch.float32, device=ctx.device)
            s = torch.full((1, nbx), -1.0, dtype=torch.float32, device=ctx.device)
            check(lib.bbx_set_option(ctx.h, 8, full_sort), 'bbx_set_option', ctx.h)
            check(lib.bbx_bkg_boxstats(ctx.h, ny, nx, box, G._p(t_data), G._p(t_mask), G._p(None), 0.5, G._p(m), G._p(s), ctx.stream()),
                  'bbx_bkg_boxstats', ctx.h)
            ctx.sync()
            got[full_sort] = m.cpu().numpy(), s.cpu().numpy()
    finally:
        check(lib.bbx_set_option(ctx.h, 8, 0), 'bbx_set_option', ctx.h)
    for full_sort in (0, 1):
        mh, sh = got[full_sort]
        print('BOXVAR full_sort=%d std max rel diff %.3e' % (full_sort, np.max(np.abs(sh - std_o) / std_o)))
        assert np.array_equal(mh.view(np.uint32), med_o.view(np.uint32))
        np.testing.assert_allclose(sh, std_o, rtol=2e-6, atol=1e-7)
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))


@pytest.mark.parametrize('n', [1, 2, 1025, 32768, 32769, 40000])
def test_mini_median_kernels(ctx, n):
    """k_mini_median_regs up to 32768 values, k_mini_median above: np.median of float32 values, odd and even counts, ties
    across the middle"""
    assert S.median_kernel(n) == ('k_mini_median_regs' if n <= 32768 else 'k_mini_median')
    rs = np.random.RandomState(n)
    a = np.round(rs.normal(-3, 20, n) * 4).astype(F) / F(4)
    out = torch.full((1,), -1.0, dtype=torch.float32, device=ctx.device)
    d_a = dev(ctx, a)
    check(lib.bbx_mini_median(ctx.h, n, G._p(d_a), G._p(out), ctx.stream()), 'bbx_mini_median', ctx.h)
    ctx.sync()
    assert out.item() == np.median(a)
