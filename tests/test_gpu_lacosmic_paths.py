"""GPU: bbx_lacosmic on the scenes of tests/lacosmic_paths.py -- every queue, spill and seam path of the
sparse formulation at small shapes, against oracle/lacosmic.py detect_cosmics(..., return_iters=True).
Every comparison is exact and covers every pixel: the CR bit, every other mask bit, the cleaned float32 image
as bits, the per-iteration counts, the pixel count and the 8-connected object count.  That the scenes are on
their paths is asserted on the CPU by tests/test_lacosmic_paths_host.py.

Left to tests/test_gpu_fullsize.py (frames are not enlarged here to chase them): the direct-append branch of
k_lac_grow2 when its 1024-entry workgroup queue is full (needs a few hundred thousand stage-2 pixels); the
FEED_WQ spill of k_lac_cand_v4 is driven by the constant-sky case of test_gpu_parity.py
test_lacosmic_background_level.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import lacosmic_paths as P                 # noqa: E402
from blackbox_amd import _lib              # noqa: E402
from blackbox_amd import reduce as R       # noqa: E402

BBX_OPT_DEBUG_LISTCAP = 2
BBX_ERR_ARG, BBX_ERR_OVERFLOW = -1, -4
GUARD_F, GUARD_M = np.float32(-7.25e30), np.uint8(0xA5)


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


class Frame:
    """image and mask of a scene on the device, each inside a larger buffer with guard values around it.
    data_off: offset of the image in floats (4: 16-byte aligned, the vector kernel where nx % 4 == 0; 1: the
    scalar fallback); mask_off: offset of the mask in bytes."""

    def __init__(self, ctx, name, data_off=4, mask_off=4):
        self.name = name
        self.img, self.mask = P.make_scene(name), P.make_mask(name)
        ny, nx = self.img.shape
        n = ny * nx
        self.dbuf = torch.full((n + 8,), float(GUARD_F), dtype=torch.float32, device=ctx.device)
        self.mbuf = torch.full((n + 8,), int(GUARD_M), dtype=torch.uint8, device=ctx.device)
        assert self.dbuf.data_ptr() % 16 == 0 and self.mbuf.data_ptr() % 16 == 0
        self.d = self.dbuf[data_off:data_off + n].view(ny, nx)
        self.m = self.mbuf[mask_off:mask_off + n].view(ny, nx)
        self.d.copy_(torch.from_numpy(self.img))
        self.m.copy_(torch.from_numpy(self.mask))
        self.doff, self.moff, self.n = data_off, mask_off, n
        self.st = torch.full((16,), -1, dtype=torch.int32, device=ctx.device)

    def vector(self):
        """the launch condition of k_lac_cand_v4 in bbx_lacosmic"""
        return self.img.shape[1] % 4 == 0 and self.d.data_ptr() % 16 == 0

    def call(self, ctx, sigclip, sigfrac, niter, rn=P.RN, d_rdn16=None):
        ny, nx = self.img.shape
        return _lib.lib.bbx_lacosmic(ctx.h, ny, nx, C.c_void_p(self.d.data_ptr()), C.c_void_p(self.m.data_ptr()), float(sigclip),
                                     float(sigfrac), float(P.OBJLIM), int(niter), float(np.float32(rn)),
                                     C.c_void_p(d_rdn16.data_ptr() if d_rdn16 is not None else 0),
                                     C.c_void_p(self.st.data_ptr()), ctx.stream())

    def results(self):
        """-> (image, mask, stats) on the host, after checking the guard values"""
        dbuf, mbuf = self.dbuf.cpu().numpy(), self.mbuf.cpu().numpy()
        gd = np.concatenate([dbuf[:self.doff], dbuf[self.doff + self.n:]])
        gm = np.concatenate([mbuf[:self.moff], mbuf[self.moff + self.n:]])
        assert (gd == GUARD_F).all() and (gm == GUARD_M).all(), 'a write outside the frame'
        shape = self.img.shape
        return (dbuf[self.doff:self.doff + self.n].reshape(shape), mbuf[self.moff:self.moff + self.n].reshape(shape),
                self.st.cpu().numpy())


def run(ctx, name, sigclip, sigfrac, niter, feed=False, rn=P.RN, d_rdn16=None, data_off=4):
    fr = Frame(ctx, name, data_off=data_off)
    ctx.set_lac_level_feed(feed)
    try:
        _lib.check(fr.call(ctx, sigclip, sigfrac, niter, rn, d_rdn16), 'bbx_lacosmic', ctx.h)
        ctx.sync()
    finally:
        ctx.set_lac_level_feed(False)
    return fr


def assert_equals_oracle(fr, sigclip, sigfrac, niter, rn=P.RN):
    cr, clean, iters, nobj = P.oracle(fr.name, sigclip, sigfrac, niter, rn=rn)
    d, m, st = fr.results()
    got_cr = (m & 2) != 0
    print('%s sigclip %g niter %d: oracle %r, %d pixels, %d objects; device %r' % (fr.name, sigclip, niter, iters, cr.sum(), nobj,
                                                                              list(st[:8])))
    assert np.array_equal(got_cr, cr), 'CR bit differs at %r' % (np.argwhere(got_cr != cr)[:10].tolist(),)
    assert np.array_equal(m & ~np.uint8(2), fr.mask)                      # every other mask bit unchanged
    assert np.array_equal(d.view(np.uint32), clean.view(np.uint32)), \
        'cleaned image differs at %r' % (np.argwhere(d.view(np.uint32) != clean.view(np.uint32))[:10].tolist(),)
    assert list(st[:len(iters)]) == iters
    assert not st[len(iters):6].any()                                     # (the oracle stops after an iteration without a new pixel)
    assert st[7] == cr.sum()
    assert st[6] == nobj
    return d, m, st


# ---- a. every scene, both candidate kernels' launch conditions as they fall, feed off / on, both parameter sets
CASES = [(name, 3) for name in P.SCENES] + [('bars', 1), ('bars', 6)]


@pytest.mark.parametrize('sigclip,sigfrac', P.PARAMS)
@pytest.mark.parametrize('feed', [False, True], ids=['nofeed', 'feed'])
@pytest.mark.parametrize('name,niter', CASES)
def test_scene(ctx, name, niter, feed, sigclip, sigfrac):
    fr = run(ctx, name, sigclip, sigfrac, niter, feed=feed)
    assert fr.vector()                                                    # every scene is 4 columns wide a multiple, aligned
    assert_equals_oracle(fr, sigclip, sigfrac, niter)


@pytest.mark.parametrize('feed', [False, True], ids=['nofeed', 'feed'])
def test_no_iteration(ctx, feed):
    """niter = 0: image and mask come back as they went in, the statistics are zero"""
    fr = run(ctx, 'seams', 15.0, 0.01, 0, feed=feed)
    d, m, st = fr.results()
    assert np.array_equal(d.view(np.uint32), fr.img.view(np.uint32)) and np.array_equal(m, fr.mask)
    assert not st[:8].any()


def test_niter_out_of_range_is_refused(ctx):
    fr = Frame(ctx, 'tiny')
    assert fr.call(ctx, 15.0, 0.01, 7) == BBX_ERR_ARG and fr.call(ctx, 15.0, 0.01, -1) == BBX_ERR_ARG
    ctx.sync()
    d, m, _ = fr.results()
    assert np.array_equal(d.view(np.uint32), fr.img.view(np.uint32)) and np.array_equal(m, fr.mask)


# ---- b. scalar fallback by pointer: nx % 4 == 0, the image 4 bytes off a 16-byte boundary
@pytest.mark.parametrize('sigclip,sigfrac', P.PARAMS)
@pytest.mark.parametrize('feed', [False, True], ids=['nofeed', 'feed'])
@pytest.mark.parametrize('name', ['dense', 'seams'])
def test_scalar_fallback_by_pointer(ctx, name, feed, sigclip, sigfrac):
    fr = run(ctx, name, sigclip, sigfrac, 3, feed=feed, data_off=1)
    assert fr.img.shape[1] % 4 == 0 and fr.d.data_ptr() % 16 == 4 and not fr.vector()
    assert_equals_oracle(fr, sigclip, sigfrac, 3)


@pytest.mark.parametrize('mask_off', [1, 2, 3])
def test_mask_off_four_bytes_is_refused(ctx, mask_off):
    fr = Frame(ctx, 'seams', mask_off=mask_off)
    assert fr.m.data_ptr() % 4 == mask_off
    assert fr.call(ctx, 15.0, 0.01, 3) == BBX_ERR_ARG
    ctx.sync()
    d, m, _ = fr.results()
    assert np.array_equal(d.view(np.uint32), fr.img.view(np.uint32)) and np.array_equal(m, fr.mask)


# ---- c. call order on one context: the flag plane is cleared by list, not by memset
@pytest.mark.parametrize('sigclip,sigfrac', P.PARAMS)
def test_scenes_of_one_shape_back_to_back(ctx, sigclip, sigfrac):
    assert P.SHAPES['streaks'] == P.SHAPES['dense']
    for name, niter in (('dense', 3), ('streaks', 6), ('dense', 3), ('streaks', 1), ('dense', 6)):
        assert_equals_oracle(run(ctx, name, sigclip, sigfrac, niter), sigclip, sigfrac, niter)


@pytest.mark.parametrize('sigclip,sigfrac', P.PARAMS)
def test_larger_frame_then_smaller(ctx, sigclip, sigfrac):
    for name, niter in (('seams', 3), ('tiny', 3), ('bars', 6), ('sliver', 3), ('one_tile', 3), ('tiny', 3)):
        assert_equals_oracle(run(ctx, name, sigclip, sigfrac, niter), sigclip, sigfrac, niter)


# ---- e. read noise from the 16 channel sigmas on the device
def rdn_vector(with_nan):
    v = 7.9 + 0.7 * np.random.RandomState(31).random_sample(16)
    v[3], v[12] = 7.9, 8.6
    if with_nan:
        v[[0, 8, 15]] = np.nan
    return v


@pytest.mark.parametrize('feed', [False, True], ids=['nofeed', 'feed'])
@pytest.mark.parametrize('with_nan', [False, True], ids=['finite', 'nan_0_8_15'])
def test_read_noise_from_the_channel_sigmas(ctx, with_nan, feed):
    v = rdn_vector(with_nan)
    assert v.dtype == np.float64 and np.isnan(v).sum() == (3 if with_nan else 0)
    assert np.nanmin(v) >= 7.9 and np.nanmax(v) <= 8.6
    rn = np.float32(np.nanmean(v))
    # the order of summation matters at this spread: the plain left-to-right sum differs in its last bits
    seq = 0.0
    for x in v[~np.isnan(v)]:
        seq += x
    print('nanmean %.17g, left-to-right %.17g, float32 %r' % (np.nanmean(v), seq / (~np.isnan(v)).sum(), rn))
    d_v = torch.from_numpy(v).to(ctx.device)
    for sigclip, sigfrac in P.PARAMS:
        a = run(ctx, 'seams', sigclip, sigfrac, 3, feed=feed, rn=0.0, d_rdn16=d_v)      # the scalar is ignored
        b = run(ctx, 'seams', sigclip, sigfrac, 3, feed=feed, rn=rn)
        da, ma, sa = assert_equals_oracle(a, sigclip, sigfrac, 3, rn=rn)
        db, mb, sb = assert_equals_oracle(b, sigclip, sigfrac, 3, rn=rn)
        assert np.array_equal(da.view(np.uint32), db.view(np.uint32)) and np.array_equal(ma, mb) and np.array_equal(sa[:8], sb[:8])
    assert np.array_equal(d_v.cpu().numpy().view(np.uint64), v.view(np.uint64))


def test_read_noise_decides_a_pixel(ctx):
    """the last bits of the read noise reach the result only through threshold decisions; a read noise far
    off the mean does change this scene, so the comparison above can tell a wrong mean at that scale"""
    lo, hi = P.oracle('seams', 4.5, 0.3, 3, rn=np.float32(7.9)), P.oracle('seams', 4.5, 0.3, 3, rn=np.float32(30.0))
    assert not np.array_equal(lo[0], hi[0])
    assert_equals_oracle(run(ctx, 'seams', 4.5, 0.3, 3, rn=30.0), 4.5, 0.3, 3, rn=30.0)


# ---- d. the frame after an overflowed frame
@pytest.fixture()
def own_ctx():
    """a context of its own: a flag plane left dirty here must not reach the other tests"""
    c = R.Context(0)
    yield c
    _lib.lib.bbx_set_option(c.h, BBX_OPT_DEBUG_LISTCAP, 0)
    c.close()


def overflow_bars(ctx, listcap):
    _lib.check(_lib.lib.bbx_set_option(ctx.h, BBX_OPT_DEBUG_LISTCAP, listcap), 'bbx_set_option')
    try:
        fr = Frame(ctx, 'bars')
        _lib.check(fr.call(ctx, 15.0, 0.01, 6), 'bbx_lacosmic', ctx.h)
        with pytest.raises(_lib.BBXError) as e:
            ctx.sync()
        assert e.value.code == BBX_ERR_OVERFLOW
    finally:
        _lib.check(_lib.lib.bbx_set_option(ctx.h, BBX_OPT_DEBUG_LISTCAP, 0), 'bbx_set_option')
    fr.results()                                                          # guards only: what an overflowed frame holds is unspecified


@pytest.mark.parametrize('listcap', [64, 24])
def test_frame_after_an_overflowed_frame(own_ctx, listcap):
    """`bars` with work lists of [listcap] entries overflows; the next frame of that shape on the context
    must be right.  The list of the dense pass is cut at either capacity.  At 64 the later iterations stay
    below it (30 to 40 candidates around the one seed that survives); at 24 k_lac_cand_sparse drops
    candidates of the second iteration after it has set their bit in the flag plane (a host replay of the
    clipped run: 32 candidates).  The frames that follow hold pixels that only k_lac_cand_sparse can queue and
    whose flag byte the first iteration neither writes nor clears (test_lacosmic_paths_host.py), each pixel
    around the left end of the bar in one of the eighteen.  Before k_lac_cand_sparse took the bit of a
    dropped pixel back, the case of 24 failed at `chain2`: [25, 8] new pixels per iteration against the
    oracle's [25, 12]; the case of 64 passed then as it does now."""
    ctx = own_ctx
    assert_equals_oracle(run(ctx, 'bars', 15.0, 0.01, 6), 15.0, 0.01, 6)
    for k in range(P.NCHAIN):
        overflow_bars(ctx, listcap)
        assert_equals_oracle(run(ctx, 'chain%d' % k, 15.0, 0.01, 3), 15.0, 0.01, 3)
    overflow_bars(ctx, listcap)
    assert_equals_oracle(run(ctx, 'bars', 15.0, 0.01, 6), 15.0, 0.01, 6)
    # and the streaks of (c) after an overflowed frame (a frame of more pixels: the plane is zeroed for it)
    overflow_bars(ctx, listcap)
    assert_equals_oracle(run(ctx, 'streaks', 15.0, 0.01, 6), 15.0, 0.01, 6)
