"""GPU: bbx_sat_trails on the scenes of tests/sattrail_paths.py -- every decision of the trail detector behind the
Canny front end, against oracle/sattrail.py detect / make_mask.  The device does the oracle's float64 operations in
the oracle's order, so every comparison is exact: the whole uint8 mask (bit 16 and every other bit, guard bytes around
it), NSATS, the eight words of d_info, and -- through bbx_sat_trails_state -- the decisions in between: accepted or
not, the refined line, the support's extent, the segment, the rotated frame, the start of the walk and every strip
it painted.  A wrong segment often paints the same mask (the walk runs both ways from its start), so the mask alone
would not tell.  That the scenes are on their paths is asserted on the CPU by tests/test_sattrail_paths_host.py.

Left to the full-size frame of tests/test_gpu_fullsize_zogy.py test_sat_trail_fullsize (frames are not enlarged here to
chase them): SAT_SEG_CAP (more than 8192 voters of one cell), SAT_MAXWIN (more than 1200 strips) and the capacity of the
edge list.  Unreached by any test: the band exit of k_sat_walk (BBX_ERR_NOTCONV when a window leaves the
2 x SAT_BANDH rows that were interpolated) -- no scene of up to 400 x 4000 pixels was found that takes the oracle's
walk that far, see sattrail_paths.BAND_EXIT_SEARCH.
"""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import sattrail_paths as P                 # noqa: E402
from blackbox_amd import _lib              # noqa: E402
from blackbox_amd import reduce as R       # noqa: E402

BBX_ERR_ARG = -1
NSTATE = 25
(ACCEPT, SEG_OK, FOUND, K, VOTES, RHO, T0, T1, TMIN, TMAX, ICPT, SLOPE, SEG, ROT_ROWS, ROT_COLS, SX, SY, BAND_R0, BAND_ROWS, NWIN,
 ROW_MIN, ROW_MAX) = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, slice(12, 16), 16, 17, 18, 19, 20, 21, 22, 23, 24)
GUARD_F, GUARD_M = np.float32(-7.25e30), np.uint8(0xA5)
DATA_OFF, MASK_OFF = 2, 4                  # floats: 8-byte, not 16-byte aligned (the entry allows it); bytes


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def sprinkled(shape):
    """a mask that already carries bits 1 and 32"""
    m = np.zeros(shape, np.uint8)
    m[::7, ::11] = 1
    m[3::13, 5::17] |= 32
    return m


class Frame:
    """image and mask of a scene on the device, each inside a larger buffer with guard values around it"""

    def __init__(self, ctx, name, mask0=None, data_off=DATA_OFF):
        self.name, self.img = name, P.make_scene(name)
        self.mask0 = sprinkled(self.img.shape) if mask0 is None else mask0
        ny, nx = self.img.shape
        n = ny * nx
        self.dbuf = torch.full((n + 8,), float(GUARD_F), dtype=torch.float32, device=ctx.device)
        self.mbuf = torch.full((n + 8,), int(GUARD_M), dtype=torch.uint8, device=ctx.device)
        assert self.dbuf.data_ptr() % 16 == 0 and self.mbuf.data_ptr() % 16 == 0
        self.d = self.dbuf[data_off:data_off + n].view(ny, nx)
        self.m = self.mbuf[MASK_OFF:MASK_OFF + n].view(ny, nx)
        self.d.copy_(torch.from_numpy(np.array(self.img)))
        self.m.copy_(torch.from_numpy(self.mask0))
        self.doff, self.n = data_off, n
        self.d_n = torch.full((1,), -1, dtype=torch.int32, device=ctx.device)
        self.d_info = torch.full((8,), -1.0, dtype=torch.float32, device=ctx.device)

    def call(self, ctx, ny=None, nx=None, ntheta=R.NTHETA_SAT, info=True):
        gw, gr = R.sat_gauss_weights()
        return _lib.lib.bbx_sat_trails(ctx.h, self.img.shape[0] if ny is None else ny, self.img.shape[1] if nx is None else nx,
                                       C.c_void_p(self.d.data_ptr()), C.c_void_p(self.m.data_ptr()), R.sat_cos_sin(), ntheta, gw, gr,
                                       C.c_void_p(self.d_n.data_ptr()), C.c_void_p(self.d_info.data_ptr() if info else 0), ctx.stream())

    def state(self, ctx):
        """bbx_sat_trails_state -> (the doubles, the strips as (r0, r1, c0, c1))"""
        st = (C.c_double * NSTATE)()
        rects = (C.c_int32 * (4 * 64))()
        ny, nx = self.img.shape
        _lib.check(_lib.lib.bbx_sat_trails_state(ctx.h, ny, nx, R.NTHETA_SAT, st, rects, 64, ctx.stream()), 'bbx_sat_trails_state', ctx.h)
        st = np.array(st[:])
        nwin = int(st[NWIN])
        assert 0 <= nwin <= 64
        return st, [tuple(rects[4 * i:4 * i + 4]) for i in range(nwin)]

    def results(self):
        """-> (mask, NSATS, d_info) on the host, after checking the guard values and that the frame itself is untouched"""
        dbuf, mbuf = self.dbuf.cpu().numpy(), self.mbuf.cpu().numpy()
        gd = np.concatenate([dbuf[:self.doff], dbuf[self.doff + self.n:]])
        gm = np.concatenate([mbuf[:MASK_OFF], mbuf[MASK_OFF + self.n:]])
        assert (gd == GUARD_F).all() and (gm == GUARD_M).all(), 'a write outside the frame'
        assert np.array_equal(dbuf[self.doff:self.doff + self.n].view(np.uint32), self.img.reshape(-1).view(np.uint32))
        return mbuf[MASK_OFF:MASK_OFF + self.n].reshape(self.img.shape), int(self.d_n.item()), self.d_info.cpu().numpy()


def run(ctx, name, mask0=None):
    fr = Frame(ctx, name, mask0)
    assert fr.d.data_ptr() % 16 == 8
    _lib.check(fr.call(ctx), 'bbx_sat_trails', ctx.h)
    ctx.sync()
    st, rects = fr.state(ctx)
    return fr, st, rects


def same(a, b):
    """float64 values equal as bits (NaN equals NaN, -0.0 does not equal 0.0)"""
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def assert_equals_oracle(fr, st, rects, nsats_want=None):
    rec = P.oracle(fr.name)
    info = rec.info
    mask, nsats, dinfo = fr.results()
    print('%s: oracle votes %d k %d rho %g, %s; device info %r, state %r, strips %r' % (
        fr.name, info['votes'], info['k'], info['rho'], sorted(k for k in info if k in ('refine', 'support', 'segment', 'windows')),
        dinfo.tolist(), st.tolist(), rects))
    # ---- the mask: bit 16 and every other bit
    want = fr.mask0 | (rec.mask * np.uint8(16))
    assert np.array_equal(mask, want), 'mask differs at %r' % (np.argwhere(mask != want)[:10].tolist(),)
    assert nsats == (rec.nsats if nsats_want is None else nsats_want)
    # ---- d_info
    assert dinfo[0] == np.float32(info['bmax']) and dinfo[1] == np.float32(info['bmin'])
    assert dinfo[2] == info['votes'] and dinfo[3] == info['k'] and dinfo[4] == info['rho']
    assert dinfo[5] == len(rec.painted) and dinfo[6] == (1 if rec.seg_ok else 0) and dinfo[7] == (1 if rec.nsats > 0 else 0)
    # ---- the decisions in between
    assert st[ACCEPT] == (1 if 'segment' in info else 0) and st[SEG_OK] == dinfo[6] and st[FOUND] == dinfo[7]
    assert st[K] == info['k'] and st[VOTES] == info['votes'] and st[RHO] == info['rho']
    if 'refine' in info:
        assert same(st[[ICPT, SLOPE]], info['refine'][:2])
    if 'support' in info:
        tmin, tmax, span = info['support']
        assert same(st[[TMIN, TMAX]], [tmin, tmax]) and same(st[[T0, T1]], span)
    else:
        assert np.isnan(st[TMIN]) and np.isnan(st[TMAX])
    if 'segment' not in info:
        # nothing of a frame before: the fields this frame did not reach read as zero
        assert st[NWIN] == 0 and rects == [] and not st[SEG].any() and not st[[ROT_ROWS, ROT_COLS, SX, SY, BAND_R0, BAND_ROWS]].any()
        return
    assert st[SEG].tolist() == [info['segment'][0][0], info['segment'][0][1], info['segment'][1][0], info['segment'][1][1]]
    assert (st[ROT_ROWS], st[ROT_COLS]) == rec.rot_shape
    assert same(st[[SX, SY]], rec.start)
    r0 = min(max(int(rec.start[1]) - P.SAT_BANDH, 0), rec.rot_shape[0])
    r1 = max(min(int(rec.start[1]) + P.SAT_BANDH, rec.rot_shape[0]), r0)
    assert (st[BAND_R0], st[BAND_ROWS]) == (r0, r1 - r0)
    assert rects == rec.rects() and st[NWIN] == len(rec.painted)
    if rects:
        assert st[ROW_MIN] == min(r[0] for r in rects) and st[ROW_MAX] == max(r[1] for r in rects)


@pytest.mark.parametrize('name', list(P.SCENES))
def test_scene(ctx, name):
    fr, st, rects = run(ctx, name)
    assert_equals_oracle(fr, st, rects)
    if name in P.REJECTED:
        mask, nsats, _ = fr.results()
        assert np.array_equal(mask, fr.mask0) and nsats == 0


def test_state_between_calls():
    """an accepted frame, the empty edge list, a line with too few votes, a larger frame (the workspace is regrown), a tall
    one (the same pixels in another layout) and the first again on one context: each result equals the one from a context
    that has seen nothing else, and the read-out after a rejected frame shows that frame, not the one before it"""
    order = ['support_in', 'no_edges', 'votes_low', 'gap_small', 'theta_le45', 'support_in']
    assert P.make_scene('gap_small').size > P.make_scene('support_in').size == P.make_scene('theta_le45').size
    fresh = {}
    for name in sorted(set(order)):
        c = R.Context(0)
        try:
            fr, st, rects = run(c, name)
            fresh[name] = (fr.results(), st, rects)
        finally:
            c.close()
    c = R.Context(0)
    try:
        for name in order:
            fr, st, rects = run(c, name)
            (mask, nsats, dinfo), st0, rects0 = fresh[name]
            got = fr.results()
            assert np.array_equal(got[0], mask) and got[1] == nsats and np.array_equal(got[2], dinfo), name
            assert same(st, st0) and rects == rects0, name
            assert_equals_oracle(fr, st, rects)
            if name in ('no_edges', 'votes_low'):
                assert st[ACCEPT] == 0 and st[NWIN] == 0 and st[SEG_OK] == 0 and st[FOUND] == 0 and rects == []
    finally:
        c.close()


def test_mask_that_already_carries_bit_16(ctx):
    """a small blob of bit 16 away from the trail: the trail's pixels are OR-ed in, every other pixel stays.  NSATS is
    bbx_count_objects of bit 16 over the whole mask -- the blob counts; the oracle's sat_detect labels only the pixels
    it adds itself, so its count is one less here."""
    name = 'support_in'
    mask0 = sprinkled(P.make_scene(name).shape)
    mask0[500:506, 100:108] |= 16
    rec = P.oracle(name)
    assert not rec.mask[480:526, 80:128].any() and rec.nsats == 1
    want = mask0 | (rec.mask * np.uint8(16))
    nlab = ndimage.label((want & 16) != 0, structure=np.ones((3, 3), bool))[1]
    assert nlab == 2
    fr, st, rects = run(ctx, name, mask0)
    assert_equals_oracle(fr, st, rects, nsats_want=nlab)


BAD = {'odd_ny': dict(ny=599), 'odd_nx': dict(nx=899), 'ny_below_8': dict(ny=6), 'ntheta_3': dict(ntheta=3), 'ntheta_4097': dict(ntheta=4097),
       'null_info': dict(info=False), 'frame_4_byte_aligned': dict()}


@pytest.mark.parametrize('what', sorted(BAD))
def test_bad_arguments(ctx, what):
    """BBX_ERR_ARG before anything is launched: the mask, its guards, NSATS and d_info stay as they were"""
    fr = Frame(ctx, 'support_in', data_off=1 if what == 'frame_4_byte_aligned' else DATA_OFF)
    assert fr.d.data_ptr() % 8 == (4 if what == 'frame_4_byte_aligned' else 0)
    assert fr.call(ctx, **BAD[what]) == BBX_ERR_ARG
    ctx.sync()
    mask, nsats, dinfo = fr.results()
    assert np.array_equal(mask, fr.mask0) and nsats == -1 and (dinfo == -1.0).all()


def test_read_out_refuses_what_was_not_run():
    """no bbx_sat_trails call on the context yet, or a frame larger than the one that ran: BBX_ERR_ARG"""
    c = R.Context(0)
    try:
        st = (C.c_double * NSTATE)()
        rects = (C.c_int32 * 4)()
        L = _lib.lib
        assert L.bbx_sat_trails_state(c.h, 600, 900, R.NTHETA_SAT, st, rects, 1, c.stream()) == BBX_ERR_ARG
        run(c, 'support_in')
        assert L.bbx_sat_trails_state(c.h, 600, 900, R.NTHETA_SAT, st, rects, 1, c.stream()) == 0 and st[NWIN] >= 5
        assert L.bbx_sat_trails_state(c.h, 2400, 3600, R.NTHETA_SAT, st, rects, 1, c.stream()) == BBX_ERR_ARG
        assert L.bbx_sat_trails_state(c.h, 600, 901, R.NTHETA_SAT, st, rects, 1, c.stream()) == BBX_ERR_ARG
        assert L.bbx_sat_trails_state(c.h, 600, 900, R.NTHETA_SAT, None, rects, 1, c.stream()) == BBX_ERR_ARG
        assert L.bbx_sat_trails_state(c.h, 600, 900, R.NTHETA_SAT, st, None, 1, c.stream()) == BBX_ERR_ARG
    finally:
        c.close()
