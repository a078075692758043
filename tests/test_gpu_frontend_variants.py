"""GPU: every kernel variant of the calibration front end (bbx_overscan.hip, bbx_calibrate.hip) at small shapes
against the float64 numpy restatements of tests/frontend_ref.py (held against the oracle's os_corr / mask_init
in tests/test_frontend_restatement.py).

The front end picks its kernels by geometry and pointer alignment.  Each test asserts the conditions of the
variant it means to run (the launch conditions are quoted next to the asserts), so that a change of geometry
cannot silently move it to another variant.  Bars: counts, masks, copies and calibrated pixels bit-exact; row
means rel 1e-12; read noise as stated at RDN_REL."""
import ctypes as C
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import bbx_oracle as O                                  # noqa: E402
import frontend_ref as F                                # noqa: E402
from test_nonlin import make_splines                    # noqa: E402
from blackbox_amd import _lib, settings                 # noqa: E402
from blackbox_amd import reduce as R                    # noqa: E402
from blackbox_amd._lib import lib                       # noqa: E402

TEL = 'ML1'
GAIN, SATLEVEL = settings.gain[TEL], settings.satlevel[TEL]
G32 = _lib.f32x16(GAIN)
YS, XS, OS_Y = F.YS, F.XS, F.OS_Y
BBX_ERR_ARG = -1
# read noise against the float64 restatement.  The project's bar for RDN is rel 1e-6 (test_golden_reduction); the largest
# difference seen over the channels, geometries and raw types of test_read_noise is 1.23e-10 (scalar path, a channel
# whose fit is zero: the kernel's one-pass variance q/n - mean^2 cancels six digits there), so the bar is 100 x that
RDN_REL = 1.25e-8


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def hv(h, k):
    return R.hval(h, k)


def overscan_stats(ctx, d_raw, ys=YS, xs=XS):
    geom = R.geometry(d_raw.shape, ys, xs)
    dy, dx = d_raw.shape[0] // 2, d_raw.shape[1] // 8
    d_mean = torch.full((16, dy), -1.0, dtype=torch.float64, device=ctx.device)
    d_hos = torch.full((16, dy - ys - 10, dx), -1.0, dtype=torch.float32, device=ctx.device)
    d_ninf = torch.full((1,), -1, dtype=torch.int64, device=ctx.device)
    rc = lib.bbx_overscan_stats(ctx.h, C.byref(geom), R._ptr(d_raw), R.raw_type_of(d_raw), G32, R._ptr(d_mean), R._ptr(d_hos),
                                R._ptr(d_ninf), ctx.stream())
    if rc != 0:
        return rc, None, None, None
    ctx.sync()
    return rc, d_mean.cpu().numpy(), d_hos.cpu().numpy(), int(d_ninf.item())


# ---- row statistics and the horizontal-overscan copy ------------------------------------------------------------
@pytest.mark.parametrize('os_x', sorted(F.STRIP_SEEDS))
def test_row_statistics_and_hos_copy(ctx, os_x):
    """bbx_overscan_stats launches k_vos_rowstats16<*, 11> for vos_w <= 176, k_vos_rowstats16<*, 16> for
    vos_w <= 256 and the 64-lane k_vos_rowstats up to 512 (vos_w = os_x - 6)"""
    vos_w = os_x - 6
    assert vos_w == {45: 39, 182: 176, 183: 177, 262: 256, 263: 257, 518: 512}[os_x]
    fr = F.strip_frame(os_x)
    c0, r0 = fr['dead']
    want = F.row_means(fr['u16'], GAIN, YS, XS)
    want_hos = F.hos_copy(fr['u16'], GAIN, YS, XS)
    assert np.isnan(want[c0, r0]) and np.isnan(want).sum() == 1
    got = {}
    for kind, raw in (('u16', fr['u16']), ('f32', fr['u16'].astype(np.float32))):
        rc, mean, hos, ninf = overscan_stats(ctx, dev(ctx, raw))
        assert rc == 0
        got[kind] = mean
        assert np.array_equal(np.isnan(mean), np.isnan(want)), kind
        ok = ~np.isnan(want)
        print('os_x %d %s: max rel diff of the row means %.3g' % (os_x, kind, np.max(np.abs(mean[ok] / want[ok] - 1))))
        np.testing.assert_allclose(mean[ok], want[ok], rtol=1e-12, atol=0)
        assert np.array_equal(hos, want_hos), kind                # float32 copy: bit-exact
        assert ninf == 0
    assert np.array_equal(got['u16'], got['f32'], equal_nan=True)    # the two raw types: bit-identical
    # float32 with NaN / Inf in the strip, the horizontal-overscan rows and the data sections
    rc, mean, hos, ninf = overscan_stats(ctx, dev(ctx, fr['f32nan']))
    want = F.row_means(fr['f32nan'], GAIN, YS, XS)
    assert rc == 0 and ninf == fr['n_infnan']
    assert np.array_equal(np.isnan(mean), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(mean[ok], want[ok], rtol=1e-12, atol=0)
    assert np.array_equal(hos, F.hos_copy(fr['f32nan'], GAIN, YS, XS))


def test_row_statistics_refuse_a_strip_wider_than_512(ctx):
    raw = torch.zeros((2 * (YS + OS_Y), 8 * (XS + 519)), dtype=torch.uint16, device=ctx.device)
    assert raw.shape[1] // 8 - XS - 6 == 513
    assert overscan_stats(ctx, raw)[0] == BBX_ERR_ARG


# ---- read noise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', sorted(F.RDN_GEOMS))
def test_read_noise(ctx, path):
    """k_vos_std_pass reads float4 when dy * vos_w % 4 == 0 and scalars otherwise.  Per channel: vfit a cubic near
    the data, zero (a failed fit: mean >> sigma) or 500 e- off; dlevel != 0; channels whose clip loop stops after
    pass 1 (nothing clipped) and channels that clip in all five passes (frontend_ref.rdn_frame)"""
    os_y, os_x = F.RDN_GEOMS[path]
    dy, vos_w = YS + os_y, os_x - 6
    assert ((dy * vos_w) % 4 == 0) == (path == 'float4')         # `if (total % 4 == 0)` in k_vos_std_pass
    fr = F.rdn_frame(os_y, os_x)
    want = F.read_noise(fr['u16'], GAIN, fr['vfit'], fr['dlevel'], YS, XS)
    passes = F.read_noise_passes(fr['u16'], GAIN, fr['vfit'], fr['dlevel'], YS, XS)
    assert all(passes[c] == 0 for c in F.RDN_FROZEN) and all(passes[c] == 5 for c in F.RDN_FIVE)
    d_vfit = dev(ctx, fr['vfit'].reshape(-1))
    dl = _lib.f32x16(np.float32(fr['dlevel']))
    got = {}
    for kind, raw in (('u16', fr['u16']), ('f32', fr['u16'].astype(np.float32))):
        d_raw = dev(ctx, raw)
        geom = R.geometry(raw.shape, YS, XS)
        d_std = torch.full((16,), -1.0, dtype=torch.float64, device=ctx.device)
        for _ in range(2):                                       # twice: the ping-pong state must not carry over
            _lib.check(lib.bbx_vos_std(ctx.h, C.byref(geom), R._ptr(d_raw), R.raw_type_of(d_raw), G32, R._ptr(d_vfit), dl,
                                       R._ptr(d_std), ctx.stream()), 'bbx_vos_std', ctx.h)
            ctx.sync()
            got[kind] = d_std.cpu().numpy()
            rel = np.abs(got[kind] / want - 1)
            print('%s %s: max rel diff of the read noise %.3g (channel %d)' % (path, kind, rel.max(), int(rel.argmax())))
            np.testing.assert_allclose(got[kind], want, rtol=RDN_REL, atol=0)
    assert np.array_equal(got['u16'], got['f32'])


# ---- saturated columns --------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', F.SATCOL_ROWS)
def test_saturated_column_counts(ctx, rows):
    """k_satcol: `v >= thr`, rows counted from the overscan edge in blocks of 64 (rows2 = 10, 70, 96), pixels exactly at
    the threshold and one float32 ulp below it, lower and upper channels that differ, a vfit that varies by row"""
    rows1, rows2 = rows
    ys = F.SATCOL_YS
    fr = F.satcol_frame()
    want = F.satcol_counts(fr['u16'], GAIN, fr['vfit'], fr['thr'], rows1, rows2, ys, XS)
    assert want[1].max() >= min(rows2, 12) and (want[0] != want[1]).any()
    d_vfit = dev(ctx, fr['vfit'].reshape(-1))
    thr = _lib.f32x16(fr['thr'])
    for raw in (fr['u16'], fr['u16'].astype(np.float32)):
        d_raw = dev(ctx, raw)
        geom = R.geometry(raw.shape, ys, XS)
        d_cnt = torch.full((2, 16, XS), -1, dtype=torch.int32, device=ctx.device)
        _lib.check(lib.bbx_satcol_counts(ctx.h, C.byref(geom), R._ptr(d_raw), R.raw_type_of(d_raw), G32, R._ptr(d_vfit), thr,
                                         rows1, rows2, R._ptr(d_cnt), ctx.stream()), 'bbx_satcol_counts', ctx.h)
        ctx.sync()
        assert np.array_equal(d_cnt.cpu().numpy(), want), raw.dtype
    if rows2 == ys:
        assert lib.bbx_satcol_counts(ctx.h, C.byref(geom), R._ptr(d_raw), R.raw_type_of(d_raw), G32, R._ptr(d_vfit), thr,
                                     rows1, ys + 1, R._ptr(d_cnt), ctx.stream()) == BBX_ERR_ARG


# ---- calibrate: the vector variant and the scalar variant on the same inputs --------------------------------------
@pytest.fixture(scope='module')
def calib():
    cs = F.calib_case()
    cs['splines'] = make_splines()
    cs['sat'] = np.float32(np.array(SATLEVEL) * np.array(GAIN) - cs['biasm'])
    cs['header'] = {'BIASM%d' % (c + 1): float(cs['biasm'][c]) for c in range(16)}
    return cs


def off_aligned(ctx, a):
    """the same values one element off 16-byte alignment: a contiguous view into a larger buffer"""
    t = dev(ctx, a)
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize('nonlin', [False, True])
@pytest.mark.parametrize('rawkind', ['u16', 'f32', 'f32nan'])
def test_calibrate_vector_and_scalar(ctx, calib, rawkind, nonlin):
    """bbx_calibrate launches k_calibrate_v4<RAW, NONLIN> when
        xsz % 4 == 0 && dx % 4 == 0 && ysz % 8 == 0 && raw, data, flat, bias % 16 == 0 && mask, bpm % 4 == 0
    and k_calibrate_s otherwise.  Masters: none, flat + BPM, bias, bias + flat + BPM; a flat with a zero, a bias with
    NaN and with values that put pixels exactly on the saturation threshold.  Data and mask bit-exact against the
    restatement; the scalar kernel (raw one element off alignment) bit-identical to the vector kernel."""
    ys, xs, os_y, os_x = F.CAL_GEOM
    assert xs % 4 == 0 and (xs + os_x) % 4 == 0 and ys % 8 == 0
    cs = calib
    raw = {'u16': cs['u16'], 'f32': cs['u16'].astype(np.float32), 'f32nan': cs['f32nan']}[rawkind]
    spl = cs['splines'] if nonlin else None
    geom = R.geometry(raw.shape, ys, xs)
    sol = R.OverscanSolution()
    sol.d_vfit, sol.d_oscan = dev(ctx, cs['vfit'].reshape(-1)), dev(ctx, cs['oscan'].reshape(-1))
    d_raw, d_raw_off = dev(ctx, raw), off_aligned(ctx, raw)
    d_flat, d_bpm = dev(ctx, cs['flat']), dev(ctx, cs['bpm'])
    nobias, _ = F.calibrate(raw, GAIN, cs['vfit'], cs['oscan'], cs['sat'], ys, xs, splines=spl)
    bias = F.plant_bias_on_sat(cs['bias'], nobias, cs['sat'], ys, xs)
    d_bias = dev(ctx, bias)
    out = (torch.empty((2 * ys, 8 * xs), dtype=torch.float32, device=ctx.device),
           torch.empty((2 * ys, 8 * xs), dtype=torch.uint8, device=ctx.device))
    assert d_raw.data_ptr() % 16 == 0 and out[0].data_ptr() % 16 == 0 and out[1].data_ptr() % 4 == 0
    assert d_flat.data_ptr() % 16 == 0 and d_bias.data_ptr() % 16 == 0 and d_bpm.data_ptr() % 4 == 0
    R.set_nonlin(ctx, spl)
    try:
        for masters in F.MASTERS:
            kw = dict(mflat=d_flat if 'flat' in masters else None, bpm=d_bpm if 'bpm' in masters else None,
                      mbias=d_bias if 'bias' in masters else None)
            want_d, want_m = F.calibrate(raw, GAIN, cs['vfit'], cs['oscan'], cs['sat'], ys, xs, splines=spl,
                                         bias=bias if 'bias' in masters else None, flat=cs['flat'] if 'flat' in masters else None,
                                         bpm=cs['bpm'] if 'bpm' in masters else None)
            # (nonlin_corr halves every pixel above 50000 counts, sic: with it only the planted pixels saturate)
            if not nonlin:
                assert ((want_m & 4) != 0).sum() > 100
            if 'bias' in masters:
                assert want_m[33, 650] & 4 and want_m[90, 1931] & 4 and not np.isfinite(bias[30, 500])
            res = {}
            for variant, r in (('v4', d_raw), ('s', d_raw_off)):
                out[0].fill_(-7.0); out[1].fill_(255)
                hdr = dict(cs['header'])
                R.calibrate(ctx, r, sol, hdr, {}, TEL, geom, out=out, **kw)
                ctx.sync()
                res[variant] = (out[0].cpu().numpy(), out[1].cpu().numpy())
                assert np.array_equal(res[variant][1], want_m), (masters, variant)
                assert np.array_equal(res[variant][0], want_d, equal_nan=True), (masters, variant)
            assert np.array_equal(res['v4'][0], res['s'][0], equal_nan=True) and np.array_equal(res['v4'][1], res['s'][1])
    finally:
        R.set_nonlin(ctx, None)


# ---- the saturated-pixel queue of the vector variant ----------------------------------------------------------
@pytest.mark.parametrize('kind', ['round', 'blocks'])
def test_saturated_pixel_queue_vector_variant(ctx, kind):
    """k_calibrate_v4 queues its saturated pixels with one reservation per wave (prefix sum over the lanes' satbits):
    > 1 % saturated pixels as blobs ('round': the frame of test_saturated_frame_one_percent at this geometry) and as
    rectangles that fill whole 4-pixel groups and 8-row strips ('blocks': up to 32 bits per lane); calibrate +
    mask_init_finish == the oracle's mask_init, NOBJ-SAT included"""
    ys, xs, os_y, os_x = F.CAL_GEOM
    assert xs % 4 == 0 and (xs + os_x) % 4 == 0 and ys % 8 == 0      # the vector variant's geometry
    case, rawf = F.blob_frame(kind)
    geom = R.geometry(rawf.shape, ys, xs)
    header, hm = {}, {}
    R.gain_corr(header, TEL)
    d_raw = dev(ctx, rawf)
    sol = R.os_solve(ctx, d_raw, header, TEL, geom)
    bpm, flat = dev(ctx, case['bpm']), dev(ctx, case['flat'])
    out = (torch.empty((2 * ys, 8 * xs), dtype=torch.float32, device=ctx.device),
           torch.empty((2 * ys, 8 * xs), dtype=torch.uint8, device=ctx.device))
    assert d_raw.data_ptr() % 16 == 0 and out[0].data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0
    assert out[1].data_ptr() % 4 == 0 and bpm.data_ptr() % 4 == 0
    data, mask = R.calibrate(ctx, d_raw, sol, header, hm, TEL, geom, mflat=flat, bpm=bpm, out=out)
    d_nobj = R.mask_init_finish(ctx, mask, header, hm, geom)
    ctx.sync()
    o = rawf.copy()
    O.gain_corr(o, GAIN, ys, xs)
    o_os, oh, _ = O.os_corr(o, ys, xs, tel=TEL, gain=GAIN, satlevel=SATLEVEL)
    o_mask, _ = O.mask_init(o_os, oh, case['bpm'], GAIN, SATLEVEL, ys, xs)
    frac = ((o_mask & 4) != 0).mean()
    assert 0.01 < frac and ((o_mask & 4) != 0).sum() < o_mask.size // 8 + 4096      # > 1 % saturated, no overflow
    assert ((o_mask & 8) != 0).sum() > 0
    assert np.array_equal(mask.cpu().numpy(), o_mask)
    assert int(d_nobj.item()) == int(oh['NOBJ-SAT'])


def test_saturated_pixel_queue_overflow_vector_variant(ctx):
    """four whole channels saturated (3, 4, 11, 12): more than npix / 8 + 4096 pixels, the queue of k_calibrate_v4 overflows
    (`base + cnt > satcap`) -> MASK-P False, every other step ran, and the next ordinary frame on the same context is
    fully green (modelled on test_device_side_overflow_flags_the_step_only)"""
    ys, xs, os_y, os_x = F.CAL_GEOM
    assert xs % 4 == 0 and (xs + os_x) % 4 == 0 and ys % 8 == 0
    case = F.e2e_case(os_x)
    raw = case['raw'].copy()
    secs = O.define_sections(raw.shape, ys, xs)
    dsec, red = secs[1], secs[4]
    chans = (3, 4, 11, 12)
    for c in chans:
        # 64000 ADU times the flat: every pixel above its channel's threshold, and a smooth plateau after the flat division.
        # (A constant 65535 divided by the flat's 0.5 % pixel noise is a field of 700 e- spikes: a candidate of LA-Cosmic in
        # every other pixel, whose own list then overflows as well -- COSMIC-P False, as designed, but not this test's subject)
        raw[dsec[c]] = np.floor(64000.0 * case['flat'][red[c]].astype(np.float64) + 0.5)
        assert raw[dsec[c]].min() > 1.03 * SATLEVEL[c] and raw[dsec[c]].max() < 65535
    assert 4 * ys * xs > (16 * ys * xs) // 8 + 4096
    coeffs = O.xtalk_coeffs(case['xtalk'])
    flags = ('GAIN-P', 'OS-P', 'MFLAT-P', 'MASK-P', 'COSMIC-P', 'XTALK-P', 'SAT-P')

    def run(r):
        d_raw, flat, bpm = dev(ctx, r), dev(ctx, case['flat']), dev(ctx, case['bpm'])
        assert d_raw.data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0 and bpm.data_ptr() % 4 == 0
        return R.reduce_object(ctx, d_raw, {}, TEL, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, ysize_chan=ys,
                               xsize_chan=xs, log=logging.getLogger('t'))
    d, m, h, hm = run(raw)
    assert hv(h, 'MASK-P') is False
    for k in flags:
        if k != 'MASK-P':
            assert hv(h, k) is True, k
    sat = (m.cpu().numpy() & 4) != 0
    for c in chans:
        assert sat[red[c]].all()                                   # the mask bits themselves do not go through the queue
    d2, m2, h2, _ = run(case['raw'])
    for k in flags:
        assert hv(h2, k) is True, k


# ---- end to end at the vector geometry --------------------------------------------------------------------------
def check_header_vos(header, oh, skip=()):
    for c in range(16):
        assert hv(header, 'VFITOK%d' % (c + 1)) == oh['VFITOK%d' % (c + 1)], c
        if c in skip:
            continue
        assert hv(header, 'BIASM%d' % (c + 1)) == pytest.approx(oh['BIASM%d' % (c + 1)], rel=1e-12), c
        for k in range(4):
            assert hv(header, 'BIAS%dA%d' % (c + 1, k)) == pytest.approx(oh['BIAS%dA%d' % (c + 1, k)], rel=1e-6, abs=1e-12)


@pytest.mark.parametrize('os_x', F.E2E_OS_X)
def test_reduce_object_at_the_vector_geometry(ctx, os_x):
    """reduce_object (flat + BPM, no cosmics, no trails) == gain_corr, os_corr, mask_init, / flat, edge_fill of the
    oracle, at the tolerances of test_golden_reduction.  os_x = 180, 200, 300: the vertical fit is fed by
    k_vos_rowstats16<*, 11>, k_vos_rowstats16<*, 16> and k_vos_rowstats in turn; k_calibrate_v4 in all three"""
    ys, xs = YS, XS
    assert xs % 4 == 0 and (xs + os_x) % 4 == 0 and ys % 8 == 0
    assert (os_x - 6 <= 176, os_x - 6 <= 256) == {180: (True, True), 200: (False, True), 300: (False, False)}[os_x]
    case = F.e2e_case(os_x)
    d_raw, flat, bpm = dev(ctx, case['raw']), dev(ctx, case['flat']), dev(ctx, case['bpm'])
    assert d_raw.data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0 and bpm.data_ptr() % 4 == 0
    geom = R.geometry(case['raw'].shape, ys, xs)
    o_os, o_data, o_mask, oh = F.oracle_chain(case, 'bn32')
    oh64 = F.oracle_chain(case, 'f64')[3]
    # overscan only: float32 pixels bit-exact (f32seq accumulation = the oracle's 'bn32')
    header = {}
    R.gain_corr(header, TEL)
    sol = R.os_solve(ctx, d_raw, header, TEL, geom)
    data_os, _ = R.calibrate(ctx, d_raw, sol, header, {}, TEL, geom)
    ctx.sync()
    assert np.array_equal(data_os.cpu().numpy(), o_os)
    check_header_vos(header, oh)
    for c in range(16):
        assert hv(header, 'RDN%d' % (c + 1)) == pytest.approx(oh['RDN%d' % (c + 1)], rel=1e-4)
        assert hv(header, 'RDN%d' % (c + 1)) == pytest.approx(oh64['RDN%d' % (c + 1)], rel=1e-6)
    assert hv(header, 'RDNOISE') == pytest.approx(oh['RDNOISE'], rel=1e-4)
    assert hv(header, 'BIASMEAN') == pytest.approx(oh['BIASMEAN'], rel=1e-12)
    # the whole chain
    data, mask, h, hm = R.reduce_object(ctx, d_raw, {}, TEL, mflat=flat, bpm=bpm, ysize_chan=ys, xsize_chan=xs,
                                        do_cosmics=False, detect_sats=False)
    got = data.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy(), o_mask)
    assert hv(h, 'NOBJ-SAT') == oh['NOBJ-SAT'] and oh['NOBJ-SAT'] > 0
    np.testing.assert_allclose(got, o_data, rtol=1.2e-7, atol=0)
    assert (got != o_data).mean() <= 1e-6


# ---- a channel whose vertical overscan reads zero ----------------------------------------------------------------
def test_dead_vertical_overscan(ctx):
    """os_corr 6480-6490: sigma_clipped_stats(mask_value=0) raises on a strip that is all zero and the reference takes
    the row means without the mask value: 0.0 -> BIASM 0.0, VFITOK True, RDN 0.0 for that channel.  The row kernel
    marks rows without a valid value with NaN; the host puts the reference's fallback back (overscan.dead_vos_rows)"""
    ys, xs, os_x = YS, XS, 180
    c0 = F.DEAD_CHAN
    case = F.e2e_case(os_x, dead=True)
    d_raw, flat, bpm = dev(ctx, case['raw']), dev(ctx, case['flat']), dev(ctx, case['bpm'])
    o_os, o_data, o_mask, oh = F.oracle_chain(case, 'bn32')
    oh64 = F.oracle_chain(case, 'f64')[3]
    assert oh64['BIASM%d' % (c0 + 1)] == 0.0 and oh64['RDN%d' % (c0 + 1)] == 0.0 and oh64['VFITOK%d' % (c0 + 1)] is True
    data, mask, h, hm = R.reduce_object(ctx, d_raw, {}, TEL, mflat=flat, bpm=bpm, ysize_chan=ys, xsize_chan=xs,
                                        do_cosmics=False, detect_sats=False)
    print('dead channel: OS-P %r' % hv(h, 'OS-P'), ['%s %r' % (k, hv(h, k % (c0 + 1))) for k in ('BIASM%d', 'RDN%d', 'VFITOK%d')])
    assert hv(h, 'OS-P') is True
    assert hv(h, 'BIASM%d' % (c0 + 1)) == 0.0 and hv(h, 'VFITOK%d' % (c0 + 1)) is True
    assert hv(h, 'RDN%d' % (c0 + 1)) == 0.0
    check_header_vos(h, oh, skip=(c0,))
    for c in range(16):
        assert hv(h, 'RDN%d' % (c + 1)) == pytest.approx(oh64['RDN%d' % (c + 1)], rel=1e-6), c
    assert hv(h, 'RDNOISE') == pytest.approx(oh64['RDNOISE'], rel=1e-4)
    assert hv(h, 'BIASMEAN') == pytest.approx(oh['BIASMEAN'], rel=1e-12)
    got = data.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy(), o_mask)
    np.testing.assert_allclose(got, o_data, rtol=1.2e-7, atol=0)
    assert (got != o_data).mean() <= 1e-6


def test_dead_vertical_overscan_pipeline_equals_serial(ctx):
    """the same frame through the frames-in-flight path (fits in the worker pool): pixels, mask and header equal the
    serial reduce_object's (the check of test_pipeline_equals_serial)"""
    from blackbox_amd.pipeline import FramePipeline, HostPool
    ys, xs, os_x = YS, XS, 180
    cases = [F.e2e_case(os_x, dead=True), F.e2e_case(os_x)]
    flat, bpm = dev(ctx, cases[0]['flat']), dev(ctx, cases[0]['bpm'])
    raws = [dev(ctx, c['raw']) for c in cases]
    geom = R.geometry(cases[0]['raw'].shape, ys, xs)
    serial = []
    for raw in raws:
        d, m, h, _ = R.reduce_object(ctx, raw, {}, TEL, mflat=flat, bpm=bpm, exptime=60.0, ysize_chan=ys, xsize_chan=xs,
                                     detect_sats=False)
        serial.append((d.cpu().numpy(), m.cpu().numpy(), h))
    assert hv(serial[0][2], 'BIASM%d' % (F.DEAD_CHAN + 1)) == 0.0 and hv(serial[0][2], 'OS-P') is True
    pool = HostPool(2)
    got = {}
    try:
        pipe = FramePipeline(ctx, TEL, geom, mflat=flat, bpm=bpm, exptime=60.0, pool=pool, depth=2, lanes=2, do_finish=True,
                             keep_outputs=True)
        try:
            n = pipe.run([(r, {}) for r in raws], on_done=lambda i, f: got.__setitem__(i, (f.data.cpu().numpy(), f.mask.cpu().numpy(), f.header)))
        finally:
            pipe.close()
    finally:
        pool.close()
    assert n == 2 and sorted(got) == [0, 1]
    keys = ['BIASMEAN', 'RDNOISE', 'NOBJ-SAT', 'NCOSMICS', 'N-INFNAN', 'OS-P'] + \
           ['%s%d' % (p, c + 1) for p in ('BIASM', 'RDN', 'VFITOK') for c in range(16)] + \
           ['BIAS%dA%d' % (c + 1, j) for c in range(16) for j in range(4)]
    for k in range(2):
        assert np.array_equal(serial[k][1], got[k][1]), 'frame %d: mask' % k
        assert np.array_equal(serial[k][0], got[k][0]), 'frame %d: pixels' % k
        for key in keys:
            assert hv(serial[k][2], key) == hv(got[k][2], key), (k, key)
