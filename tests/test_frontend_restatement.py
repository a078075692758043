"""CPU: the numpy restatements of the calibration front end (tests/frontend_ref.py) against the
oracle's os_corr / mask_init, and what the GPU tests rely on in their seeded frames: clip decisions
far from their bounds, planted values that land exactly where they are meant to.  The kernel variants
themselves are held against the restatements in tests/test_gpu_frontend_variants.py."""
import numpy as np
import pytest

import bbx_oracle as O
import frontend_ref as F
from blackbox_amd import settings, synth

TEL = 'ML1'
GAIN, SATLEVEL = settings.gain[TEL], settings.satlevel[TEL]


@pytest.fixture(scope='module')
def oracle_run():
    ys, xs, os_y, os_x = F.CAL_GEOM
    case = synth.make_case(ys, xs, 41, tel=TEL, os_y=os_y, os_x=os_x, n_stars=40, n_sat=4, n_cr=10)
    o = case['raw'].astype(np.float32)
    O.gain_corr(o, GAIN, ys, xs)
    data, header, aux = O.os_corr(o, ys, xs, tel=TEL, accum='f64')
    return case, data, header, aux


def test_calibrate_restatement_equals_os_corr(oracle_run):
    """fed os_corr's own vectors, the restatement gives os_corr's pixels bit for bit"""
    case, data, header, aux = oracle_run
    ys, xs = F.CAL_GEOM[:2]
    got, mask = F.calibrate(case['raw'], GAIN, aux['vfit'], aux['oscan'], np.full(16, np.inf), ys, xs)
    assert got.dtype == np.float32 and np.array_equal(got, data)
    assert not mask.any()


def test_calibrate_restatement_mask_equals_mask_init(oracle_run):
    """... and, with the bad-pixel mask, the first half of mask_init: the BPM, bad where a pixel is not finite and
    the BPM has nothing, saturated (the later steps of mask_init add bits 8 and 64 only)"""
    case, data, header, aux = oracle_run
    ys, xs = F.CAL_GEOM[:2]
    sat = np.float32(np.array(SATLEVEL) * np.array(GAIN) - np.array([header['BIASM%d' % (c + 1)] for c in range(16)]))
    o_mask, _ = O.mask_init(data.copy(), dict(header), case['bpm'], GAIN, SATLEVEL, ys, xs)
    got, mask = F.calibrate(case['raw'], GAIN, aux['vfit'], aux['oscan'], sat, ys, xs, bpm=case['bpm'])
    assert ((o_mask & 4) != 0).sum() > 20
    assert np.array_equal(mask, o_mask & ~np.uint8(8 | 64))
    assert np.array_equal(got, data)
    # non-finite pixels (here from the master bias): 0 and bad, unless the BPM already says something
    bias = np.zeros(data.shape, np.float32)
    bias[30, 500], bias[2, 900] = np.nan, np.inf
    assert case['bpm'][30, 500] == 0 and case['bpm'][2, 900] == 32
    got, mask = F.calibrate(case['raw'], GAIN, aux['vfit'], aux['oscan'], sat, ys, xs, bpm=case['bpm'], bias=bias)
    d2 = data - bias
    o_mask2, _ = O.mask_init(d2, dict(header), case['bpm'], GAIN, SATLEVEL, ys, xs)
    assert mask[30, 500] == 1 and mask[2, 900] == 32 and got[30, 500] == 0 and got[2, 900] == 0
    assert np.array_equal(mask, o_mask2 & ~np.uint8(8 | 64)) and np.array_equal(got, d2)


def test_row_mean_restatement_equals_os_corr(oracle_run):
    case, data, header, aux = oracle_run
    ys, xs = F.CAL_GEOM[:2]
    got = F.row_means(case['raw'], GAIN, ys, xs)
    assert np.array_equal(got, np.array(aux['mean_vos_col']))
    hos = F.hos_copy(case['raw'], GAIN, ys, xs)
    assert hos.shape == (16, 10, xs + F.CAL_GEOM[3]) and hos.dtype == np.float32


def test_read_noise_restatement_equals_os_corr(oracle_run):
    case, data, header, aux = oracle_run
    ys, xs = F.CAL_GEOM[:2]
    got = F.read_noise(case['raw'], GAIN, aux['vfit'], aux['dlevel'], ys, xs)
    assert np.array_equal(got, np.array([header['RDN%d' % (c + 1)] for c in range(16)]))


def test_satcol_restatement_equals_os_corr():
    """the brute-force counts give the mask_sat_row of the oracle's BlackGEM branch"""
    ys, xs, os_y, os_x = 96, 320, 20, 45
    tel = 'BG3'
    gain, satl = settings.gain[tel], settings.satlevel[tel]
    case = synth.make_case(ys, xs, 8, tel=tel, os_y=os_y, os_x=os_x, n_stars=30, n_sat=6, n_cr=0)
    raw = case['raw'].copy()
    raw[ys - 8:ys, 700:704] = 65535                           # columns saturated next to the overscan
    f = F.gain_f32(raw, gain, ys, xs)
    lim = {tel: (6, 40)}
    _, _, aux = O.os_corr(f, ys, xs, tel=tel, gain=gain, satlevel=satl, ypix_lim=lim)
    thr = np.float32(0.9 * np.array(satl) * np.array(gain))
    cnt = F.satcol_counts(raw, gain, aux['vfit'], thr, 6, 40, ys, xs)
    msr = (cnt[0] >= 3) | (cnt[1] >= 10)
    assert msr.sum() >= 4
    # os_corr does not return the mask; recompute it the way it does, from its own corrected strip
    dy, dx = ys + os_y, xs + os_x
    for c in range(16):
        iy, ix = divmod(c, 8)
        rows = slice(0, ys) if iy == 0 else slice(dy + os_y, 2 * dy)
        dsec = (F.gain_f32(raw, gain, ys, xs)[rows, ix * dx:ix * dx + xs].astype(np.float64)
                - aux['vfit'][c][(0 if iy == 0 else os_y):(ys if iy == 0 else dy), None]).astype(np.float32)
        r1, r2 = (slice(0, 6), slice(0, 40)) if iy else (slice(ys - 6, ys), slice(ys - 40, ys))
        want = (np.sum(dsec[r1] >= thr[c], axis=0) >= 3) | (np.sum(dsec[r2] >= thr[c], axis=0) >= 10)
        assert np.array_equal(msr[c], want), c


@pytest.mark.parametrize('os_x', sorted(F.STRIP_SEEDS))
def test_strip_frames_clip_far_from_the_bounds(os_x):
    """the row-mean tolerance of the GPU test (1e-12) must not hide a flipped clip decision: in the seeded
    frames no value in the running comes within 1e-9 (relative) of a bound it is compared with"""
    fr = F.strip_frame(os_x)
    assert os_x - 6 in (39, 176, 177, 256, 257, 512)
    for key in ('u16', 'f32nan'):
        assert F.row_clip_margin(fr[key], GAIN, F.YS, F.XS) > 1e-9, key
    means = F.row_means(fr['u16'], GAIN, F.YS, F.XS)
    c, r = fr['dead']
    assert np.isnan(means[c, r]) and np.isnan(means).sum() == 1
    assert int((~np.isfinite(fr['f32nan'])).sum()) == fr['n_infnan'] >= 16 * 4
    # the last strip column matters: without its planted offset the row means move by far more than the tolerance
    dx = F.XS + os_x
    alt = fr['u16'].copy()
    alt[:, dx - 2::dx] -= 8
    with np.errstate(invalid='ignore'):
        assert np.nanmedian(np.abs(F.row_means(alt, GAIN, F.YS, F.XS) / means - 1)) > 1e-7


@pytest.mark.parametrize('path', sorted(F.RDN_GEOMS))
def test_read_noise_frames_take_the_paths_they_claim(path):
    os_y, os_x = F.RDN_GEOMS[path]
    dy, vos_w = F.YS + os_y, os_x - 6
    assert ((dy * vos_w) % 4 == 0) == (path == 'float4')
    fr = F.rdn_frame(os_y, os_x)
    passes = F.read_noise_passes(fr['u16'], GAIN, fr['vfit'], fr['dlevel'], F.YS, F.XS)
    for c in F.RDN_FROZEN:
        assert passes[c] == 0, (c, passes)
    for c in F.RDN_FIVE:
        assert passes[c] == 5, (c, passes)
    std, n, n0 = F.read_noise(fr['u16'], GAIN, fr['vfit'], fr['dlevel'], F.YS, F.XS, with_n=True)
    assert np.all(np.isfinite(std)) and np.all(std > 2) and np.all(std < 40)
    # a raw zero is a residual of zero, and left out, only where vfit is zero; elsewhere it is a -13000 e- outlier
    for c in range(16):
        if c not in F.RDN_FROZEN + F.RDN_FIVE:
            assert (n0[c] < dy * vos_w) == (c % 3 == 1), c
            assert n[c] < n0[c]


def test_satcol_frame_lands_on_the_threshold():
    fr = F.satcol_frame()
    ys, xs = F.SATCOL_YS, F.XS
    f = F.gain_f32(fr['u16'], GAIN, ys, xs)
    dy, dx = ys + F.OS_Y, xs + 45
    assert len(np.unique(fr['vfit'][0])) > 10                 # a non-constant fit
    for (lst, want) in ((fr['exact'], 0), (fr['below'], -1)):
        for (c, k, x) in lst:
            iy, ix = divmod(c, 8)
            rl = (ys - 1 - k) if iy == 0 else (F.OS_Y + k)
            v = np.float32(np.float64(f[iy * dy + rl, ix * dx + x]) - fr['vfit'][c][rl])
            t = fr['thr'][c]
            assert v == (t if want == 0 else np.nextafter(t, np.float32(-np.inf))), (c, k, x)
    full = F.satcol_counts(fr['u16'], GAIN, fr['vfit'], fr['thr'], 64, 96, ys, xs)
    for c in range(8):                                        # lower and upper channels differ
        assert not np.array_equal(full[1, c] > 0, full[1, c + 8] > 0)
    # the counts change with the window: rows 10 and 70 are planted on both sides of rows2
    a = F.satcol_counts(fr['u16'], GAIN, fr['vfit'], fr['thr'], 3, 10, ys, xs)
    b = F.satcol_counts(fr['u16'], GAIN, fr['vfit'], fr['thr'], 3, 70, ys, xs)
    assert np.array_equal(a[0], b[0]) and (b[1] - a[1]).sum() > 16 and (full[1] - b[1]).sum() > 16
    assert a[1].max() == 10


def test_calib_case_plants():
    ys, xs = F.CAL_GEOM[:2]
    cs = F.calib_case()
    sat = np.float32(np.array(SATLEVEL) * np.array(GAIN) - cs['biasm'])
    d0, m0 = F.calibrate(cs['u16'], GAIN, cs['vfit'], cs['oscan'], sat, ys, xs)
    assert ((m0 & 4) != 0).sum() > 50 and (m0 & 4)[5, 7] and (m0 & 4)[-1, -1]
    bias = F.plant_bias_on_sat(cs['bias'], d0, sat, ys, xs)
    d1, m1 = F.calibrate(cs['u16'], GAIN, cs['vfit'], cs['oscan'], sat, ys, xs, bias=bias, flat=cs['flat'], bpm=cs['bpm'])
    for (y, x) in ((33, 650), (90, 1931)):
        assert m1[y, x] & 4 and not m0[y, x] & 4              # exactly on the threshold counts as saturated
    assert m1[30, 500] == 1 and m1[2, 900] == 32
    assert not np.isfinite(d1[20, 1000])                      # the zero of the flat: after the mask step, not flagged
    assert m1[20, 1000] == cs['bpm'][20, 1000]
    assert int((~np.isfinite(cs['f32nan'])).sum()) == 5


@pytest.mark.parametrize('kind', ['round', 'blocks'])
def test_blob_frames(kind):
    ys, xs, os_y, os_x = F.CAL_GEOM
    case, rawf = F.blob_frame(kind)
    sat = (rawf == 65535)
    dy, dx = ys + os_y, xs + os_x
    red = np.concatenate([np.concatenate([sat[iy * dy + (os_y if iy else 0):iy * dy + (os_y if iy else 0) + ys, ix * dx:ix * dx + xs]
                                          for ix in range(8)], axis=1) for iy in range(2)], axis=0)
    assert 0.01 < red.mean() < 0.125                          # > 1 % and below the queue's capacity (N / 8 + 4096)
    if kind == 'blocks':
        # whole 4-pixel groups in whole 8-row strips: a lane of the vector kernel queues up to 32 pixels at once
        groups = red.reshape(2 * ys // 8, 8, 8 * xs // 4, 4).sum(axis=(1, 3))
        assert (groups == 32).sum() > 50


def test_dead_vertical_overscan_host_fallback():
    """a channel whose vertical overscan reads zero: the oracle (as the reference, blackbox.py:6480-6490) takes row means
    of 0.0 -> BIASM 0.0, RDN 0.0, VFITOK True.  The device marks such rows with NaN; overscan.dead_vos_rows restores
    the zeros, and the host fit then gives the oracle's vectors"""
    from blackbox_amd import overscan
    c0 = F.DEAD_CHAN
    case = F.e2e_case(180, dead=True)
    oh = F.oracle_chain(case, 'f64')[3]
    assert oh['BIASM%d' % (c0 + 1)] == 0.0 and oh['RDN%d' % (c0 + 1)] == 0.0 and oh['VFITOK%d' % (c0 + 1)] is True
    o = case['raw'].astype(np.float32)
    O.gain_corr(o, GAIN, F.YS, F.XS)
    _, _, aux = O.os_corr(o, F.YS, F.XS, tel=TEL, accum='bn32')
    means = F.row_means(case['raw'], GAIN, F.YS, F.XS)          # what the row kernel delivers
    assert np.isnan(means[c0]).all() and np.isfinite(np.delete(means, c0, axis=0)).all()
    m0 = means[0]
    assert overscan.dead_vos_rows(m0) is m0
    part = means[c0].copy(); part[3] = 1.0
    assert overscan.dead_vos_rows(part) is part                 # a strip with anything valid in it is left alone
    m = overscan.dead_vos_rows(means[c0])
    assert np.array_equal(m, np.zeros(F.YS + F.OS_Y))
    hos = F.hos_copy(case['raw'], GAIN, F.YS, F.XS)
    for use_c in (True, False):
        overscan.USE_C_DRIVER = use_c
        try:
            r = overscan.channel_solve((c0, m, hos[c0], F.YS, F.XS, 3, TEL, 2000, 'f32seq'))
        finally:
            overscan.USE_C_DRIVER = True
        assert r['ok'] is True and r['level'] == 0.0 and not r['fit'].any()
        assert np.array_equal(r['oscan'], aux['oscan'][c0])
        assert r['dlevel'] == pytest.approx(aux['dlevel'][c0], rel=1e-6)
