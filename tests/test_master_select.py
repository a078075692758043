"""Master frames, host side (blackbox_amd/masters.py; reference create_masters / master_prep / get_nearest_master,
blackbox.py:617-782, 4625-5412): which reduced frames make a master, when none is made, which existing master is
used instead, and how --master_date is read.  Trees of small FITS files with controlled headers; no GPU."""
import importlib.util
import os
import time

import numpy as np
import pytest

from blackbox_amd import fitsio, masters as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame(red, tel, imgtype, date_obs, filt=None, eve=None, **keys):
    """a reduced calibration frame <red>/<yyyy/mm/dd of the evening>/<imgtype>/<tel>_<yyyymmdd>_<hhmmss>[_<filt>].fits
    taken at [date_obs]; the evening is the UT date of date_obs - 12 h unless given"""
    mjd = M.isot2mjd(date_obs)
    eve = eve or M._day_path(mjd - 0.5)
    d = os.path.join(red, eve, imgtype)
    os.makedirs(d, exist_ok=True)
    stamp = date_obs.replace('-', '').replace(':', '').replace('T', '_')
    name = os.path.join(d, '{}_{}{}.fits'.format(tel, stamp, '_' + filt if filt else ''))
    h = {'IMAGETYP': imgtype, 'DATE-OBS': date_obs, 'MJD-OBS': mjd, 'QC-FLAG': 'green'}
    if filt:
        h['FILTER'] = filt
    h.update(keys)
    fitsio.write_image(name, np.zeros((4, 8), np.float32), h)
    return name


def master_file(path, flag='green'):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    fitsio.write_image(path, np.ones((4, 8), np.float32), {'QC-FLAG': flag})
    return path


def names(files):
    return [os.path.basename(f) for f in files]


# ---- dates -------------------------------------------------------------------------------------------------------
def test_dates():
    assert M.date2mjd('20240105', '12:00') == 60314.5
    assert M.date2mjd('2024-01-05', '235900') == pytest.approx(60314 + 1439 / 1440., abs=1e-12)
    assert M.isot2mjd('2019-07-01T12:00:00') == 58665.5
    assert M.isot2mjd('2024-01-06T03:00:30.5') == pytest.approx(60315.125 + 30.5 / 86400, abs=1e-12)
    assert [M.delta_one_month('20240105', k) for k in (-1, 0, 1)] == ['2023/12/', '2024/01/', '2024/02/']
    assert M.delta_one_month('20241231', 1) == '2025/01/' and M.delta_one_month('20240301', -1) == '2024/02/'
    assert 3600 * M.haversine(10.0, 20.0, 10.0, 20.001) == pytest.approx(3.6, rel=1e-9)


# ---- selection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('imgtype,window', [('bias', 3), ('flat', 7)])
def test_window_edges(tmp_path, imgtype, window):
    red = str(tmp_path)
    filt = 'q' if imgtype == 'flat' else None
    inside, outside = [], []
    for n in range(-window - 1, window + 2):
        day = M._day_path(M.date2mjd('20240105', '12:00') + n)
        f = frame(red, 'ML1', imgtype, '{}T03:00:00'.format(M._day_path(M.date2mjd('20240105', '12:00') + n + 1).replace('/', '-')),
                  filt=filt, eve=day)
        (outside if abs(n) > window else inside).append(f)
    got = M.list_cal_files(red, 'ML1', imgtype, '20240105', filt)
    assert got == sorted(inside)
    assert not set(got) & set(outside)


def test_name_rules_and_fz_twin(tmp_path):
    red = str(tmp_path)
    a = frame(red, 'ML1', 'flat', '2024-01-06T03:00:00', filt='q')
    frame(red, 'ML1', 'flat', '2024-01-06T03:01:00', filt='r')                       # another filter
    b = frame(red, 'ML1', 'flat', '2024-01-06T03:02:00', filt='q')
    with open(b + '.fz', 'wb') as f:                                                # the same frame, compressed
        f.write(open(b, 'rb').read())
    d = os.path.dirname(a)
    open(os.path.join(d, 'BG2_20240106_030300_q.fits'), 'wb').write(open(a, 'rb').read())    # other telescope
    open(os.path.join(d, 'ML1_20240106_030000_q.log'), 'w').write('log')             # no '.fits'
    assert names(M.list_cal_files(red, 'ML1', 'flat', '20240105', 'q')) == [os.path.basename(a), os.path.basename(b) + '.fz']


def test_red_frames_dropped(tmp_path):
    red = str(tmp_path)
    fs = [frame(red, 'ML1', 'bias', '2024-01-06T0%d:00:00' % k) for k in range(6)]
    frame(red, 'ML1', 'bias', '2024-01-05T23:30:00', **{'QC-FLAG': 'red'})
    sel = M.select_frames(red, 'ML1', 'bias', '20240105')
    assert sel['nfound'] == 7 and sel['nkept'] == 6 and sel['skip'] is None
    assert sorted(sel['files']) == sorted(fs)


def test_ml1_evening_rule_2019_2020(tmp_path):
    red = str(tmp_path)
    morning = [frame(red, 'ML1', 'bias', '2019-10-11T0%d:00:00' % k) for k in range(5)]
    evening = [frame(red, 'ML1', 'bias', '2019-10-10T1%d:00:00' % k, eve='2019/10/10') for k in range(7, 9)]
    sel = M.select_frames(red, 'ML1', 'bias', '20191010')
    assert sorted(sel['files']) == sorted(morning) and not set(evening) & set(sel['files'])
    # outside the period, and for BlackGEM, evening frames count
    red2 = str(tmp_path / 'later')
    ev2 = [frame(red2, 'ML1', 'bias', '2020-03-10T1%d:00:00' % k, eve='2020/03/10') for k in range(5)]
    assert sorted(M.select_frames(red2, 'ML1', 'bias', '20200310')['files']) == sorted(ev2)
    red3 = str(tmp_path / 'bg')
    ev3 = [frame(red3, 'BG2', 'bias', '2019-10-10T1%d:00:00' % k, eve='2019/10/10') for k in range(5)]
    assert sorted(M.select_frames(red3, 'BG2', 'bias', '20191010')['files']) == sorted(ev3)


@pytest.mark.parametrize('tel', ['BG2', 'ML1'])
def test_evening_flats(tmp_path, tel):
    red = str(tmp_path)
    morning = [frame(red, tel, 'flat', '2024-01-06T0%d:30:00' % k, filt='q') for k in range(3, 8)]
    evening = [frame(red, tel, 'flat', '2024-01-05T1%d:00:00' % k, filt='q', eve='2024/01/05') for k in range(7, 9)]
    after_midnight = [frame(red, tel, 'flat', '2024-01-06T00:30:00', filt='q')]       # MJD fraction 0.02
    sel = M.select_frames(red, tel, 'flat', '20240105', 'q')
    if tel == 'BG2':                   # flat_reject_eve: morning flats only
        assert sorted(sel['files']) == sorted(morning)
    else:
        assert sorted(sel['files']) == sorted(morning + evening + after_midnight)


def test_ncal_max_nearest_midnight(tmp_path):
    red = str(tmp_path)
    mid = M.date2mjd('20240105', '23:59')
    fs, delta = [], []
    for k in range(25):                 # every 37 min from 16:00 on the evening to the morning after
        mjd = M.date2mjd('20240105', '16:00') + k * 37 / 1440.
        dt = M._MJD0 + __import__('datetime').timedelta(days=mjd)
        fs.append(frame(red, 'ML1', 'bias', dt.strftime('%Y-%m-%dT%H:%M:%S'), eve='2024/01/05'))
        delta.append(abs(M.isot2mjd(dt.strftime('%Y-%m-%dT%H:%M:%S')) - mid))
    sel = M.select_frames(red, 'ML1', 'bias', '20240105')
    want = [fs[i] for i in np.argsort(delta, kind='stable')[:20]]
    assert sel['files'] == want and sel['nkept'] == 25
    assert np.all(np.diff(np.abs(sel['mjd_obs'] - mid)) >= 0)


def test_four_frames_no_master(tmp_path):
    red, mdir = str(tmp_path / 'red'), str(tmp_path / 'masters')
    for k in range(4):
        frame(red, 'ML1', 'bias', '2024-01-06T0%d:00:00' % k)
    assert M.select_frames(red, 'ML1', 'bias', '20240105')['skip'] == 'few'
    fm = os.path.join(mdir, '2024/01/05/bias/ML1_bias_20240105.fits')
    assert M.master_prep(fm, (4, 8), True, pick_alt=False, tel='ML1', red_dir=red, master_dir=mdir) is None
    assert not os.path.exists(fm)


def test_all_old_no_master(tmp_path):
    red, mdir = str(tmp_path / 'red'), str(tmp_path / 'masters')
    for k in range(6):                 # evening 2024-01-02 (within the window), nothing later
        frame(red, 'ML1', 'bias', '2024-01-03T0%d:00:00' % k)
    sel = M.select_frames(red, 'ML1', 'bias', '20240105')
    assert sel['skip'] == 'old' and len(sel['files']) == 6
    fm = os.path.join(mdir, '2024/01/05/bias/ML1_bias_20240105.fits')
    assert M.master_prep(fm, (4, 8), True, pick_alt=True, tel='ML1', red_dir=red, master_dir=mdir) is None
    # one frame of the night after: not all old any more
    frame(red, 'ML1', 'bias', '2024-01-07T03:00:00')
    assert M.select_frames(red, 'ML1', 'bias', '20240105')['skip'] is None


def test_existing_green_master_kept(tmp_path):
    red, mdir = str(tmp_path / 'red'), str(tmp_path / 'masters')
    for k in range(6):
        frame(red, 'ML1', 'bias', '2024-01-06T0%d:00:00' % k)
    fm = os.path.join(mdir, '2024/01/05/bias/ML1_bias_20240105.fits')
    for existing in (fm, fm + '.fz'):
        master_file(existing)
        os.utime(existing, (1e9, 1e9))
        assert M.master_prep(fm, (4, 8), True, tel='ML1', red_dir=red, master_dir=mdir) == existing
        assert os.path.getmtime(existing) == 1e9
        os.remove(existing)


def test_existing_red_master_rebuilt(tmp_path, monkeypatch):
    red, mdir = str(tmp_path / 'red'), str(tmp_path / 'masters')
    fs = [frame(red, 'ML1', 'bias', '2024-01-06T0%d:00:00' % k) for k in range(6)]
    fm = os.path.join(mdir, '2024/01/05/bias/ML1_bias_20240105.fits')
    master_file(fm + '.fz', flag='red')
    seen = {}

    def fake_build(ctx, sel, imgtype, tel, data_shape, **kw):       # the device part, stood in for
        import torch
        seen['files'] = sel['files']
        return torch.full(data_shape, 2.0), {'QC-FLAG': ('green', '')}
    monkeypatch.setattr(M, 'build_master', fake_build)
    got = M.master_prep(fm, (4, 8), True, tel='ML1', red_dir=red, master_dir=mdir, ctx=object())
    assert got == fm and sorted(seen['files']) == sorted(fs)
    assert not os.path.exists(fm + '.fz')                           # the red master it replaces
    data, h = fitsio.read_image(fm, get_header=True)
    assert np.all(data == 2.0) and M._hv(h, 'QC-FLAG') == 'green' and 'DATEFILE' in h
    assert not [n for n in os.listdir(os.path.dirname(fm)) if 'tmp' in n]


def test_get_nearest_master(tmp_path):
    mdir = str(tmp_path)
    fm = os.path.join(mdir, '2024/02/01/bias/ML1_bias_20240201.fits')
    p = lambda d, ext='.fits.fz', flag='green': master_file(                                      # noqa: E731
        os.path.join(mdir, d[0:4], d[4:6], d[6:8], 'bias', 'ML1_bias_{}{}'.format(d, ext)), flag)
    near = [p('20240129'), p('20240205'), p('20240130', flag='red'), p('20240202', ext='.fits')]
    yest = p('20240131', ext='.fits')
    assert M.get_nearest_master('20240201', 'bias', fm, master_dir=mdir, tel='ML1') == yest     # yesterday first
    os.remove(yest)
    p('20240131', flag='red')
    # yesterday red, 20240130 red, 20240202 not .fits.fz: the nearest acceptable one is in the previous month
    assert M.get_nearest_master('20240201', 'bias', fm, master_dir=mdir, tel='ML1') == near[0]
    # master_prep without frames falls back to it with pick_alt, and returns None without
    red = str(tmp_path / 'red')
    assert M.master_prep(fm, (4, 8), True, pick_alt=True, tel='ML1', red_dir=red, master_dir=mdir) == near[0]
    assert M.master_prep(fm, (4, 8), True, pick_alt=False, tel='ML1', red_dir=red, master_dir=mdir) is None
    assert M.master_prep(fm, (4, 8), False, pick_alt=False, tel='ML1', red_dir=red, master_dir=mdir) == near[0]
    # flats: the filter is part of the name
    ff = os.path.join(mdir, '2024/02/01/flat/ML1_flat_20240201_q.fits')
    master_file(os.path.join(mdir, '2024/01/20/flat/ML1_flat_20240120_r.fits.fz'))
    q = master_file(os.path.join(mdir, '2024/03/10/flat/ML1_flat_20240310_q.fits.fz'))
    assert M.get_nearest_master('20240201', 'flat', ff, filt='q', master_dir=mdir, tel='ML1') == q
    assert M.get_nearest_master('20240501', 'bias', fm.replace('0201', '0501').replace('02/01', '05/01'),
                                master_dir=mdir, tel='ML1') is None


def test_master_date_forms(tmp_path):
    assert M.master_dates('20240105') == [('20240105', None)]
    lst = tmp_path / 'dates.txt'
    lst.write_text('2024-01-05 qr\n\n20240106\n')
    assert M.master_dates(str(lst)) == [('20240105', 'qr'), ('20240106', None)]
    got = M.list_masters(str(lst), '/m', 'ML1', imgtypes='bias,flat')
    assert got == ['/m/2024/01/05/bias/ML1_bias_20240105.fits', '/m/2024/01/05/flat/ML1_flat_20240105_q.fits',
                   '/m/2024/01/05/flat/ML1_flat_20240105_r.fits', '/m/2024/01/06/bias/ML1_bias_20240106.fits'] + \
        ['/m/2024/01/06/flat/ML1_flat_20240106_{}.fits'.format(f) for f in 'ugqriz']
    assert M.list_masters('20240105', '/m', 'BG2', filters='g,r', imgtypes='flat') == \
        ['/m/2024/01/05/flat/BG2_flat_20240105_g.fits', '/m/2024/01/05/flat/BG2_flat_20240105_r.fits']
    assert len(M.list_masters('20240105', '/m', 'ML1')) == 2 + 6
    for bad in ('2024', '202401', '20241305', 'tonight'):
        with pytest.raises(ValueError):
            M.master_dates(bad)


def _cli():
    spec = importlib.util.spec_from_file_location('bbx_cli_masters', os.path.join(ROOT, 'blackbox.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_refusals(tmp_path):
    cli = _cli()
    base = ['--telescope', 'ML1', '--red_dir', str(tmp_path), '--master_dir', str(tmp_path / 'm')]
    for argv in (base + ['--master_date', '2024'],
                 ['--telescope', 'ML1', '--master_date', '20240105', '--red_dir', str(tmp_path)],
                 ['--telescope', 'ML1', '--master_date', '20240105', '--master_dir', str(tmp_path)],
                 base + ['--master_date', '20240105', '--flat_norm_sec', '32:96']):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    assert cli.section('32:96,400:800') == (slice(32, 96), slice(400, 800))


@pytest.mark.parametrize('ra,dec,want', [
    ([150.0] * 6, [2.0] * 6, (0, 0, False)),                                      # not dithered
    ([150.0, 150.01, 150.02, 150.03, 150.04, 150.05], [2.0] * 6, None),           # every flat offset ~36"
    ([150.0, 150.0, 150.0, 150.01, 150.01, 150.01], [2.0] * 6, (2, None, False)),  # two offsets of six
    ([], [], (0, 0, False)),                                                      # no RA / DEC in the headers
])
def test_dither_keywords(ra, dec, want):
    h = M.dither_keywords({}, ra, dec, 6)
    n, mean, dith = (M._hv(h, k) for k in ('N-OFFSET', 'OFF-MEAN', 'FLATDITH'))
    off = 3600 * M.haversine(ra, dec, np.roll(ra, 1), np.roll(dec, 1)) if ra else np.zeros(0)
    if want is None:
        assert n == 6 and dith is True
        assert mean == pytest.approx(np.mean(off), rel=1e-12)
        assert off[1] == pytest.approx(36.0 * np.cos(np.radians(2.0)), rel=1e-4)
    else:
        assert n == want[0] and dith is want[2]
        if want[1] is not None:
            assert mean == want[1]
        else:
            assert mean == pytest.approx(np.mean(off[off >= 5]), rel=1e-12)
    assert list(h) == ['N-OFFSET', 'OFF-MEAN', 'FLATDITH']


def test_lock_serialises(tmp_path):
    """two master_prep calls for the same master: the second waits for the first's lock and finds its file"""
    import threading
    fm = str(tmp_path / '2024/01/05/bias/ML1_bias_20240105.fits')
    order = []
    with M._Lock(fm):
        t = threading.Thread(target=lambda: order.append(M.master_prep(fm, (4, 8), True, tel='ML1', red_dir=str(tmp_path),
                                                                       master_dir=str(tmp_path))))
        t.start()
        time.sleep(0.3)
        assert not order                                  # waiting on the lock
        master_file(fm)
    t.join(10)
    assert order == [fm]
