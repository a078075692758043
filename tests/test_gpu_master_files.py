"""GPU: master frames from files (masters.create_masters / master_prep, blackbox.py --master_date; reference
blackbox.py:617-782, 4625-5247).  The reduced frames of the round-2 fixture (tests/golden/pins_r02.*, made by the
reference's own master_prep on files in this layout, oracle/gen_golden_r02.py) are laid out on disk; the masters read
back from the written files carry the reference's pixels and header values.  Also: tile-compressed inputs, a flat
without its bad-pixel mask, a frame of the wrong shape, the command line, reductions with .fits.fz masters and one
full-size master."""
import glob
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import bbx_oracle as O                                          # noqa: E402
from blackbox_amd import fitsio, fpack as P, masters as M, synth  # noqa: E402
from blackbox_amd import reduce as R                            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'pins_r02.json')))
YS, XS = synth.MASTER_GEOM
hv = R.hval


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def layout(root, ctx=None, frames_of=None):
    """the fixture's inputs as gen_golden_r02.py laid them out: <root>/red/2024/01/05/{flat,bias}/
    ML1_20240106_03{k:02d}00[_q].fits (with [ctx]: device-fpacked .fits.fz) and <root>/bpm_q.fits -> red dir"""
    red = os.path.join(root, 'red')
    fitsio.write_image(os.path.join(root, 'bpm_q.fits'), synth.master_bpm())
    for imgtype in ('flat', 'bias'):
        d = os.path.join(red, '2024', '01', '05', imgtype)
        os.makedirs(d, exist_ok=True)
        frames, medsec = (frames_of or synth.master_frames)(imgtype)
        for k, img in enumerate(frames):
            h = {'IMAGETYP': imgtype, 'FILTER': 'q', 'QC-FLAG': 'green', 'DATE-OBS': '2024-01-06T03:0%d:00' % k}
            h['MJD-OBS'] = M.isot2mjd(h['DATE-OBS'])
            if imgtype == 'flat':
                h['MEDSEC'] = float(medsec[k])
            name = os.path.join(d, 'ML1_20240106_03{:02d}00{}.fits'.format(k, '_q' if imgtype == 'flat' else ''))
            if ctx is None:
                fitsio.write_image(name, img, h)
            else:
                P.fpack_image(ctx, name, torch.from_numpy(img).to(ctx.device), h, quant=16)
    return red


def run(ctx, root, mdir, imgtypes='bias,flat', bpm=True, **kw):
    return M.create_masters('20240105', os.path.join(root, 'red'), mdir, tel='ML1', ctx=ctx, imgtypes=imgtypes,
                            filters='q', bpm=os.path.join(root, 'bpm.fits') if bpm else None,
                            flat_norm_sec=synth.MASTER_NORM_SEC, ysize_chan=YS, xsize_chan=XS, **kw)


def test_masters_from_files_match_reference(tmp_path):
    ctx = R.Context(0)
    layout(str(tmp_path))
    res = run(ctx, str(tmp_path), str(tmp_path / 'masters'))
    assert [r[2] for r in res] == [None, None]
    mb, mf = res[0][1], res[1][1]
    assert mb == str(tmp_path / 'masters/2024/01/05/bias/ML1_bias_20240105.fits')
    assert mf == str(tmp_path / 'masters/2024/01/05/flat/ML1_flat_20240105_q.fits')

    data, h = fitsio.read_image(mf, get_header=True)
    want = META['master_flat']['header']
    assert data.dtype == np.float32 and sha(data) == META['master_flat']['sha']      # every pixel of the reference's
    assert hv(h, 'NFLAT') == want['NFLAT'] == 6 and hv(h, 'FLAT-WIN') == 7
    for c in range(16):
        assert hv(h, 'GAINCF%d' % (c + 1)) == pytest.approx(want['GAINCF%d' % (c + 1)], rel=2e-15), c
    assert hv(h, 'MFMEDSEC') == want['MFMEDSEC']
    assert hv(h, 'MFSTDSEC') == pytest.approx(want['MFSTDSEC'], rel=1e-6)
    frames, medsec = synth.master_frames('flat')
    unfixed = O.master_median(np.stack(frames), 'flat', medsec=medsec)               # MFMED / MFSTD: before the edge fix
    _, med, std, _ = O.sigma_clipped_stats_median(unfixed)
    assert hv(h, 'MFMED') == pytest.approx(med, abs=1e-4) and hv(h, 'MFSTD') == pytest.approx(std, abs=1e-4)
    assert hv(h, 'STATSEC') == '[33:97,401:801]'
    assert (hv(h, 'N-OFFSET'), hv(h, 'OFF-MEAN'), hv(h, 'FLATDITH')) == (0, 0, False)
    assert [hv(h, 'FLAT%d' % (k + 1)) for k in range(6)] == ['ML1_20240106_03%02d00_q' % k for k in range(6)]
    keys = list(h)
    order = ['IMAGETYP', 'DATE-OBS', 'FILTER', 'MJD-OBS', 'FLAT1', 'FLAT6', 'NFLAT', 'FLAT-WIN', 'STATSEC', 'MFMEDSEC',
             'MFSTDSEC', 'MFMED', 'MFSTD', 'N-OFFSET', 'OFF-MEAN', 'FLATDITH', 'GAINCF1', 'GAINCF16', 'QC-FLAG', 'DATEFILE']
    assert [keys.index(k) for k in order] == sorted(keys.index(k) for k in order)
    assert hv(h, 'DATE-OBS') == '2024-01-06T03:00:00'

    data, h = fitsio.read_image(mb, get_header=True)
    want = META['master_bias']['header']
    assert sha(data) == META['master_bias']['sha']
    assert hv(h, 'NBIAS') == want['NBIAS'] == 6 and hv(h, 'BIAS-WIN') == 3
    for k in ['MBMEAN', 'MBRDN'] + ['MBIASM%d' % (c + 1) for c in range(16)] + ['MBRDN%d' % (c + 1) for c in range(16)]:
        assert hv(h, k) == pytest.approx(want[k], rel=1e-4, abs=1e-4), k
    assert [hv(h, 'BIAS%d' % (k + 1)) for k in range(6)] == ['ML1_20240106_03%02d00' % k for k in range(6)]
    ctx.close()


def test_fz_inputs_bit_identical(tmp_path):
    ctx = R.Context(0)
    red = layout(str(tmp_path), ctx=ctx)
    assert not glob.glob(os.path.join(red, '*/*/*/*/*.fits'))                        # only the compressed frames
    res = run(ctx, str(tmp_path), str(tmp_path / 'masters'))
    assert [r[2] for r in res] == [None, None]
    bpm = torch.from_numpy(synth.master_bpm()).to(ctx.device)
    for (_, path, _), imgtype in zip(res, ('bias', 'flat')):
        files = sorted(glob.glob(os.path.join(red, '2024/01/05', imgtype, '*.fits.fz')))
        dec = [P.funpack_image(ctx, f) for f in files]
        medsec = [hv(h, 'MEDSEC') for _, h in dec] if imgtype == 'flat' else None
        want = M.master_median(ctx, [t for t, _ in dec], imgtype, medsec=medsec, bpm=bpm if imgtype == 'flat' else None)
        data = fitsio.read_image(path)
        assert np.array_equal(data, want.cpu().numpy()), imgtype
        assert hv(fitsio.read_image(path, get_header=True)[1], 'N' + imgtype.upper()) == 6
    ctx.close()


def test_flat_without_bpm_keeps_nonpositive(tmp_path):
    def frames_of(imgtype):
        frames, medsec = synth.master_frames(imgtype)
        if imgtype == 'flat':
            for f in frames:
                f[10, 30] = -5.0                     # non-positive in every frame: non-positive in the master
        return frames, medsec
    ctx = R.Context(0)
    layout(str(tmp_path), frames_of=frames_of)
    (_, path, err), = run(ctx, str(tmp_path), str(tmp_path / 'masters'), imgtypes='flat', bpm=False)
    assert err is None
    frames, medsec = frames_of('flat')
    want = O.master_median(np.stack(frames), 'flat', medsec=medsec)                 # no fix without the mask
    data = fitsio.read_image(path)
    assert np.array_equal(data, want) and data[10, 30] < 0 and data[0, 5] != 1.0
    # with the per-filter mask (found next to --bpm as bpm_q.fits) the same pixels become 1
    (_, path, err), = run(ctx, str(tmp_path), str(tmp_path / 'masters_bpm'), imgtypes='flat')
    data = fitsio.read_image(path)
    assert err is None and data[10, 30] == 1.0 and data[0, 5] == 1.0
    ctx.close()


def test_wrong_shape_fails_that_master_only(tmp_path):
    ctx = R.Context(0)
    red = layout(str(tmp_path))
    bad = os.path.join(red, '2024/01/05/bias/ML1_20240106_030300.fits')
    img, h = fitsio.read_image(bad, get_header=True)
    fitsio.write_image(bad, img[:, :-8], h)
    res = run(ctx, str(tmp_path), str(tmp_path / 'masters'))
    assert res[0][1] is None and 'ML1_20240106_030300' in res[0][2]
    assert res[1][2] is None and sha(fitsio.read_image(res[1][1])) == META['master_flat']['sha']
    d = str(tmp_path / 'masters/2024/01/05/bias')
    assert sorted(os.listdir(d)) == ['ML1_bias_20240105.fits.lock']                  # no master, no half-written file
    ctx.close()


def load_cli():
    spec = importlib.util.spec_from_file_location('bbx_cli_m', os.path.join(ROOT, 'blackbox.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_master_date(tmp_path, capsys):
    cli = load_cli()
    red = layout(str(tmp_path))
    argv = lambda mdir: ['--telescope', 'ML1', '--master_date', '20240105', '--red_dir', red, '--master_dir', mdir,  # noqa: E731
                         '--imgtypes', 'bias,flat', '--filters', 'q', '--bpm', str(tmp_path / 'bpm.fits'),
                         '--ysize_chan', str(YS), '--xsize_chan', str(XS), '--flat_norm_sec', '32:96,400:800']
    M_ = str(tmp_path / 'M')
    out = cli.main(argv(M_))
    mb = os.path.join(M_, '2024/01/05/bias/ML1_bias_20240105.fits')
    mf = os.path.join(M_, '2024/01/05/flat/ML1_flat_20240105_q.fits')
    assert out == [mb, mf] and cli._STATE['exit_status'] == 0
    assert capsys.readouterr().out.split() == [mb, mf]
    assert sha(fitsio.read_image(mb)) == META['master_bias']['sha']
    assert sha(fitsio.read_image(mf)) == META['master_flat']['sha']
    stamp = [(os.stat(f).st_mtime_ns, open(f, 'rb').read()) for f in (mb, mf)]
    assert cli.main(argv(M_)) == [mb, mf]                                              # there already: untouched
    assert [(os.stat(f).st_mtime_ns, open(f, 'rb').read()) for f in (mb, mf)] == stamp
    # compressed masters
    Mz = str(tmp_path / 'Mz')
    outz = cli.main(argv(Mz) + ['--fpack', 'True'])
    assert outz == [mb.replace(M_, Mz) + '.fz', mf.replace(M_, Mz) + '.fz'] and cli._STATE['exit_status'] == 0
    assert not os.path.exists(mb.replace(M_, Mz))
    ctx = R.Context(0)
    for f, plain in zip(outz, (mb, mf)):
        t, h = P.funpack_image(ctx, f)
        ref = fitsio.read_image(plain)
        assert hv(h, 'NBIAS' if '_bias_' in f else 'NFLAT') == 6
        assert np.abs(t.cpu().numpy() - ref).max() <= 0.2 * np.std(ref)              # quantised: q = 16
    ctx.close()
    # a master that fails (a truncated frame) makes the exit status non-zero; the other is made
    bad = os.path.join(red, '2024/01/05/bias/ML1_20240106_030200.fits')
    with open(bad, 'r+b') as f:
        f.truncate(os.path.getsize(bad) // 2)
    Mb = str(tmp_path / 'Mb')
    outb = cli.main(argv(Mb))
    assert outb[0] is None and outb[1] == mf.replace(M_, Mb) and cli._STATE['exit_status'] == 1


def _without_card(path, key):
    """the file's bytes with the header card [key] blanked"""
    b = bytearray(open(path, 'rb').read())
    for i in range(0, len(b), 80):
        if bytes(b[i:i + 8]).rstrip() == key.encode():
            b[i:i + 80] = b' ' * 80
        if bytes(b[i:i + 8]).rstrip() == b'END':
            break
    return bytes(b)


def test_fz_masters_applied(tmp_path):
    """a raw frame reduced with .fits.fz masters and with the plain files they decode to (tmp_path: no "_red" in it)"""
    cli = load_cli()
    ys, xs, tel = 64, 330, 'ML1'
    case = synth.make_case(ys, xs, 37, tel=tel, os_y=20, os_x=45, n_stars=30, n_sat=1, n_cr=20, with_bias=True)
    raw = str(tmp_path / 'ML1_raw.fits')
    fitsio.write_image(raw, case['raw'], {'DATE-OBS': '2024-01-02T03:04:05', 'EXPTIME': 60.0, 'IMAGETYP': 'object',
                                          'FILTER': 'q'})
    z, p = tmp_path / 'z', tmp_path / 'p'
    os.makedirs(str(z))
    os.makedirs(str(p))
    ctx = R.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)     # noqa: E731
    P.fpack_image(ctx, str(z / 'X.fits'), dev(case['flat']), {'IMAGETYP': 'flat'}, quant=16)
    P.fpack_image(ctx, str(z / 'Y.fits'), dev(case['bias'] + 5.0), {'IMAGETYP': 'bias'}, quant=16)
    P.fpack_image(ctx, str(z / 'bpm.fits'), dev(case['bpm']), {})
    for n, dtype in (('X', np.float32), ('Y', np.float32), ('bpm', np.uint8)):     # the plain files they decode to
        t, _ = P.funpack_image(ctx, str(z / (n + '.fits.fz')))
        fitsio.write_image(str(p / (n + '.fits')), t.cpu().numpy())
        assert torch.equal(R.image_to_device(ctx, str(z / (n + '.fits.fz')), dtype),
                           R.image_to_device(ctx, str(p / (n + '.fits')), dtype))
    assert np.array_equal(fitsio.read_image(str(p / 'bpm.fits')), case['bpm'])
    ctx.close()
    common = ['--telescope', tel, '--image', raw, '--ysize_chan', str(ys), '--xsize_chan', str(xs)]
    for d, ext in ((z, '.fits.fz'), (p, '.fits')):
        out = cli.main(common + ['--red_dir', str(d / 'red'), '--mflat', str(d / ('X' + ext)),
                                 '--mbias', str(d / ('Y' + ext)), '--bpm', str(d / ('bpm' + ext))])
        assert out == [str(d / 'red' / 'ML1_20240102_030405_red.fits')]
    red_z, red_p = (str(d / 'red' / 'ML1_20240102_030405_red.fits') for d in (z, p))
    h = fitsio.read_image(red_z, get_header=True)[1]
    assert hv(h, 'MFLAT-P') is True and hv(h, 'MFLAT-F') == 'X'
    # the same bytes; only the start time of the run may differ
    assert _without_card(red_z, 'BB-START') == _without_card(red_p, 'BB-START')
    assert open(red_z.replace('_red', '_mask'), 'rb').read() == open(red_p.replace('_red', '_mask'), 'rb').read()


def test_full_size_bias_master(tmp_path):
    """five 10560 x 10560 bias frames as .fits.fz -> the master, bit-identical to np.median of the decoded frames"""
    ctx = R.Context(0)
    red = str(tmp_path / 'red')
    d = os.path.join(red, '2024/01/05/bias')
    os.makedirs(d)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(3)
    for k in range(5):
        img = (3.0 * torch.randn((10560, 10560), generator=g, device=ctx.device) + 0.5 * k).contiguous()
        img[::97, ::89] = 0.0
        h = {'IMAGETYP': 'bias', 'QC-FLAG': 'green', 'DATE-OBS': '2024-01-06T03:0%d:00' % k}
        h['MJD-OBS'] = M.isot2mjd(h['DATE-OBS'])
        P.fpack_image(ctx, os.path.join(d, 'ML1_20240106_03%02d00.fits' % k), img, h, quant=16)
        del img
    timing = {}
    (_, path, err), = M.create_masters('20240105', red, str(tmp_path / 'M'), tel='ML1', ctx=ctx, imgtypes='bias',
                                       timing=timing)
    assert err is None and path.endswith('ML1_bias_20240105.fits')
    cube = np.stack([P.funpack_image(ctx, f)[0].cpu().numpy() for f in sorted(glob.glob(os.path.join(d, '*.fz')))])
    want = O.master_median(cube, 'bias')
    del cube
    data, h = fitsio.read_image(path, get_header=True)
    assert data.shape == (10560, 10560) and np.array_equal(data, want)
    assert hv(h, 'NBIAS') == 5 and 'MBRDN16' in h
    ctx.close()
