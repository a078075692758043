"""Transient thumbnails, host side (no GPU): the numpy restatement of the display-plane arithmetic against the
fixture made by the reference's own functions (tools/gen_golden_thumbs.py), the table columns, the PNG files,
the command-line flags.

zscale_limits / scale_u8 below restate, in plain numpy with every cast written out,
    data = np.flipud(stamp); vmin, vmax = ZScaleInterval().get_limits(data); scale_data(data, vmin, vmax)
(blackbox.py:2786-2826).  tests/golden/thumbs.npz pins them; the GPU tests (test_gpu_thumbs.py) then use them at
sizes the fixture does not hold.
"""
import hashlib
import importlib.util
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden', 'thumbs.npz')

# sha256 of the `_trans.fits` of TRANSIENTS / HEADER below as the commit before the thumbnails wrote it
PARENT_TRANS_SHA256 = '47d90e9dfae67e46903736ea46df73c3952e0004fc609c73f55ee883cec1019c'
TRANSIENTS = [dict(y=10 + 7 * k, x=900 - 13 * k, scorr=6.5 + k, fpsf=100.25 * (k + 1), fpsferr=3.5 + 0.125 * k) for k in range(5)]
HEADER = {'T-NTRANS': (5, 'number of transient candidates'), 'T-NSIGMA': (6.0, '[sigma] transient detection threshold'),
          'Z-P': (True, 'successfully processed by ZOGY?')}


# ---- the restatement -----------------------------------------------------------------------------------------------
def zscale_limits(data):
    """astropy ZScaleInterval().get_limits of a float32 array -> (vmin, vmax) as Python floats (float64), or None when no
    value is finite.  The weighted least-squares line in closed form (centred sums) instead of numpy.polyfit."""
    v = np.asarray(data, np.float32).reshape(-1)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return None
    stride = int(max(1.0, v.size / 1000))
    s = np.sort(v[::stride][:1000])
    npix = s.size
    vmin, vmax = float(s[0]), float(s[-1])
    minpix = max(5, int(npix * 0.5))
    x = np.arange(npix, dtype=np.float64)
    y = s.astype(np.float64)
    ngood, last = npix, npix + 1
    bad = np.zeros(npix, bool)
    ngrow = max(1, int(npix * 0.01))
    gs = (ngrow - 1) // 2                         # numpy.convolve(bad, ones(ngrow), 'same'): out[i] = any(bad[i + gs - ngrow + 1 : i + gs + 1])
    slope = 0.0
    for _ in range(5):
        if ngood >= last or ngood < minpix:
            break
        g = ~bad
        n = float(g.sum())
        xm, ym = x[g].sum() / n, y[g].sum() / n
        dx = x[g] - xm
        slope = float((dx * (y[g] - ym)).sum() / (dx * dx).sum())
        icpt = ym - slope * xm
        flat = y - (slope * x + icpt)
        f = flat[g]
        mf = f.sum() / n
        thr = 2.5 * np.sqrt(((f - mf) ** 2).sum() / n)
        bad = bad | (flat < -thr) | (flat > thr)
        grown = np.zeros(npix, bool)
        for j in np.nonzero(bad)[0]:
            grown[max(0, j - gs):max(0, min(npix, j - gs + ngrow))] = True
        bad = grown
        last, ngood = ngood, int((~bad).sum())
    if ngood >= minpix:
        slope = slope / 0.25
        c = (npix - 1) // 2
        # numpy.median of float32 samples: the float32 mean of the middle pair
        med = s[npix // 2] if npix % 2 else np.float32(np.float32(s[npix // 2 - 1] + s[npix // 2]) / np.float32(2))
        vmin = max(vmin, float(med) - (c - 1) * slope)
        vmax = min(vmax, float(med) + (npix - c) * slope)
    return vmin, vmax


def scale_u8(data, vmin, vmax):
    """scale_data in numpy's float32: three separately rounded operations, clip, truncate; NaN -> 0"""
    d = np.array(data, np.float32)
    out = np.zeros(d.shape, np.uint8)
    if vmax == vmin:
        return out
    with np.errstate(invalid='ignore', over='ignore'):
        d = d - np.float32(vmin)
        d = d / np.float32(np.float64(vmax) - np.float64(vmin))
        d = d * np.float32(255)
        m = d > 0
        out[m] = np.minimum(d[m], np.float32(255)).astype(np.uint8)
    return out


def display_plane(stamp):
    """what save_thumbs_row makes of one cut-out -> (uint8 plane, (vmin, vmax)); zeros and (0, 0) without a finite value"""
    data = np.flipud(np.asarray(stamp, np.float32))
    lim = zscale_limits(data)
    if lim is None:
        return np.zeros(data.shape, np.uint8), (0.0, 0.0)
    return scale_u8(data, *lim), lim


def load_fixture():
    z = np.load(GOLDEN)
    counts, scale = z['counts'], z['scale']
    stamps = counts.astype(np.float32) * scale.astype(np.float32)[:, None, None]
    stamps[counts == z['nan_count']] = np.nan
    return stamps, z['limits'], z['planes'], z['kinds']


def decode_png_gray8(buf):
    """8-bit grayscale PNG -> uint8 [h, w]: Pillow where it is installed, else the chunks by hand (filter 0-4)"""
    try:
        import io
        from PIL import Image
        im = Image.open(io.BytesIO(buf))
        assert im.mode == 'L'
        return np.array(im)
    except ImportError:
        pass
    assert buf[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, w = 8, b'', None
    while pos < len(buf):
        n, tag = struct.unpack('>I4s', buf[pos:pos + 8])
        body = buf[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', buf[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b'IHDR':
            w, h, depth, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', body)
            assert (depth, ctype, comp, filt, lace) == (8, 0, 0, 0, 0)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any()                    # our writer uses filter type 0 only
    return raw[:, 1:].copy()


# ---- tests ---------------------------------------------------------------------------------------------------------
def test_fixture_contents():
    stamps, limits, planes, kinds = load_fixture()
    assert stamps.shape[0] >= 24 and stamps.shape[1:] == (100, 100) and planes.shape == stamps.shape
    assert set(kinds.tolist()) == {0, 1, 2, 3}
    assert all(np.nanmax(s) > np.nanmin(s) for s in stamps)                       # no constant stamp
    assert sum(int(np.isnan(s).any()) for s in stamps) >= 3
    assert os.path.getsize(GOLDEN) <= 1 << 20


def test_restatement_reproduces_reference():
    """the restatement gives the reference's uint8 planes byte for byte; its limits agree to 1e-9 relative (closed-form
    line against numpy.polyfit's least squares)"""
    stamps, limits, planes, _ = load_fixture()
    for k, stamp in enumerate(stamps):
        plane, lim = display_plane(stamp)
        ref = limits[k]
        scale = max(abs(ref[0]), abs(ref[1]))
        assert abs(lim[0] - ref[0]) <= 1e-9 * scale and abs(lim[1] - ref[1]) <= 1e-9 * scale, (k, lim, ref)
        assert plane.tobytes() == planes[k].tobytes(), (k, int((plane != planes[k]).sum()))


def test_table_roundtrip_tdim(tmp_path):
    from blackbox_amd import catalogs, fitsio
    rng = np.random.default_rng(3)
    th = rng.normal(size=(3, 4, 100, 100)).astype(np.float32)
    trans = [dict(t, flags=f) for t, f in zip(TRANSIENTS[:3], (0, 5, 96))]
    path = str(tmp_path / 'a_trans.fits')
    catalogs.format_cat(catalogs.transient_table(trans, th), path, cat_type='trans', header2add=HEADER)
    cols, h = fitsio.read_table(path)
    assert list(cols) == ['NUMBER', 'X_PEAK', 'Y_PEAK', 'SNR_ZOGY', 'E_FLUX_ZOGY', 'E_FLUXERR_ZOGY', 'THUMBNAIL_RED',
                          'THUMBNAIL_REF', 'THUMBNAIL_D', 'THUMBNAIL_SCORR', 'FLAGS_MASK']
    for k, name in enumerate(('THUMBNAIL_RED', 'THUMBNAIL_REF', 'THUMBNAIL_D', 'THUMBNAIL_SCORR')):
        assert str(fitsio._hv(h, 'TFORM%d' % (7 + k))).strip() == '10000E' and str(fitsio._hv(h, 'TDIM%d' % (7 + k))).strip() == '(100,100)'
        assert cols[name].shape == (3, 100, 100) and cols[name].dtype == np.float32
        assert np.array_equal(cols[name], th[:, k])
    assert str(fitsio._hv(h, 'TFORM11')).strip() == 'B' and cols['FLAGS_MASK'].tolist() == [0, 5, 96]
    assert cols['X_PEAK'].tolist() == [t['x'] + 1 for t in trans]
    # a plain write_table: non-square cells keep their shape, one- and two-dimensional columns get no TDIM
    p2 = str(tmp_path / 'b.fits')
    fitsio.write_table(p2, {'A': np.arange(4, dtype=np.int32), 'B': np.ones((4, 3), np.float32),
                            'C': np.arange(4 * 2 * 5, dtype=np.float32).reshape(4, 2, 5)})
    c2, h2 = fitsio.read_table(p2)
    assert 'TDIM1' not in h2 and 'TDIM2' not in h2 and str(fitsio._hv(h2, 'TDIM3')).strip() == '(5,2)'
    assert c2['B'].shape == (4, 3) and c2['C'].shape == (4, 2, 5) and c2['C'][3, 1, 4] == 39


def test_table_without_thumbnails_is_unchanged(tmp_path):
    from blackbox_amd import catalogs
    path = str(tmp_path / 'p_trans.fits')
    catalogs.write_small_products([('trans', (TRANSIENTS, path, dict(HEADER)))])
    assert hashlib.sha256(open(path, 'rb').read()).hexdigest() == PARENT_TRANS_SHA256
    # 'flags' in the rows alone (PNG files without the columns) does not change the table either
    p2 = str(tmp_path / 'q_trans.fits')
    catalogs.write_small_products([('trans', ([dict(t, flags=3) for t in TRANSIENTS], p2, dict(HEADER), dict(thumbnails=None, png8=None)))])
    assert open(p2, 'rb').read() == open(path, 'rb').read()


def test_png_files_decode_to_their_planes(tmp_path):
    from blackbox_amd import catalogs
    rng = np.random.default_rng(5)
    png8 = rng.integers(0, 256, (3, 4, 100, 100), dtype=np.uint8)
    png8[1, 2] = 0
    png8[2, 3, :50] = 255
    dest = str(tmp_path / 'thumbnails' / 'frame')
    os.makedirs(dest)
    open(os.path.join(dest, '99_RED.png'), 'wb').write(b'stale')                   # an earlier reduction's file goes away
    written = catalogs.save_png_thumbnails(png8, [1, 2, 3], dest)
    assert sorted(os.listdir(dest)) == sorted('{}_{}.png'.format(n, c) for n in (1, 2, 3) for c in ('RED', 'REF', 'D', 'SCORR'))
    assert len(written) == 12
    for i, n in enumerate((1, 2, 3)):
        for j, c in enumerate(('RED', 'REF', 'D', 'SCORR')):
            buf = open(os.path.join(dest, '{}_{}.png'.format(n, c)), 'rb').read()
            assert np.array_equal(decode_png_gray8(buf), png8[i, j])
    # a non-square plane through the zlib-only decoder as well
    plane = rng.integers(0, 256, (7, 13), dtype=np.uint8)
    buf = catalogs._png_gray8(plane)
    assert buf[:8] == b'\x89PNG\r\n\x1a\n' and struct.unpack('>II', buf[16:24]) == (13, 7)
    assert np.array_equal(decode_png_gray8(buf), plane)


def test_zero_rows_make_no_directory(tmp_path):
    from blackbox_amd import catalogs, fitsio
    dest = str(tmp_path / 'thumbnails' / 'frame')
    path = str(tmp_path / 'z_trans.fits')
    extra = dict(thumbnails=np.zeros((0, 4, 100, 100), np.float32), png8=np.zeros((0, 4, 100, 100), np.uint8), png_dir=dest)
    catalogs.write_small_products([('trans', ([], path, dict(HEADER), extra))])
    assert not os.path.exists(dest) and not os.path.exists(os.path.dirname(dest))
    cols, h = fitsio.read_table(path)
    assert int(fitsio._hv(h, 'NAXIS2')) == 0 and cols['THUMBNAIL_D'].shape == (0, 100, 100) and 'FLAGS_MASK' in cols
    assert catalogs.save_png_thumbnails(np.zeros((0, 4, 100, 100), np.uint8), [], dest) == [] and not os.path.exists(dest)


def test_cli_parses_thumbnail_flags():
    spec = importlib.util.spec_from_file_location('bbx_cli_thumbs', os.path.join(ROOT, 'blackbox.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    a = ap.parse_args(['--image', 'x.fits'])
    assert a.save_thumbnails is None and a.save_thumbnails_pngs is None and a.thumbnails_dir is None
    a = ap.parse_args(['--image', 'x.fits', '--save_thumbnails', 'True', '--save_thumbnails_pngs', 'false', '--thumbnails_dir', '/data/th'])
    assert a.save_thumbnails is True and a.save_thumbnails_pngs is False and a.thumbnails_dir == '/data/th'
    from blackbox_amd import settings
    assert settings.save_thumbnails is False and settings.save_thumbnails_pngs is False
    assert settings.size_thumbnails == 100 and settings.thumbnails_dir is None and settings.trans_flags_window == 5
