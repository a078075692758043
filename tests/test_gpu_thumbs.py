"""GPU: transient thumbnails -- bbx_thumb_png8 against the fixture made by the reference's own functions
(tests/golden/thumbs.npz) and against the numpy restatement pinned by it (test_thumbs_host.py) at other sizes;
bbx_thumbnails against numpy slicing with zero padding; the switches of zogy.optimal_subtraction; the operator's
products on the serial path and the list run; one full-size frame."""
import importlib.util
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
import bbx_oracle as O                                  # noqa: E402
import test_thumbs_host as H                            # noqa: E402
from blackbox_amd import fitsio, synth                  # noqa: E402
from blackbox_amd import reduce as R                    # noqa: E402
from blackbox_amd import zogy as G                      # noqa: E402
from blackbox_amd._lib import lib, check, BBXError      # noqa: E402

F = np.float32
NAMES = ('RED', 'REF', 'D', 'SCORR')


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def png8(ctx, stamps):
    """bbx_thumb_png8 on float32 [n, S, S] -> (uint8 planes, limits [n, 2])"""
    n, S = stamps.shape[0], stamps.shape[-1]
    d_in = dev(ctx, stamps.astype(F))
    d_out = torch.full((n, S, S), 7, dtype=torch.uint8, device=ctx.device)
    d_lim = torch.full((n, 2), -1.0, dtype=torch.float64, device=ctx.device)
    check(lib.bbx_thumb_png8(ctx.h, n, S, G._p(d_in), G._p(d_out), G._p(d_lim), ctx.stream()), 'bbx_thumb_png8', ctx.h)
    ctx.sync()
    return d_out.cpu().numpy(), d_lim.cpu().numpy()


def compare_planes(got, want, what):
    """identical on at least 23 of every 24 stamps (one per started group of 24 may differ); no pixel of any stamp off by
    more than one grey level"""
    n = len(want)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16)).reshape(n, -1)
    worst = diff.max(axis=1)
    nbad = int((worst > 0).sum())
    print('{}: {} stamps, {} not identical, largest difference {} grey levels, pixels off: {}'.format(
        what, n, nbad, int(worst.max()), diff.astype(bool).sum(axis=1)[worst > 0].tolist()))
    assert int(worst.max()) <= 1, (what, worst.tolist())
    assert nbad <= -(-n // 24), (what, nbad, n)


def test_png8_fixture(ctx):
    stamps, limits, planes, _ = H.load_fixture()
    got, lim = png8(ctx, stamps)
    rel = np.abs(lim - limits) / np.abs(limits).max(axis=1, keepdims=True)
    print('limits: largest relative difference to the reference {:.3e}'.format(rel.max()))
    assert rel.max() <= 1e-9, rel.max(axis=1).tolist()
    compare_planes(got, planes, 'fixture')


@pytest.mark.parametrize('size', [100, 64, 33, 16, 122])
def test_png8_other_sizes_against_restatement(ctx, size):
    """sizes the fixture does not hold, NaN / inf pixels, few finite values, constant and all-NaN stamps"""
    rs = np.random.RandomState(size)
    n = 24
    stamps = rs.normal(0, 10, (n, size, size)).astype(F)
    yy, xx = np.mgrid[0:size, 0:size]
    for k in range(n):
        stamps[k] += F(rs.uniform(5, 3000)) * np.exp(-((yy - size // 2) ** 2 + (xx - size // 2) ** 2) / 6.0).astype(F)
    stamps[1, :, :size // 3] = 0                                     # a padded band
    stamps[2].reshape(-1)[rs.choice(size * size, size, replace=False)] = np.nan
    stamps[3, 0, :5] = (np.inf, -np.inf, np.nan, np.inf, -np.inf)
    stamps[4] = np.nan; stamps[4, 1, :4] = (3, 1, 2, 7)              # four finite values: sample minimum / maximum
    stamps[5] = np.nan; stamps[5, 2, :9] = np.arange(9) ** 2         # nine: the fit runs
    stamps[6] = 42.5                                                 # constant -> zeros (our convention)
    stamps[7] = np.nan                                               # nothing finite -> zeros, limits (0, 0)
    stamps[8] = np.round(stamps[8] / 8) * 8                          # many ties in the sort
    got, lim = png8(ctx, stamps)
    want = [H.display_plane(s) for s in stamps]
    wl = np.array([w[1] for w in want])
    den = np.maximum(np.abs(wl).max(axis=1, keepdims=True), 1e-300)
    assert (np.abs(lim - wl) / den).max() <= 1e-9, (np.abs(lim - wl) / den).max(axis=1).tolist()
    assert not got[6].any() and not got[7].any() and lim[7].tolist() == [0.0, 0.0] and lim[6, 0] == lim[6, 1] == 42.5
    compare_planes(got, np.stack([w[0] for w in want]), 'size %d' % size)


def test_png8_refuses_what_does_not_fit_lds(ctx):
    d = torch.zeros(4 * 128 * 128, dtype=torch.float32, device=ctx.device)
    o = torch.zeros(4 * 128 * 128, dtype=torch.uint8, device=ctx.device)
    for size in (123, 128, 4096):
        with pytest.raises(BBXError) as e:
            check(lib.bbx_thumb_png8(ctx.h, 1, size, G._p(d), G._p(o), None, ctx.stream()), 'bbx_thumb_png8', ctx.h)
        assert e.value.code == -1
    check(lib.bbx_thumb_png8(ctx.h, 0, 100, None, None, None, ctx.stream()), 'bbx_thumb_png8', ctx.h)      # nothing to do
    ctx.sync()


def slices(frames, ys, xs, size):
    """numpy slicing with zero padding: [n, 4, size, size]"""
    ny, nx = frames[0].shape
    out = np.zeros((len(ys), len(frames), size, size), frames[0].dtype)
    for k, (y, x) in enumerate(zip(ys, xs)):
        y0, x0 = y - size // 2, x - size // 2
        a, b, c, d = max(0, y0), min(ny, y0 + size), max(0, x0), min(nx, x0 + size)
        if b > a and d > c:
            for p, f in enumerate(frames):
                out[k, p, a - y0:b - y0, c - x0:d - x0] = f[a:b, c:d]
    return out


def mask_or(masks, ys, xs, win):
    ny, nx = masks[0].shape
    out = np.zeros(len(ys), np.uint8)
    for k, (y, x) in enumerate(zip(ys, xs)):
        y0, x0 = y - win // 2, x - win // 2
        for m in masks:
            out[k] |= np.bitwise_or.reduce(m[max(0, y0):max(0, min(ny, y0 + win)), max(0, x0):max(0, min(nx, x0 + win))], axis=None, initial=0)
    return out


def gather(ctx, frames, ys, xs, size, new_mask, ref_mask, win):
    res = {}
    d_fl = G.thumbnail_stamps(ctx, res, [dev(ctx, f) for f in frames], ys, xs, size, dev(ctx, new_mask),
                              dev(ctx, ref_mask) if ref_mask is not None else None, floats=True, pngs=False, flag_win=win)
    ctx.sync()
    return res['thumbnails'].cpu().numpy(), d_fl.cpu().numpy()


@pytest.mark.parametrize('size', [100, 64])
def test_gather_against_numpy_slicing(ctx, size):
    ny, nx = 700, 900
    yy, xx = np.mgrid[0:ny, 0:nx]
    frames = [(yy * 1000 + xx).astype(F), (xx * 1000 + yy + 0.5).astype(F), -(yy * nx + xx).astype(F), np.sin(yy * 0.37 + xx * 1.3).astype(F)]
    rs = np.random.RandomState(1)
    new_mask = np.where(rs.rand(ny, nx) < 0.02, 2 ** rs.randint(0, 7, (ny, nx)), 0).astype(np.uint8)
    ref_mask = np.where(rs.rand(ny, nx) < 0.02, 2 ** rs.randint(0, 7, (ny, nx)), 0).astype(np.uint8)
    new_mask[0, 0] = 1; ref_mask[ny - 1, nx - 1] = 64
    pos = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1),                      # the four corners
           (0, 450), (ny - 1, 450), (350, 0), (350, nx - 1),                       # each edge
           (size // 2, size // 2), (size // 2 - 1, 200), (ny - size // 2, nx - size // 2), (ny - size // 2 + 1, 300),
           (350, 450), (123, 777), (601, 55), (2, 3), (ny - 3, nx - 2)]
    pos += [(int(rs.randint(0, ny)), int(rs.randint(0, nx))) for _ in range(40)]
    ys, xs = np.array([p[0] for p in pos]), np.array([p[1] for p in pos])
    for masks, win in (((new_mask, ref_mask), 5), ((new_mask,), 5), ((new_mask, ref_mask), 1), ((new_mask, ref_mask), 4), ((new_mask,), 17)):
        got, fl = gather(ctx, frames, ys, xs, size, masks[0], masks[1] if len(masks) > 1 else None, win)
        want = slices(frames, ys, xs, size)
        assert got.tobytes() == want.tobytes()                                     # bit-exact
        assert np.array_equal(fl, mask_or(masks, ys, xs, win)), win
    assert got[12, 0, size // 2, size // 2] == frames[0][350, 450]                 # the peak pixel is [size/2][size/2]


def moffat_stamp(S, fwhm):
    a = fwhm / (2 * np.sqrt(2 ** (1 / 2.5) - 1))
    y, x = np.mgrid[0:S, 0:S] - S // 2
    p = (1 + (y * y + x * x) / (a * a)) ** -2.5
    return (p / p.sum()).astype(F)


def zogy_scene():
    """the scene of test_gpu_subtraction.test_optimal_subtraction_chain (80 x 320, sub-images of 40 + 2 x 6)"""
    rs = np.random.RandomState(8)
    size, border, box = 40, 6, 20
    ny, nx = 2 * size, 8 * size
    S = 15
    pn, pr = moffat_stamp(S, 3.6), moffat_stamp(S, 3.0)
    truth = np.zeros((ny, nx))
    for _ in range(25):
        truth[rs.randint(10, ny - 10), rs.randint(10, nx - 10)] += rs.uniform(3e3, 3e4)
    tnew = truth.copy()
    for y, x, f in [(30, 45, 4.0e4), (62, 170, 2.5e4), (40, 120, 6.0e4), (3, 317, 5.0e4)]:
        tnew[y, x] += f

    def conv(img, p):
        k = np.zeros((ny, nx)); h = S // 2
        for j in range(S):
            for i in range(S):
                k[(j - h) % ny, (i - h) % nx] = p[j, i]
        return np.fft.ifft2(np.fft.fft2(img) * np.fft.fft2(k)).real
    sky_n = 300 + 0.2 * np.arange(nx)[None, :] + 0.1 * np.arange(ny)[:, None]
    new = (conv(tnew, pn) + sky_n + rs.normal(0, 14, (ny, nx))).astype(F)
    ref = (conv(truth, pr) + 120 + rs.normal(0, 6, (ny, nx))).astype(F)
    mask_n = np.zeros((ny, nx), np.uint8); mask_n[5:9, 200:230] = 1
    mask_n[28:30, 46:48] = 2                                        # next to a transient: inside its 5 x 5 window
    mask_r = np.zeros((ny, nx), np.uint8); mask_r[64, 171] = 16
    nsub = (ny // size) * (nx // size)
    kw = dict(fratio=1.0, dx=0.03, dy=0.02, subimage_size=size, subimage_border=border, bkg_boxsize=box)
    return new, ref, mask_n, mask_r, np.repeat(pn[None], nsub, 0), np.repeat(pr[None], nsub, 0), kw


@pytest.mark.parametrize('tsize', [None, 32])
def test_optimal_subtraction_switches(ctx, tsize):
    new, ref, mask_n, mask_r, psf_n, psf_r, kw = zogy_scene()

    def call(**extra):
        r = G.optimal_subtraction(ctx, dev(ctx, new), dev(ctx, ref), dev(ctx, mask_n), dev(ctx, mask_r), dev(ctx, psf_n), dev(ctx, psf_r),
                                  **kw, **extra)
        ctx.sync()
        return r
    off = call()
    on = call(thumbnails=True, thumbnail_pngs=True, thumbnail_size=tsize)
    S = tsize or 100
    n = len(on['transients'])
    assert n >= 4 and on['thumbnails'].shape == (n, 4, S, S) and on['thumbnails'].dtype == torch.float32
    assert on['thumbnail_png8'].shape == (n, 4, S, S) and on['thumbnail_png8'].dtype == torch.uint8
    ys, xs = [t['y'] for t in on['transients']], [t['x'] for t in on['transients']]
    frames = [on[k].cpu().numpy() for k in ('data_bkgsub', 'ref_bkgsub', 'D', 'Scorr')]
    th = on['thumbnails'].cpu().numpy()
    assert th.tobytes() == slices(frames, ys, xs, S).tobytes()
    flags = np.array([t['flags'] for t in on['transients']], np.uint8)
    assert np.array_equal(flags, mask_or((mask_n, mask_r), ys, xs, 5)) and flags.any()
    want = np.stack([H.display_plane(s)[0] for s in th.reshape(-1, S, S)])
    compare_planes(on['thumbnail_png8'].cpu().numpy().reshape(-1, S, S), want, 'zogy scene, size %d' % S)
    # switched off: no new key, everything else equal
    assert set(on) - set(off) == {'thumbnails', 'thumbnail_png8'} and set(off) <= set(on)
    assert all('flags' not in t for t in off['transients'])
    assert [{k: v for k, v in t.items() if k != 'flags'} for t in on['transients']] == off['transients']
    for k in off:
        if torch.is_tensor(off[k]):
            assert torch.equal(off[k], on[k]), k
        elif isinstance(off[k], np.ndarray):
            assert np.array_equal(off[k], on[k]), k
    assert dict(off['header_new']) == dict(on['header_new']) and dict(off['header_trans']) == dict(on['header_trans'])
    # only one of the two
    only_png = call(thumbnail_pngs=True, thumbnail_size=tsize)
    assert 'thumbnails' not in only_png and torch.equal(only_png['thumbnail_png8'], on['thumbnail_png8'])
    assert [t['flags'] for t in only_png['transients']] == flags.tolist()
    only_f = call(thumbnails=True, thumbnail_size=tsize)
    assert 'thumbnail_png8' not in only_f and torch.equal(only_f['thumbnails'], on['thumbnails'])
    # no candidates: empty tensors
    none = call(thumbnails=True, thumbnail_pngs=True, thumbnail_size=tsize, nsigma=1e6)
    assert none['transients'] == [] and none['thumbnails'].shape == (0, 4, S, S) and none['thumbnail_png8'].shape == (0, 4, S, S)


# ---- the operator -----------------------------------------------------------------------------------------------------
YS, XS, TEL = 120, 330, 'ML1'


def load_cli():
    spec = importlib.util.spec_from_file_location('bbx_cli', os.path.join(ROOT, 'blackbox.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_thumbnail_products_serial_and_list(tmp_path, ctx):
    """in the style of test_gpu_operator.test_cli_subtraction_products_and_image_list: --save_thumbnails True
    --save_thumbnails_pngs True through --image and through --image_list (plain and --fpack True: the output stage)"""
    cli = load_cli()
    case = synth.make_case(YS, XS, 77, tel=TEL, os_y=20, os_x=45, n_stars=60, n_sat=2, n_cr=40)
    hdr = {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q'}
    raws = []
    # the new frames carry point sources the reference (made below from the frame without them) does not have: transients
    raw_new = case['raw'].astype(np.float64)
    dx = raw_new.shape[1] // 8
    star = moffat_stamp(15, 3.5).astype(np.float64)
    for y, x, peak in ((60, 100, 1500.0), (30, dx + 200, 800.0), (9, 3 * dx + 40, 2500.0), (100, 5 * dx + 290, 1200.0),
                       (75, 7 * dx + 150, 600.0)):                  # rows of the lower channels' data sections
        raw_new[y - 7:y + 8, x - 7:x + 8] += peak * star / star.max()
    raw_new = np.clip(np.rint(raw_new), 0, 65535).astype(case['raw'].dtype)
    for k in range(3):
        p = str(tmp_path / ('ML1_raw%d.fits' % k))
        fitsio.write_image(p, raw_new, dict(hdr, **{'DATE-OBS': '2024-01-02T03:04:0%d' % k}))
        raws.append(p)
    fitsio.write_image(str(tmp_path / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp_path / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp_path / 'xtalk.dat'), case['xtalk'])
    coeffs = O.xtalk_coeffs(case['xtalk'])
    d0, m0, h0, _ = R.reduce_object(ctx, dev(ctx, case['raw']), {}, TEL, mflat=dev(ctx, case['flat']), bpm=dev(ctx, case['bpm']),
                                    xtalk_coeffs=coeffs, exptime=60.0, ysize_chan=YS, xsize_chan=XS, log=logging.getLogger('t'))
    rs = np.random.RandomState(3)
    ref = (d0.cpu().numpy() - 100.0 + rs.normal(0, 4, d0.shape)).astype(F)
    fitsio.write_image(str(tmp_path / 'ref.fits'), ref)
    fitsio.write_image(str(tmp_path / 'psf.fits'), moffat_stamp(15, 3.5))
    common = ['--telescope', TEL, '--mflat', str(tmp_path / 'flat.fits'), '--bpm', str(tmp_path / 'bpm.fits'),
              '--crosstalk', str(tmp_path / 'xtalk.dat'), '--ysize_chan', str(YS), '--xsize_chan', str(XS),
              '--cat_extract', 'True', '--trans_extract', 'True', '--ref', str(tmp_path / 'ref.fits'),
              '--psf_new', str(tmp_path / 'psf.fits'), '--psf_ref', str(tmp_path / 'psf.fits'),
              '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30']
    on = ['--save_thumbnails', 'True', '--save_thumbnails_pngs', 'True']
    name = 'ML1_20240102_030400'

    # switched off (the defaults): today's six columns, no PNG directory
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'off')])
    t_off, _ = fitsio.read_table(str(tmp_path / 'off' / (name + '_red_trans.fits')))
    assert list(t_off) == ['NUMBER', 'X_PEAK', 'Y_PEAK', 'SNR_ZOGY', 'E_FLUX_ZOGY', 'E_FLUXERR_ZOGY']
    assert not os.path.exists(str(tmp_path / 'off' / 'thumbnails'))

    # serial path
    cli.main(common + on + ['--image', raws[0], '--red_dir', str(tmp_path / 'a')])
    base = str(tmp_path / 'a' / (name + '_red'))
    tr, ht = fitsio.read_table(base + '_trans.fits')
    n = len(tr['NUMBER'])
    assert n == R.hval(ht, 'T-NTRANS') and n >= 1
    assert list(tr) == list(t_off) + ['THUMBNAIL_' + c for c in NAMES] + ['FLAGS_MASK']
    for k in t_off:
        assert np.array_equal(tr[k], t_off[k]), k
    # the columns are the slices of the images on disk
    frames = [None, None, fitsio.read_image(base + '_D.fits'), fitsio.read_image(base + '_Scorr.fits')]
    ys, xs = tr['Y_PEAK'] - 1, tr['X_PEAK'] - 1
    for p in (2, 3):
        assert tr['THUMBNAIL_' + NAMES[p]].tobytes() == slices([frames[p]], ys, xs, 100)[:, 0].tobytes()
    assert tr['THUMBNAIL_RED'].shape == (n, 100, 100) and tr['FLAGS_MASK'].dtype == np.uint8
    mask = fitsio.read_image(base.replace('_red', '_mask') + '.fits')
    assert np.array_equal(tr['FLAGS_MASK'], mask_or((mask,), ys, xs, 5))           # (the reference's mask is all zero here)
    pdir = str(tmp_path / 'a' / 'thumbnails' / name)
    want_files = sorted('{}_{}.png'.format(i, c) for i in tr['NUMBER'].tolist() for c in NAMES)
    assert sorted(os.listdir(pdir)) == want_files and len(want_files) == 4 * n
    got = [H.decode_png_gray8(open(os.path.join(pdir, '{}_{}.png'.format(i + 1, c)), 'rb').read()) for i in range(n) for c in NAMES]
    want = [H.display_plane(tr['THUMBNAIL_' + c][i])[0] for i in range(n) for c in NAMES]
    assert all(g.shape == (100, 100) for g in got)
    compare_planes(np.stack(got), np.stack(want), 'PNG files')

    # PNG files alone, into --thumbnails_dir: the table keeps its six columns
    cli.main(common + ['--save_thumbnails_pngs', 'True', '--thumbnails_dir', str(tmp_path / 'th'), '--image', raws[0],
                       '--red_dir', str(tmp_path / 'p')])
    assert list(fitsio.read_table(str(tmp_path / 'p' / (name + '_red_trans.fits')))[0]) == list(t_off)
    assert sorted(os.listdir(str(tmp_path / 'th' / name))) == want_files
    for fn in want_files:
        assert open(str(tmp_path / 'th' / name / fn), 'rb').read() == open(os.path.join(pdir, fn), 'rb').read(), fn

    # the list run, without and with the output stage: identical columns and PNG bytes
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(raws) + '\n')
    for sub, extra in (('b', []), ('c', ['--fpack', 'True'])):
        outs = cli.main(common + on + extra + ['--image_list', lst, '--red_dir', str(tmp_path / sub)])
        assert len(outs) == 3 and all(o and os.path.isfile(o) for o in outs)
        for k in range(3):
            nk = 'ML1_20240102_03040%d' % k
            tb, _ = fitsio.read_table(str(tmp_path / sub / (nk + '_red_trans.fits')))
            assert list(tb) == list(tr)
            for col in tr:
                assert tb[col].tobytes() == tr[col].tobytes(), (sub, k, col)       # (the same field three times)
            d = str(tmp_path / sub / 'thumbnails' / nk)
            assert sorted(os.listdir(d)) == want_files
            for fn in want_files:
                assert open(os.path.join(d, fn), 'rb').read() == open(os.path.join(pdir, fn), 'rb').read(), (sub, k, fn)


def test_fullsize_frame_cutouts(ctx):
    """10560 x 10560, about 2000 candidates: cut-outs and flags against slices taken on the device"""
    ny = nx = 10560
    g = torch.Generator(device=ctx.device); g.manual_seed(5)
    frames = [torch.randn((ny, nx), generator=g, device=ctx.device, dtype=torch.float32) for _ in range(4)]
    mask = (torch.rand((ny, nx), generator=g, device=ctx.device) < 0.01).to(torch.uint8) * 4
    rmask = (torch.rand((ny, nx), generator=g, device=ctx.device) < 0.01).to(torch.uint8) * 32
    rs = np.random.RandomState(9)
    n = 2000
    ys, xs = rs.randint(0, ny, n), rs.randint(0, nx, n)
    ys[:8] = (0, 0, ny - 1, ny - 1, 49, 50, ny - 50, ny - 51); xs[:8] = (0, nx - 1, 0, nx - 1, 5000, 49, nx - 50, 7)
    res = {}
    d_fl = G.thumbnail_stamps(ctx, res, frames, ys, xs, 100, mask, rmask, floats=True, pngs=True)
    ctx.sync()
    th = res['thumbnails']
    assert th.shape == (n, 4, 100, 100) and res['thumbnail_png8'].shape == (n, 4, 100, 100)
    want = torch.zeros_like(th)
    wfl = torch.zeros(n, dtype=torch.uint8, device=ctx.device)
    both = mask | rmask
    for k in range(n):
        y0, x0 = int(ys[k]) - 50, int(xs[k]) - 50
        a, b, c, d = max(0, y0), min(ny, y0 + 100), max(0, x0), min(nx, x0 + 100)
        for p in range(4):
            want[k, p, a - y0:b - y0, c - x0:d - x0] = frames[p][a:b, c:d]
        w = both[max(0, int(ys[k]) - 2):int(ys[k]) + 3, max(0, int(xs[k]) - 2):int(xs[k]) + 3]
        wfl[k] = (w & 4).max() | (w & 32).max()
    assert torch.equal(th, want)
    assert torch.equal(d_fl, wfl)
    # the display planes of a few of them against the restatement
    idx = [0, 3, 5, 100, 999, 1999]
    got = res['thumbnail_png8'][idx].cpu().numpy().reshape(-1, 100, 100)
    wp = np.stack([H.display_plane(s)[0] for s in th[idx].cpu().numpy().reshape(-1, 100, 100)])
    compare_planes(got, wp, 'full-size frame')
