"""GPU: the limiting-flux image of the reduced frame (bbx_limflux.hip; include/bbx.h: bbx_limflux_image) against the float64 numpy
restatement limflux_ref.py, against bbx_psf_optflux_sigma's err, and blackbox.py --limmag on the command line.

Tolerance against the restatement (limflux_ref.tolerance).  Every term of den is non-negative, so a float32 sum of n = T^2 terms in
any order lies within (n + 2) 2^-24 of the exact sum, relative; lim = nsigma den^(-1/2) takes half of that; allowed is
(T^2 / 2 + 8) 2^-24 relative, the + 8 for the division and the square root: 7.2e-5 at T = 49.  Where the kernel reads sigma off a
MiniImage the restatement is given that image's frame, which include/bbx.h states to lie within 3e-7 of what the kernel reads:
1e-6 more.  Zeros are zeros exactly, the windows are equal exactly, no pixel is left out of the comparison."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import limflux_ref as L                       # noqa: E402
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G            # noqa: E402
from blackbox_amd import limflux as LF        # noqa: E402
from blackbox_amd._lib import lib             # noqa: E402

F = np.float32
SHAPES = {'150x203': (150, 203, 64, 2, 3), '97x130': (97, 130, 50, 1, 2)}      # ny, nx, size, nsy, nsx: no multiples of anything
NSIGMA = 5.0


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def make_case(ny, nx, size, nsy, nsx):
    """sigma with a gradient, a NaN, a zero, a negative, an infinite value and one whose square underflows; a mask with isolated pixels, a masked row at the frame's edge, a
    block larger than the largest stamp and a block straddling a tile seam"""
    rs = np.random.RandomState(ny * 1000 + nx)
    gy, gx = np.mgrid[0:ny, 0:nx]
    sigma = (3.0 + 0.011 * gy + 0.017 * gx).astype(F)
    sigma[5, 7], sigma[ny // 2, nx // 3], sigma[ny - 4, nx - 9] = np.nan, 0.0, -2.5
    sigma[ny // 3, nx - 2] = np.inf
    sigma[ny - 20, nx // 2] = 1e-25                                  # sigma * sigma underflows: W is the largest float32, not inf
    mask = np.zeros((ny, nx), np.uint8)
    iso = rs.randint(0, ny, 25), rs.randint(0, nx, 25)
    mask[iso] = 1 << rs.randint(0, 7, 25).astype(np.uint8)
    mask[0, :] = 32                                                  # a masked row at the frame's edge
    mask[20:75, 4:59] = 4                                            # 55 x 55: larger than S = 49
    if nsy > 1:
        mask[size - 6:size + 7, size - 9:size + 5] = 8               # across the seam row and column
    mask[30:44, size - 5:size + 8] = 2                               # across the seam column
    return sigma, mask


@pytest.fixture(scope='module')
def cases():
    return {k: make_case(*v) for k, v in SHAPES.items()}


def gpu_lim(ctx, sigma, mask, planes, size, nsy, nsx, frac, nsigma=NSIGMA):
    lim, win = LF.limflux_image(ctx, sigma if not isinstance(sigma, np.ndarray) else dev(ctx, sigma), dev(ctx, mask) if mask is not None else None,
                                dev(ctx, planes), size, nsy, nsx, nsigma=nsigma, frac=frac)
    ctx.sync()
    return lim.cpu().numpy(), win.cpu().numpy()


def close(got, win, want, label, mini=False):
    """the image and the windows against the restatement's dict -> the largest ratio of a difference to its bound"""
    assert got.dtype == F and win.dtype == np.int32
    assert want['margin'] >= 1e-9, (label, want['margin'])           # (else the summation order could move a window)
    assert np.array_equal(win, want['win']), (label, win, want['win'])
    lim = want['lim']
    assert np.isfinite(got).all(), label
    assert np.array_equal(got == 0, lim == 0), (label, int((got == 0).sum()), int((lim == 0).sum()))
    tol = L.tolerance(want['tmap'].astype(np.float64), mini)         # per pixel: the window of its tile
    ratio = float((np.abs(got - lim) / (tol * np.where(lim > 0, lim, 1.0))).max())
    print('%s: T %s, largest difference %.3f of the bound (%.2e at the largest window)' % (label, sorted(set(win.tolist())), ratio, tol.max()))
    assert ratio <= 1.0, (label, ratio)
    return ratio


@pytest.mark.parametrize('frac', [0.0, 1e-4, 0.5])
@pytest.mark.parametrize('S', [9, 25, 49])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_against_the_restatement(ctx, cases, shape, S, frac):
    ny, nx, size, nsy, nsx = SHAPES[shape]
    sigma, mask = cases[shape]
    planes = L.seam_planes(S, nsy, nsx)
    want = L.limflux_ref(sigma, mask, planes, size, nsy, nsx, nsigma=NSIGMA, frac=frac)
    got, win = gpu_lim(ctx, sigma, mask, planes, size, nsy, nsx, frac)
    close(got, win, want, '%s S %d frac %g' % (shape, S, frac))
    assert (got == 0).sum() > 0 and (got > 0).sum() > got.size // 2
    if S < 49:
        assert not got[20 + S // 2:75 - S // 2, 4 + S // 2:59 - S // 2].any()      # inside the masked block nothing carries weight


def test_the_output_changes_exactly_at_the_seams(ctx):
    """uniform sigma, no mask: away from the frame's edge every pixel of a tile has the same bits, and the value jumps at the seam
    row and column -- and nowhere else: the columns past nsx * size belong to the last tile"""
    ny, nx, size, nsy, nsx = SHAPES['150x203']
    S = 9
    planes = L.seam_planes(S, nsy, nsx)                              # FWHM 2.0 | 5.68 | 2.0 over 5.68 | 2.0 | 5.68
    got, win = gpu_lim(ctx, np.full((ny, nx), 4.0, F), None, planes, size, nsy, nsx, 0.0)
    assert list(win) == [S] * 6
    h = S // 2
    a, b = got[20, 20], got[20, 70]
    assert b > 1.5 * a > 0
    assert (got[h:size, h:size] == a).all() and (got[h:size, size:2 * size] == b).all() and (got[h:size, 2 * size:nx - h] == a).all()
    assert (got[size:ny - h, h:size] == b).all() and (got[size:ny - h, size:2 * size] == a).all() and (got[size:ny - h, 2 * size:nx - h] == b).all()
    assert got[size - 1, 20] == a and got[size, 20] == b and got[20, size - 1] == a and got[20, size] == b
    assert got[20, 3 * size - 1] == got[20, 3 * size] == got[20, nx - h - 1] == a      # no seam at 192: the clamp
    assert got[0, 0] > a and got[ny - 1, nx - 1] > b                 # at the frame's edge part of the stamp carries no weight
    want = L.limflux_ref(np.full((ny, nx), 4.0, F), None, planes, size, nsy, nsx, nsigma=NSIGMA, frac=0.0)
    close(got, win, want, 'seams')


def test_frame_and_mini_image_agree(ctx):
    """the sigma map as a MiniImage and as the frame made of it: both against the restatement on that frame, and one against the other"""
    ny, nx, size, nsy, nsx, box, S = 160, 200, 64, 2, 3, 20, 25
    rs = np.random.RandomState(4)
    mini = (5.0 + 1.5 * rs.uniform(0, 1, (ny // box, nx // box))).astype(F)
    mi = G.MiniImage(ctx, mini, box, interp_Xchan=True)
    fr = mi.frame(ctx).contiguous()
    ctx.sync()
    mask = np.zeros((ny, nx), np.uint8)
    mask[40:52, 100:140] = 1
    mask[159, :] = 16
    planes = L.seam_planes(S, nsy, nsx)
    want = L.limflux_ref(fr.cpu().numpy(), mask, planes, size, nsy, nsx, nsigma=NSIGMA, frac=1e-4)
    g_fr, w_fr = gpu_lim(ctx, fr, mask, planes, size, nsy, nsx, 1e-4)
    g_mi, w_mi = gpu_lim(ctx, mi, mask, planes, size, nsy, nsx, 1e-4)
    close(g_fr, w_fr, want, 'sigma frame')
    close(g_mi, w_mi, want, 'sigma off its mini image', mini=True)
    assert np.array_equal(w_fr, w_mi) and np.array_equal(g_fr == 0, g_mi == 0)
    tol = L.tolerance(want['tmap'].astype(np.float64), mini=True)
    assert (np.abs(g_fr - g_mi) <= tol * g_fr).all()


def test_against_the_optimal_flux_error(ctx):
    """frac = 0, no mask, D = 0: lim / nsigma is bbx_psf_optflux_sigma's err with the tile's plane as stamp, within
    2 (S^2 / 2 + 8) 2^-24, at 200 random integer positions; at some the stamp runs off the frame"""
    ny, nx, size, nsy, nsx = SHAPES['150x203']
    S = 25
    gy, gx = np.mgrid[0:ny, 0:nx]
    sigma = (3.0 + 0.011 * gy + 0.017 * gx).astype(F)
    planes = L.seam_planes(S, nsy, nsx)
    got, win = gpu_lim(ctx, sigma, None, planes, size, nsy, nsx, 0.0)
    rs = np.random.RandomState(9)
    ys, xs = rs.randint(0, ny, 200).astype(np.int32), rs.randint(0, nx, 200).astype(np.int32)
    ys[:8], xs[:8] = (0, 0, ny - 1, ny - 1, 3, 70, ny - 2, 64), (0, nx - 1, 0, nx - 1, 100, 1, 190, nx - 1)
    off_frame = (ys < S // 2) | (xs < S // 2) | (ys >= ny - S // 2) | (xs >= nx - S // 2)
    assert off_frame.sum() >= 8 and (~off_frame).sum() >= 50
    t = G.tile_index(ys, xs, size, nsy, nsx)
    assert len(set(t.tolist())) == nsy * nsx
    stamps = dev(ctx, planes[t])
    _, err = G.psf_optflux(ctx, torch.zeros((ny, nx), dtype=torch.float32, device=ctx.device), dev(ctx, sigma), stamps, ys, xs, v_is_sigma=True)
    ctx.sync()
    err = err.cpu().numpy().astype(np.float64)
    mine = got[ys, xs].astype(np.float64) / NSIGMA
    tol = 2 * (S * S / 2.0 + 8) * 2.0 ** -24
    ratio = np.abs(mine - err) / (tol * err)
    print('against bbx_psf_optflux_sigma: largest difference %.3f of the bound %.2e' % (ratio.max(), tol))
    assert (err > 0).all() and ratio.max() <= 1.0


def test_same_input_same_bits_and_nsigma_scales(ctx, cases):
    ny, nx, size, nsy, nsx = SHAPES['97x130']
    sigma, mask = cases['97x130']
    planes = L.seam_planes(49, nsy, nsx)
    a, wa = gpu_lim(ctx, sigma, mask, planes, size, nsy, nsx, 1e-4)
    b, wb = gpu_lim(ctx, sigma, mask, planes, size, nsy, nsx, 1e-4)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(wa, wb)
    c, _ = gpu_lim(ctx, sigma, mask, planes, size, nsy, nsx, 1e-4, nsigma=10.0)
    assert np.array_equal(c, (a * F(2.0)))


def test_a_stamp_without_a_sum(ctx):
    ny, nx, size, nsy, nsx = 70, 90, 40, 1, 2
    planes = np.stack([L.moffat(9, 3.0), np.zeros((9, 9), F)])
    got, win = gpu_lim(ctx, np.full((ny, nx), 2.0, F), None, planes, size, nsy, nsx, 1e-4)
    assert win[1] == 0 and win[0] > 0 and (got[:, :40] > 0).all() and not got[:, 40:].any()
    planes[1] = np.nan
    got, win = gpu_lim(ctx, np.full((ny, nx), 2.0, F), None, planes, size, nsy, nsx, 0.0)
    assert list(win) == [9, 0] and (got[:, :40] > 0).all() and not got[:, 40:].any()


def test_empty_frame_returns_and_bad_arguments_write_nothing(ctx):
    """an empty frame comes back as an empty image (that nothing is launched for it is tests/test_limflux_host.py's, with a context of
    zeros that no launch would survive); a refused call leaves the output as it was"""
    planes = dev(ctx, L.seam_planes(9, 2, 2))
    for shape in ((0, 50), (40, 0)):
        lim, win = LF.limflux_image(ctx, torch.zeros(shape, dtype=torch.float32, device=ctx.device), None, planes, 25, 2, 2)
        assert tuple(lim.shape) == shape
    ctx.sync()
    sg = torch.ones((40, 50), dtype=torch.float32, device=ctx.device)
    out = torch.full((40, 50), -1.0, dtype=torch.float32, device=ctx.device)
    p = lambda t: t.data_ptr()           # noqa: E731
    mi = G.MiniImage(ctx, np.ones((4, 5), F), 10, interp_Xchan=True)

    def call(sigma=p(sg), mini=None, S=9, frac=1e-4, pl=planes):
        return lib.bbx_limflux_image(ctx.h, 40, 50, sigma, mini, None, S, p(pl), 25, 2, 2, 5.0, frac, p(out), None, ctx.stream())
    assert call(sigma=None) == -1 and call(mini=mi.ref()) == -1      # neither form of the sigma map, both
    assert call(S=8) == -1 and call(S=51) == -1 and call(frac=1.0) == -1 and call(frac=-0.1) == -1
    ctx.sync()
    assert (out == -1.0).all()                                        # nothing was written
    for bad in (dict(frac=1.0), dict(nsigma=-1.0)):
        with pytest.raises(ValueError):
            LF.limflux_image(ctx, sg, None, planes, 25, 2, 2, **bad)
    with pytest.raises(ValueError):
        LF.limflux_image(ctx, sg, None, dev(ctx, L.seam_planes(8 + 1, 2, 2)[:, :8, :8]), 25, 2, 2)
    assert call() == 0
    ctx.sync()
    assert (out > 0).all()


# ---- the stage -------------------------------------------------------------------------------------------------------
LIMKEYS = ['LIMMAG-P', 'LIMNSIG', 'LIMEFLUX', 'LIMMAG', 'LIMFNU', 'LIMPFRAC', 'LIMWIN', 'LIMNPIX']


def test_stage_failure_and_no_psf_keep_the_frame(ctx, monkeypatch):
    """optimal_subtraction(limmag=True): the image and its statistic; an exception in the stage, or no PSF: LIMMAG-P False, the other
    keys 'None', no image; a bad parameter is a ValueError"""
    import test_match_host as H
    import test_gpu_match as M
    sc = H.make_scene()
    new, new_mask, ref, kw = M.subtraction_inputs(ctx, sc)
    kw = dict(kw, cat_extract=True, fratio=1.0)
    base = M.run_sub(ctx, new, new_mask, ref, kw)
    assert 'limflux' not in base and not any(k.startswith('LIM') for k in base['header_new'])
    on = M.run_sub(ctx, new, new_mask, ref, kw, limmag=True)
    hn = on['header_new']
    assert [k for k in hn if k.startswith('LIM')] == LIMKEYS and hn['LIMMAG-P'][0] is True
    lim = on['limflux'].cpu().numpy()
    st = G.fetch(ctx, G.frame_clipped_stats_enqueue(ctx, on['limflux'], new_mask))
    assert hn['LIMNPIX'][0] == int(st[0]) > 1000 and np.array_equal(on['limflux_info']['stat'], st)
    assert hn['LIMEFLUX'][0] == 'None' and hn['LIMNSIG'][0] == 5.0 and hn['LIMPFRAC'][0] == 1e-4
    assert hn['LIMWIN'][0] == int(np.median(on['limflux_info']['win'])) and lim.shape == tuple(new.shape) and (lim > 0).all()
    # the catalogue is the one of a run without the switch
    for k in base['catalog']:
        assert np.array_equal(base['catalog'][k], on['catalog'][k]), k
    # the image is limflux_image on the run's own sigma map and stamps
    sub = G.subimage_psfs(ctx, kw['psf_new'], H.NSY, H.NSX, H.SIZE)
    again, win = LF.limflux_image(ctx, on['bkg_std'], new_mask, sub.contiguous(), H.SIZE, H.NSY, H.NSX)
    ctx.sync()
    assert np.array_equal(win.cpu().numpy(), on['limflux_info']['win'])
    # (the stage may have read sigma off the mini image and the result carry its frame, or the other way round: the 1e-6 of that read)
    tol = L.tolerance(L.tile_windows(win.cpu().numpy(), lim.shape, H.SIZE, H.NSY, H.NSX).astype(np.float64), mini=True)
    assert (np.abs(again.cpu().numpy() - lim) <= tol * lim).all()

    def boom(*a, **k):
        raise RuntimeError('made to fail')
    monkeypatch.setattr(G, '_limflux_image', boom)
    bad = M.run_sub(ctx, new, new_mask, ref, kw, limmag=True)
    monkeypatch.undo()
    nopsf = M.run_sub(ctx, new, new_mask, None, dict(kw, psf_new=None), limmag=True)
    for res in (bad, nopsf):
        h = res['header_new']
        assert 'limflux' not in res and h['LIMMAG-P'][0] is False and all(h[k][0] == 'None' for k in LIMKEYS[1:])
    for k in base['catalog']:
        assert np.array_equal(base['catalog'][k], bad['catalog'][k]), k
    with pytest.raises(ValueError):
        M.run_sub(ctx, new, new_mask, ref, kw, limmag=True, limmag_psf_frac=1.0)


# ---- command line ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cli_case(tmp_path_factory, ctx):
    """the small raw frame of test_gpu_aper.py's command-line test, its flat, bad-pixel mask, crosstalk file, reference and PSF"""
    import logging
    import bbx_oracle as O
    import test_gpu_operator as OP
    from blackbox_amd import fitsio, synth
    tmp = tmp_path_factory.mktemp('limflux_cli')
    case = synth.make_case(OP.YS, OP.XS, 77, tel=OP.TEL, os_y=20, os_x=45, n_stars=60, n_sat=2, n_cr=40)
    raws = []
    for k in range(2):
        raws.append(str(tmp / ('ML1_raw%d.fits' % k)))
        fitsio.write_image(raws[-1], case['raw'], {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q', 'DATE-OBS': '2024-01-02T03:04:0%d' % k})
    fitsio.write_image(str(tmp / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp / 'xtalk.dat'), case['xtalk'])
    d0 = R.reduce_object(ctx, dev(ctx, case['raw']), {}, OP.TEL, mflat=dev(ctx, case['flat']), bpm=dev(ctx, case['bpm']),
                         xtalk_coeffs=O.xtalk_coeffs(case['xtalk']), exptime=60.0, ysize_chan=OP.YS, xsize_chan=OP.XS,
                         log=logging.getLogger('t'))[0]
    rs = np.random.RandomState(3)
    fitsio.write_image(str(tmp / 'ref.fits'), (d0.cpu().numpy() - 100.0 + rs.normal(0, 4, d0.shape)).astype(F))
    psf = OP.moffat(15, 3.5)
    fitsio.write_image(str(tmp / 'psf.fits'), psf)
    nopsf = ['--telescope', OP.TEL, '--mflat', str(tmp / 'flat.fits'), '--bpm', str(tmp / 'bpm.fits'),
             '--crosstalk', str(tmp / 'xtalk.dat'), '--ysize_chan', str(OP.YS), '--xsize_chan', str(OP.XS),
             '--cat_extract', 'True', '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30']
    common = nopsf + ['--trans_extract', 'True', '--ref', str(tmp / 'ref.fits'), '--psf_new', str(tmp / 'psf.fits'), '--psf_ref', str(tmp / 'psf.fits')]
    cli = OP.load_cli()
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp / 'on'), '--limmag', 'True'])
    return dict(tmp=tmp, raws=raws, common=common, nopsf=nopsf, cli=cli, psf=psf, shape=tuple(d0.shape))


RED = 'ML1_20240102_03040%d_red'


def test_cli_writes_the_image_and_the_keys(ctx, cli_case):
    from blackbox_amd import fitsio
    c = cli_case
    base = str(c['tmp'] / 'on' / (RED % 0))
    lim, hl = fitsio.read_image(base + '_limmag.fits', get_header=True)
    assert lim.dtype == F and lim.shape == c['shape'] and R.hval(hl, 'LIMUNIT') == 'e-'
    for name in (base + '.fits', base + '_hdr.fits'):
        h = fitsio.read_hdus(name)[0][0]
        for k in LIMKEYS:
            assert k in h, (name, k)
        print(os.path.basename(name), {k: R.hval(h, k) for k in LIMKEYS})
        assert R.hval(h, 'LIMMAG-P') is True and R.hval(h, 'LIMNSIG') == 5.0 and R.hval(h, 'LIMPFRAC') == 1e-4
        assert R.hval(h, 'LIMEFLUX') > 0 and R.hval(h, 'LIMMAG') == 'None' and R.hval(h, 'LIMFNU') == 'None'
        assert R.hval(h, 'LIMNPIX') > 1000 and R.hval(h, 'LIMWIN') % 2 == 1
    # the image is limflux_image on the run's own products: sigma mini image, mask, PSF
    size, box = 120, 30
    ny, nx = c['shape']
    nsy, nsx = ny // size, nx // size
    mini_std = fitsio.read_image(base + '_bkg_std_mini.fits').astype(F)
    mask = fitsio.read_image(base.replace('_red', '_mask') + '.fits').astype(np.uint8)
    mi = G.MiniImage(ctx, mini_std, box, interp_Xchan=False)
    sub = G.subimage_psfs(ctx, dev(ctx, c['psf'] / c['psf'].sum()), nsy, nsx, size)
    got, win = LF.limflux_image(ctx, mi, dev(ctx, mask), sub.contiguous(), size, nsy, nsx)
    ctx.sync()
    got, win = got.cpu().numpy(), win.cpu().numpy()
    assert R.hval(h, 'LIMWIN') == int(np.median(win)) and (win > 0).all() and len(set(win.tolist())) == 1
    tol = L.tolerance(L.tile_windows(win, lim.shape, size, nsy, nsx).astype(np.float64), mini=True)      # (the run's sigma form is either)
    assert np.array_equal(got == 0, lim == 0) and (np.abs(got - lim) <= tol * got).all()
    med = np.median(lim[(lim > 0) & (mask == 0)])
    assert R.hval(h, 'LIMEFLUX') == pytest.approx(med / 60.0, rel=0.05)


def test_cli_zeropoint_gives_magnitudes(cli_case):
    from blackbox_amd import fitsio
    c = cli_case
    c['cli'].main(c['common'] + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'zp'), '--limmag', 'True', '--zeropoint', '22.5'])
    lim = fitsio.read_image(str(c['tmp'] / 'on' / (RED % 0)) + '_limmag.fits')
    mag, hm = fitsio.read_image(str(c['tmp'] / 'zp' / (RED % 0)) + '_limmag.fits', get_header=True)
    ok = lim > 0
    assert R.hval(hm, 'LIMUNIT') == 'mag' and mag.dtype == F and np.array_equal(mag == 0, ~ok)
    np.testing.assert_allclose(mag[ok], 22.5 - 2.5 * np.log10(lim[ok] / 60.0), rtol=0, atol=2e-5)
    h = fitsio.read_hdus(str(c['tmp'] / 'zp' / (RED % 0)) + '_hdr.fits')[0][0]
    eflux, m, fnu = R.hval(h, 'LIMEFLUX'), R.hval(h, 'LIMMAG'), R.hval(h, 'LIMFNU')
    assert m == pytest.approx(22.5 - 2.5 * np.log10(eflux), abs=1e-9) and fnu == pytest.approx(10 ** (-0.4 * (m - 23.9)), rel=1e-9)


def _fits_equal(a, b):
    from blackbox_amd import fitsio
    ha, hb = fitsio.read_hdus(a), fitsio.read_hdus(b)
    assert len(ha) == len(hb), a
    for (h1, d1), (h2, d2) in zip(ha, hb):
        k1 = {k: (v if isinstance(v, np.ndarray) else R.hval(h1, k)) for k, v in h1.items() if k != 'BB-START'}
        k2 = {k: (v if isinstance(v, np.ndarray) else R.hval(h2, k)) for k, v in h2.items() if k != 'BB-START'}
        assert sorted(k1) == sorted(k2), (a, set(k1) ^ set(k2))
        for k in k1:
            if isinstance(k1[k], np.ndarray):
                assert np.array_equal(k1[k], k2[k]), (a, k)
            else:
                assert k1[k] == k2[k] or (k1[k] != k1[k] and k2[k] != k2[k]), (a, k, k1[k], k2[k])
        if d1 is None or d2 is None:
            assert d1 is None and d2 is None, a
        elif isinstance(d1, dict):
            assert list(d1) == list(d2), a
            for k in d1:
                assert np.array_equal(np.asarray(d1[k]), np.asarray(d2[k]), equal_nan=np.asarray(d1[k]).dtype.kind == 'f'), (a, k)
        else:
            d1, d2 = np.asarray(d1), np.asarray(d2)
            assert d1.dtype == d2.dtype and d1.tobytes() == d2.tobytes(), a


def test_cli_switch_off_changes_nothing(cli_case):
    """--limmag False against a run that never heard of the switch: the same files with the same contents (but for the time stamp
    BB-START and the log), no _limmag file, no LIM* key; and the switch-on run's other products are these too"""
    from blackbox_amd import fitsio
    c = cli_case
    c['cli'].main(c['common'] + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'off'), '--limmag', 'False'])
    c['cli'].main(c['common'] + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'unset')])
    off, unset, on = (sorted(os.listdir(str(c['tmp'] / d))) for d in ('off', 'unset', 'on'))
    assert off == unset and not any('limmag.fits' in f and '_trans_' not in f for f in off)
    assert sorted(set(on) - set(off)) == [(RED % 0) + '_limmag.fits']
    for f in off:
        if f.endswith('.fits'):
            _fits_equal(str(c['tmp'] / 'off' / f), str(c['tmp'] / 'unset' / f))
            for h, _ in fitsio.read_hdus(str(c['tmp'] / 'off' / f)):
                assert not any(k.startswith('LIM') for k in h) or '_trans_limmag' in f, f
    # the pixels of every image of the switch-on run are those of the switch-off run
    for f in off:
        if f.endswith('.fits') and not f.endswith(('_hdr.fits', '_cat.fits', '_trans.fits')):
            assert np.array_equal(fitsio.read_image(str(c['tmp'] / 'on' / f)), fitsio.read_image(str(c['tmp'] / 'off' / f)), equal_nan=True), f


def test_cli_image_list_with_fpack(ctx, cli_case):
    """--image_list with --fpack True: _red_limmag.fits.fz, which decodes to the serial run's image within the quantisation step of
    its row (q = 2: ZSCALE), and the serial run's keys"""
    from blackbox_amd import fitsio, fpack as P
    c = cli_case
    lst = str(c['tmp'] / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(c['raws']) + '\n')
    outs = c['cli'].main(c['common'] + ['--image_list', lst, '--red_dir', str(c['tmp'] / 'lst'), '--limmag', 'True', '--fpack', 'True'])
    assert len(outs) == 2 and all(outs)
    lim = fitsio.read_image(str(c['tmp'] / 'on' / (RED % 0)) + '_limmag.fits')
    h_on = fitsio.read_hdus(str(c['tmp'] / 'on' / (RED % 0)) + '_hdr.fits')[0][0]
    for k in range(2):
        name = str(c['tmp'] / 'lst' / (RED % k)) + '_limmag.fits.fz'
        assert os.path.isfile(name), name
        parts = P.funpack_read(name)
        _, h, table, _ = parts
        lay = P._table_layout(h)
        tb = np.ascontiguousarray(table).reshape(lim.shape[0], -1)
        step = np.ascontiguousarray(tb[:, lay['ZSCALE'][0]:lay['ZSCALE'][0] + 8]).view('>f8').astype(np.float64).reshape(-1)
        assert R.hval(h, 'LIMUNIT') == 'e-' and R.hval(h, 'LIMMAG-P') is True
        got = P.funpack_decode(ctx, parts)[0].cpu().numpy()
        assert got.shape == lim.shape
        assert (np.abs(got.astype(np.float64) - lim) <= step[:, None] * (1 + 1e-6) + 1e-6 * lim).all(), k
        hk = fitsio.read_hdus(str(c['tmp'] / 'lst' / (RED % k)) + '_hdr.fits')[0][0]
        assert [R.hval(hk, s) for s in LIMKEYS] == [R.hval(h_on, s) for s in LIMKEYS], k


def test_cli_the_switch_alone(cli_case, monkeypatch):
    """--limmag True without --cat_extract and --trans_extract: the image and the keys, no catalogue; and the same from
    settings.limmag with no switch on the command line"""
    from blackbox_amd import fitsio, settings
    c = cli_case
    alone = [a for a in c['nopsf'] if a not in ('--cat_extract', 'True')] + ['--psf_new', str(c['tmp'] / 'psf.fits')]
    assert '--cat_extract' not in alone and '--trans_extract' not in alone and '--telescope' in alone
    c['cli'].main(alone + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'alone'), '--limmag', 'True'])
    monkeypatch.setattr(settings, 'limmag', True)
    c['cli'].main(alone + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'byset')])
    monkeypatch.undo()
    want = fitsio.read_image(str(c['tmp'] / 'on' / (RED % 0)) + '_limmag.fits')
    h_on = fitsio.read_hdus(str(c['tmp'] / 'on' / (RED % 0)) + '_hdr.fits')[0][0]
    for d in ('alone', 'byset'):
        base = str(c['tmp'] / d / (RED % 0))
        assert not os.path.exists(base + '_cat.fits') and not os.path.exists(base + '_D.fits'), d
        assert np.array_equal(fitsio.read_image(base + '_limmag.fits'), want), d
        h = fitsio.read_hdus(base + '_hdr.fits')[0][0]
        assert [R.hval(h, s) for s in LIMKEYS] == [R.hval(h_on, s) for s in LIMKEYS], d


def test_cli_without_a_psf(cli_case):
    from blackbox_amd import fitsio
    c = cli_case
    c['cli'].main(c['nopsf'] + ['--image', c['raws'][0], '--red_dir', str(c['tmp'] / 'nopsf'), '--limmag', 'True'])
    base = str(c['tmp'] / 'nopsf' / (RED % 0))
    assert os.path.isfile(base + '.fits') and not os.path.exists(base + '_limmag.fits')
    h = fitsio.read_hdus(base + '_hdr.fits')[0][0]
    assert R.hval(h, 'LIMMAG-P') is False and all(R.hval(h, k) == 'None' for k in LIMKEYS[1:])
