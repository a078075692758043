"""GPU: the number of host waits of one optimal_subtraction call, per switch group, on two small scenes: the 80 x 320 scene of
test_gpu_subtraction.test_optimal_subtraction_chain (sub-images of 40 + 2 x 6 = 52 px: the rocFFT path) and a 96 x 144 frame with
sub-images of 48 + 2 x 8 = 64 px (the hand-written path).  A wait is one _lib.fetch (WAIT_STATS[1]); a stage that is moved
must neither add one nor split a copy back in two."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

from blackbox_amd import _lib                # noqa: E402
from blackbox_amd import reduce as R        # noqa: E402
from blackbox_amd import zogy as G          # noqa: E402

F = np.float32

SCENES = {
    # name: size, border, box, sub-images (y, x), PSF side, stars, transients (one on a tile seam), masked rows / box, seed
    'rocfft': dict(size=40, border=6, box=20, nsy=2, nsx=8, S=15, nstars=25, trans=[(30, 45, 4.0e4), (62, 170, 2.5e4), (40, 120, 6.0e4)],
                   bad=(slice(5, 9), slice(200, 230)), dead=(slice(0, 20), slice(300, 320)), seed=8),
    'frame': dict(size=48, border=8, box=6, nsy=2, nsx=3, S=15, nstars=30, trans=[(30, 45, 4.0e4), (62, 100, 2.5e4), (48, 96, 6.0e4)],
                  bad=(slice(5, 9), slice(100, 130)), dead=(slice(0, 6), slice(120, 144)), seed=8),
}

CONFIGS = {
    'defaults': dict(),
    'new_only_cat': dict(new_only=True, cat_extract=True),
    'catalogue_extras': dict(cat_extract=True, shapes=True, phot_centroid=True, aper_phot=True, limmag=True, match=True),
    'limmag_alone': dict(limmag=True),
    'transient_extras': dict(trans_psffit=True, trans_shapefit=True, thumbnails=True, thumbnail_pngs=True, thumbnail_size=16, fake_stars=1,
                             trans_fit_size=5),                        # (the fit's window: at most the PSF stamp's side - 10),
}

# host waits of one call, MEASURED ON THE PARENT COMMIT of the change that made _optimal_subtraction a list of stage functions
# (one body of 700 lines then): the stage functions must reproduce them
WAITS = {
    ('rocfft', 'defaults'): 4, ('rocfft', 'new_only_cat'): 4, ('rocfft', 'catalogue_extras'): 10,
    ('rocfft', 'limmag_alone'): 5, ('rocfft', 'transient_extras'): 4,
    ('frame', 'defaults'): 4, ('frame', 'new_only_cat'): 4, ('frame', 'catalogue_extras'): 10,
    ('frame', 'limmag_alone'): 5, ('frame', 'transient_extras'): 4,
}


def moffat_stamp(S, fwhm):
    a = fwhm / (2 * np.sqrt(2 ** (1 / 2.5) - 1))
    y, x = np.mgrid[0:S, 0:S] - S // 2
    p = (1 + (y * y + x * x) / (a * a)) ** -2.5
    return (p / p.sum()).astype(F)


def make_scene(size, border, box, nsy, nsx, S, nstars, trans, bad, dead, seed):
    """a static field seen with two PSFs, transients only in the new frame (test_optimal_subtraction_chain's, with its numbers
    for the 'rocfft' entry) -> host arrays and the geometry keywords"""
    rs = np.random.RandomState(seed)
    ny, nx = nsy * size, nsx * size
    pn, pr = moffat_stamp(S, 3.6), moffat_stamp(S, 3.0)
    truth = np.zeros((ny, nx))
    stars = []
    for _ in range(nstars):
        y, x = rs.randint(10, ny - 10), rs.randint(10, nx - 10)
        truth[y, x] += rs.uniform(3e3, 3e4)
        stars.append((y, x))
    tnew = truth.copy()
    for y, x, f in trans:
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
    mask_n = np.zeros((ny, nx), np.uint8); mask_n[bad] = 1
    mask_n[dead] = 32                                                    # a fully masked box -> NaN -> filled
    nsub = nsy * nsx
    return dict(new=new, ref=ref, mask_new=mask_n, mask_ref=np.zeros((ny, nx), np.uint8), psf_new=np.repeat(pn[None], nsub, 0),
                psf_ref=np.repeat(pr[None], nsub, 0), stars=np.asarray(stars), shape=(ny, nx),
                kw=dict(fratio=1.0, dx=0.03, dy=0.02, subimage_size=size, subimage_border=border, bkg_boxsize=box))


def call(ctx, sc, new_only=False, **switches):
    """one optimal_subtraction call on the scene -> (result, host waits it took)"""
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(ctx.device) for k in ('new', 'ref', 'mask_new', 'mask_ref', 'psf_new', 'psf_ref')}
    if new_only:
        d['ref'] = d['mask_ref'] = d['psf_ref'] = None
    ctx.sync()
    n0 = _lib.WAIT_STATS[1]
    res = G.optimal_subtraction(ctx, d['new'], d['ref'], d['mask_new'], d['mask_ref'], d['psf_new'], d['psf_ref'], **dict(sc['kw'], **switches))
    waits = _lib.WAIT_STATS[1] - n0
    ctx.sync()
    return res, waits


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def scenes():
    return {name: make_scene(**s) for name, s in SCENES.items()}


@pytest.mark.parametrize('config', sorted(CONFIGS))
@pytest.mark.parametrize('scene', sorted(SCENES))
def test_host_waits_of_one_call(ctx, scenes, scene, config):
    sc = scenes[scene]
    L = sc['kw']['subimage_size'] + 2 * sc['kw']['subimage_border']
    assert G.frame_path_supported(L) == (scene == 'frame')
    res, waits = call(ctx, sc, **CONFIGS[config])
    print('%s / %s: %d host waits (parent commit: %s)' % (scene, config, waits, WAITS[scene, config]))
    # the call took the path it was made for: subtracted or not, and every stage that was asked for ran to its end
    assert res['header_new']['Z-P'][0] is (config != 'new_only_cat')
    ran = dict(catalogue_extras=('AP-P', 'LIMMAG-P', 'PHOT-CEN'), limmag_alone=('LIMMAG-P',), transient_extras=('T-FKP', 'T-PSFD', 'T-SHAPE'))
    assert all(res['header'][k] is True for k in ran.get(config, ()))
    if config == 'catalogue_extras':
        assert 'match' in res and 'shapes' in res and len(res['catalog']['X_POS']) > 10
    if config == 'transient_extras':
        assert len(res['transients']) >= 2 and res['thumbnail_png8'].shape[0] == len(res['transients'])
    assert waits == WAITS[scene, config]
