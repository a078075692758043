"""GPU: optimal_subtraction with a reference of ANOTHER SHAPE brought to the new frame by a caller's ref_grid -- the path the
registration from the stars rides on: coadd.resample of the reference, remap_mini(shape_out=) of its sigma mini
image.  The toy scene of test_align_host.py: new frame 240 x 480, reference 320 x 600 seen through a shift, a rotation of 0.2
degrees and a scale; the grid is the scene's true transform.  Once without the star match and once with it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import test_align_host as A                   # noqa: E402
import test_match_host as H                   # noqa: E402
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402

F = np.float32
BORDER, BOX = 12, 20


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def scene():
    return A.make_align_scene()


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def inputs(ctx, sc):
    new = dev(ctx, sc['new'] + F(300.0))
    new_mask = torch.zeros(new.shape, dtype=torch.uint8, device=ctx.device)
    ref = dev(ctx, sc['ref'])
    kw = dict(ref_mask=torch.zeros(ref.shape, dtype=torch.uint8, device=ctx.device), psf_new=dev(ctx, sc['psf_new']),
              psf_ref=dev(ctx, sc['psf_ref']), subimage_size=H.SIZE, subimage_border=BORDER, bkg_boxsize=BOX, ref_is_bkgsub=True,
              ref_bkg_std_mini=np.full((A.RNY // BOX, A.RNX // BOX), H.SKY_REF, F))
    return new, new_mask, ref, kw


@pytest.mark.parametrize('match', [False, True])
def test_subtraction_through_a_callers_grid(ctx, scene, match):
    new, new_mask, ref, kw = inputs(ctx, scene)
    grid = A.grid_of(A.true_coef(), (A.NY, A.NX))
    res = G.optimal_subtraction(ctx, new, ref, new_mask, ref_grid=grid, match=match, **kw)
    ctx.sync()
    D, Scorr, rw = res['D'].cpu().numpy(), res['Scorr'].cpu().numpy(), res['ref_bkgsub'].cpu().numpy()
    assert D.shape == (A.NY, A.NX) and rw.shape == (A.NY, A.NX) and res['bkg_std_mini_ref'].shape == (A.RNY // BOX, A.RNX // BOX)
    assert np.isfinite(D).all() and np.isfinite(Scorr).all() and np.isfinite(rw).all()
    # where the reference covers the new frame its stars subtract: the scene's stars there leave far less in D than they hold in
    # the new frame; where it does not, the resampled reference is 0
    edge = A.remap_mask_ref(None, (A.RNY, A.RNX), grid, (A.NY, A.NX))[0] != 0
    assert edge.any() and not edge.all() and not rw[edge].any()
    st = scene['stars']
    py, px = np.rint(st['ny']).astype(int), np.rint(st['nx']).astype(int)
    on = (py >= 4) & (py < A.NY - 4) & (px >= 4) & (px < A.NX - 4)
    py, px = py[on], px[on]
    cov = ~np.array([edge[y - 4:y + 5, x - 4:x + 5].any() for y, x in zip(py, px)])
    bare = np.array([edge[y - 4:y + 5, x - 4:x + 5].all() for y, x in zip(py, px)])

    def per_star(sel):
        return sum(np.abs(D[y - 3:y + 4, x - 3:x + 4]).sum() for y, x in zip(py[sel], px[sel])) / sel.sum()
    r_cov, r_bare = per_star(cov), per_star(bare)
    print('match %s: sum |D| per star %.4g under the reference (%d stars), %.4g where there is none (%d stars); %d transient candidates, '
          '%d of them under the reference' % (match, r_cov, cov.sum(), r_bare, bare.sum(), len(res['transients']),
                                              sum(1 for t in res['transients'] if not edge[t['y'], t['x']])))
    assert cov.sum() > 50 and bare.sum() > 10 and r_cov < 0.5 * r_bare
    if match:
        m = res['match']
        print('pairs %d of %d new / %d reference sources, success %s' % (m['n_pairs'], m['n_new'], m['n_ref'], m['success']))
        assert m['n_pairs'] >= 50 and m['success']
    else:
        assert 'match' not in res
