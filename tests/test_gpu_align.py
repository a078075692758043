"""GPU: registration of the reference on the new frame from the two star lists (bbx_align.hip; include/bbx.h: bbx_align_vote,
bbx_align_fit, bbx_align_apply, bbx_align_grid, bbx_remap_mask) against the float64 numpy restatements of test_align_host.py,
kernel by kernel at small shapes; zogy.RefStars and zogy.align_reference on that file's scene; optimal_subtraction(ref_align=True)
and the command line with the switch on.

The fit's kept sets can differ from the restatement's only for a pair at the clip bound (the sums are taken in another order than
BLAS takes them).  Over every pass of every case below the pair nearest the bound is 0.0095 of the bound away from it
(clip_margin, printed and asserted > 1e-6): no pair is excluded from the comparison."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import test_align_host as A                   # noqa: E402  (the restatements and the scene)
import test_match_host as H                   # noqa: E402
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402
from blackbox_amd._lib import lib             # noqa: E402

F = np.float32
SHAPE = (A.NY, A.NX)
BORDER, BOX = 12, 20


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def scene():
    """the toy scene and its two host catalogues (the reference's on its own grid)"""
    sc = A.make_align_scene()
    a = H.host_catalog(sc['new'], H.SKY_NEW, sc['psf_new'])
    b = H.host_catalog(sc['ref'], H.SKY_REF, sc['psf_ref'])
    return sc, a, b


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def dev_list(ctx, lst):
    n = len(lst[0])
    cols = [np.asarray(lst[0], np.int32), np.asarray(lst[1], np.int32), np.asarray(lst[2], F).reshape(n, 2)]
    cols += [np.asarray(t, F) for t in lst[3:5]]
    return tuple(dev(ctx, c) for c in cols)


def host(ctx, *tensors):
    ctx.sync()
    out = [t.cpu().numpy() for t in tensors]
    return out if len(out) > 1 else out[0]


EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), F), np.zeros(0, F), np.zeros(0, F))


# ---- vote ----------------------------------------------------------------------------------------------------------
def odd_list():
    """list_case() with a NaN offset, a zero flux, and two equal fluxes among the brightest"""
    a, b, _, _ = A.list_case()
    a = [np.array(t) for t in a]
    a[2][3, 1] = np.nan
    a[3][5] = 0.0
    a[3][7] = a[3][8] = a[3].max()
    return tuple(a), b


def vote_case(name, scene):
    if name == 'scene':
        return scene[1], scene[2], {}
    if name == 'list':
        return A.list_case()[:2] + ({},)
    if name == 'wrong':
        return A.list_case(wrong=0.10)[:2] + ({},)
    if name == 'unrelated':
        return A.list_case(seed=21)[0], A.list_case(seed=22)[1], {}
    if name == 'few':
        return A.list_case(n=60)[:2] + ({},)
    if name == 'empty_a':
        return EMPTY, A.list_case()[1], {}
    if name == 'empty_b':
        return A.list_case()[0], EMPTY, {}
    if name == 'cap':
        return A.list_case()[:2] + (dict(cap=64),)
    if name == 'nbright':
        return A.list_case()[:2] + (dict(nbright=100),)
    if name == 'odd':
        return odd_list() + (dict(nbright=100),)
    raise KeyError(name)


@pytest.mark.parametrize('name', ['scene', 'list', 'wrong', 'unrelated', 'few', 'empty_a', 'empty_b', 'cap', 'nbright', 'odd'])
def test_vote_equals_the_restatement(ctx, scene, name):
    a, b, kw = vote_case(name, scene)
    want = A.vote_ref(a, b, **kw)
    da, db = dev_list(ctx, a), dev_list(ctx, b)
    info, coarse, pairs = host(ctx, *G.align_vote(ctx, da, db, **kw))
    info2, coarse2, pairs2 = host(ctx, *G.align_vote(ctx, da, db, **kw))
    n = int(info[4])
    print('%s: %d x %d sources; info gpu %s restatement %s; coarse gpu %s restatement %s'
          % (name, len(a[0]), len(b[0]), info.tolist(), want['info'].tolist(), coarse.tolist(), list(want['coarse'])))
    assert np.array_equal(info, want['info'])
    assert n == len(want['pairs']) and np.array_equal(pairs[:n], want['pairs']) and (pairs[n:] == -1).all()
    assert np.array_equal(coarse, np.asarray(want['coarse'], np.float64), equal_nan=True)
    assert info.tobytes() == info2.tobytes() and coarse.tobytes() == coarse2.tobytes() and pairs.tobytes() == pairs2.tobytes()
    if name in ('unrelated', 'few', 'empty_a', 'empty_b'):
        assert info[5] == 1
    if name in ('scene', 'list', 'wrong', 'nbright', 'odd'):
        assert info[5] == 0
    if name == 'cap':
        assert info[4] == 64 and info[6] > 64


def test_vote_arguments(ctx):
    t = torch.zeros(64, dtype=torch.float32, device=ctx.device)
    p = t.data_ptr()
    assert lib.bbx_align_vote_bytes(2049, 256.0, 4.0, 8192) == 0 and lib.bbx_align_vote_bytes(2048, 256.0, 4.0, 8193) == 0
    assert lib.bbx_align_vote_bytes(2048, 256.0, 0.0, 8192) == 0 and lib.bbx_align_vote_bytes(2048, 256.0, 4.0, 8192) > 66564
    # a scratch buffer that is too small, a list without its columns
    assert lib.bbx_align_vote(ctx.h, 0, None, None, None, None, 0, None, None, None, None, 2048, 256.0, 4.0, 15, 8, 8192, p, 256, p, p, p, None) == -1
    assert lib.bbx_align_vote(ctx.h, 5, None, None, None, None, 0, None, None, None, None, 2048, 256.0, 4.0, 15, 8, 8192, p, 1 << 20, p, p, p, None) == -1
    with pytest.raises(ValueError):
        G.align_vote(ctx, dev_list(ctx, EMPTY), dev_list(ctx, EMPTY), nbright=4096)
    a = list(dev_list(ctx, A.list_case()[0]))
    a[3] = a[3][:-1].contiguous()                                    # a flux column one short
    with pytest.raises(ValueError):
        G.align_vote(ctx, tuple(a), dev_list(ctx, EMPTY))


# ---- fit -----------------------------------------------------------------------------------------------------------
def clip_margin(a, b, items, shape, poldeg, snr_min=A.SNR_MIN, clip=A.CLIP, nmin=A.NMIN):
    """smallest relative distance of a kept pair's r^2 from the clip bound over the clipping passes of fit_ref (inf: no pass)"""
    items = np.asarray(items, np.int64).reshape(-1, 2)
    nc = 6 if poldeg == 2 else 3
    ia, ib = items[:, 0], items[:, 1]
    valid = (ia >= 0) & (ib >= 0)
    ia, ib = np.where(valid, ia, 0), np.where(valid, ib, 0)
    if not len(a[0]) or not len(b[0]):
        return np.inf
    ao, bo = np.asarray(a[2], F).reshape(-1, 2)[ia], np.asarray(b[2], F).reshape(-1, 2)[ib]
    fa, ea, fb, eb = [np.asarray(t, F)[i] for t, i in ((a[3], ia), (a[4], ia), (b[3], ib), (b[4], ib))]
    with np.errstate(all='ignore'):
        q = valid & (fa > 0) & (fb > 0) & (fa / ea >= F(snr_min)) & (fb / eb >= F(snr_min)) & np.isfinite(ao).all(axis=1) & np.isfinite(bo).all(axis=1)
    ao, bo = np.where(q[:, None], ao, 0), np.where(q[:, None], bo, 0)
    B = A.basis(shape, np.asarray(a[1])[ia] + ao[:, 1].astype(np.float64), np.asarray(a[0])[ia] + ao[:, 0].astype(np.float64))[:, :nc]
    X, Y = np.asarray(b[1])[ib] + bo[:, 1].astype(np.float64), np.asarray(b[0])[ib] + bo[:, 0].astype(np.float64)
    kept, best = q.copy(), np.inf
    for p in range(3):
        n = int(kept.sum())
        if n < max(nmin, nc):
            break
        Lm = A.cholesky_ref(B[kept].T @ B[kept])
        if Lm is None:
            break
        c = [np.linalg.solve(Lm.T, np.linalg.solve(Lm, B[kept].T @ t[kept])) for t in (X, Y)]
        r2 = (X - B @ c[0]) ** 2 + (Y - B @ c[1]) ** 2
        lim = clip * clip * (r2[kept].sum() / n)
        best = min(best, np.abs(r2[kept] / lim - 1).min())
        kept = kept & (r2 <= lim)
    return best


def collinear_case():
    n = 40
    a = A.lists_of(np.full(n, 100.0), np.linspace(20, 400, n), np.full(n, 1e4), SHAPE)
    return a, a, np.stack([np.arange(n), np.arange(n)], axis=1)


@pytest.fixture(scope='module')
def fit_cases(scene):
    """name -> (a, b, items): the vote's pairs and the items of the first match round of the restatement, per list pair"""
    cases = {}
    for name, (a, b) in (('scene', scene[1:]), ('list', A.list_case()[:2]), ('wrong', A.list_case(wrong=0.10)[:2])):
        trace = []
        A.align_ref(a, b, SHAPE, 1, trace=trace)
        cases[name + '_vote'] = (a, b, trace[0][0])
        cases[name + '_round'] = (a, b, trace[1][0])
    cases['mirror'] = A.mirror_case()
    cases['collinear'] = collinear_case()
    a, b, _, _ = A.list_case(n=60)
    cases['few'] = (a, b, np.stack([np.arange(len(a[0])), np.arange(len(a[0])) % max(len(b[0]), 1)], axis=1))
    cases['empty'] = (EMPTY, A.list_case()[1], np.zeros((4, 2), np.int32))
    return cases


@pytest.mark.parametrize('poldeg', [1, 2])
@pytest.mark.parametrize('name', ['scene_vote', 'scene_round', 'list_vote', 'list_round', 'wrong_vote', 'wrong_round', 'mirror', 'collinear',
                                  'few', 'empty'])
def test_fit_meets_the_restatement(ctx, fit_cases, name, poldeg):
    a, b, items = fit_cases[name]
    want = A.fit_ref(a, b, items, SHAPE, poldeg)
    margin = clip_margin(a, b, items, SHAPE, poldeg)
    coef, stats, kept = host(ctx, *G.align_fit(ctx, dev_list(ctx, a), dev_list(ctx, b), dev(ctx, np.asarray(items, np.int32).reshape(-1, 2)),
                                               SHAPE, poldeg))
    print('%s degree %d: %d items; flags gpu %d restatement %d, n_used %d / %d, rms gpu (%.6f, %.6f) restatement (%.6f, %.6f), '
          'nearest pair to the clip bound %.3g' % (name, poldeg, len(items), stats[3], want['flags'], stats[0], want['n_used'], stats[1],
                                                   stats[2], want['rms_x'], want['rms_y'], margin))
    assert margin > 1e-6
    assert int(stats[3]) == want['flags'] and int(stats[0]) == want['n_used']
    assert np.array_equal(kept.astype(bool), want['kept'])
    assert np.array_equal(np.isfinite(coef), np.isfinite(want['coef']))
    if np.isfinite(want['coef']).all():
        err = A.corner_errors(coef, want['coef'])
        print('    corners differ by %s px' % err.tolist())
        assert (err <= 1e-9).all()
        assert abs(stats[1] - want['rms_x']) <= 1e-9 and abs(stats[2] - want['rms_y']) <= 1e-9
    if name == 'mirror' and poldeg == 1:
        assert want['flags'] == 8
    if name == 'collinear':
        assert want['flags'] & 4
    if name in ('few', 'empty'):
        assert want['flags'] & 2


def test_fit_arguments(ctx):
    a, b = dev_list(ctx, A.list_case()[0]), dev_list(ctx, A.list_case()[1])
    items = torch.zeros((4, 2), dtype=torch.int32, device=ctx.device)
    with pytest.raises(ValueError):
        G.align_fit(ctx, a, b, items, SHAPE, 3)
    with pytest.raises(ValueError):
        G.align_fit(ctx, a, b, items.to(torch.int64), SHAPE, 1)
    with pytest.raises(ValueError):
        G.align_fit(ctx, a, b[:3] + (b[3][:-1].contiguous(), b[4]), items, SHAPE, 1)
    # indices past the lists are no pairs, not reads
    wild = dev(ctx, np.array([[0, 10 ** 6], [10 ** 6, 0], [-5, 2], [1, 1]], np.int32))
    _, stats, kept = host(ctx, *G.align_fit(ctx, a, b, wild, SHAPE, 1))
    assert kept.tolist() == [0, 0, 0, 1] and int(stats[3]) == 2
    p = items.data_ptr()
    assert lib.bbx_align_fit(ctx.h, 5, None, None, None, None, None, 0, None, None, None, None, None, 4, p, 240, 480, 1, 20.0, 3.0, 15, p, p, p,
                             None) == -1


# ---- apply ---------------------------------------------------------------------------------------------------------
def quad_coef():
    c = A.true_coef()
    c[3:6] = 0.31, -0.22, 0.12
    c[9:12] = -0.17, 0.26, 0.21
    return c


APPLY_COEFS = {'true': (A.true_coef(), 1), 'quad': (quad_coef(), 2), 'true_as_2': (A.true_coef(), 2),
               'det0': (np.array([200.0, 100, 50, 0, 0, 0, 140, 200, 100, 0, 0, 0]), 1),
               'far': (np.array([200.0, 1e-12, 0, 0, 0, 0, 140, 0, 1e-12, 0, 0, 0]), 1),
               'far_2': (np.array([200.0, 1e-12, 0, 0.1, 0, 0, 140, 0, 1e-12, 0, 0, 0.1]), 2)}


@pytest.mark.parametrize('name', sorted(APPLY_COEFS))
def test_apply_meets_the_restatement(ctx, scene, name):
    coef, poldeg = APPLY_COEFS[name]
    for b in (scene[2], A.list_case()[1]):
        want = A.apply_ref(b[:3], coef, SHAPE, poldeg)
        got = host(ctx, *G.align_apply(ctx, dev_list(ctx, b)[:3], dev(ctx, coef), SHAPE, poldeg))
        nan = np.isnan(want[2])
        same = (got[2].view(np.uint32) == want[2].view(np.uint32)).all(axis=1)
        print('%s degree %d: %d sources, %d without a position; %d offsets bit-equal' % (name, poldeg, len(b[0]), nan[:, 0].sum(), same.sum()))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(np.isnan(got[2]), nan)
        if (~nan).any():
            assert np.abs(got[2] - want[2])[~nan].max() <= 1e-6
        if name in ('det0', 'far'):
            assert nan.all()
        elif name != 'far_2':
            assert np.array_equal(nan.any(axis=1), np.isnan(np.asarray(b[2])).any(axis=1))       # only the sources without a centroid
    # the sort that follows: (y, x) order of the integer peak, stable, with the permutation
    ys, xs, off = got
    sy, sx, so, perm = host(ctx, *G.align_sort(*[dev(ctx, t) for t in got]))
    wy, wx, wo, wp = A.sort_ref(ys, xs, off)
    assert np.array_equal(sy, wy) and np.array_equal(sx, wx) and np.array_equal(so, wo, equal_nan=True) and np.array_equal(perm, wp)


def test_apply_arguments(ctx):
    b = dev_list(ctx, A.list_case()[1])[:3]
    coef = dev(ctx, A.true_coef())
    with pytest.raises(ValueError):
        G.align_apply(ctx, b, coef[:6].contiguous(), SHAPE, 1)
    with pytest.raises(ValueError):
        G.align_apply(ctx, b, coef, SHAPE, 0)
    with pytest.raises(ValueError):
        G.align_apply(ctx, (b[0], b[1], b[2][:-1].contiguous()), coef, SHAPE, 1)
    e = dev_list(ctx, EMPTY)[:3]
    assert G.align_apply(ctx, e, coef, SHAPE, 1)[0].numel() == 0


# ---- grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(240, 480), (67, 93)])
@pytest.mark.parametrize('which', ['true', 'quad'])
def test_grid_meets_the_restatement(ctx, shape, which):
    coef = A.true_coef(shape) if which == 'true' else quad_coef()
    want = A.grid_of(coef, shape)
    got = host(ctx, G.align_grid(ctx, dev(ctx, coef), shape))
    assert got.shape == want.shape
    print('grid %s of %s: %s nodes, max |gpu - restatement| %.3g px' % (which, shape, got.shape[:2], np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-9
    p = dev(ctx, coef).data_ptr()
    assert lib.bbx_align_grid(ctx.h, p, shape[0], shape[1], 32, got.shape[0] - 1, got.shape[1], p, None) == -1       # one node short
    assert lib.bbx_align_grid(ctx.h, p, shape[0], shape[1], 0, got.shape[0], got.shape[1], p, None) == -1


# ---- the reference's mask on the new frame's grid -------------------------------------------------------------------
def small_mask(shape=(50, 81), seed=2):
    rs = np.random.RandomState(seed)
    return (rs.uniform(size=shape) < 0.05).astype(np.uint8) * rs.choice([1, 2, 4, 8, 16], size=shape).astype(np.uint8)


def remap_case(name):
    """-> (mask or None, in_shape, grid, out_shape)"""
    s = (50, 81)
    if name == 'identity':
        return small_mask(), s, A.shift_grid(s, 0, 0), s
    if name == 'integer':
        return small_mask(), s, A.shift_grid(s, 3, -5), s
    if name == 'fraction':
        return small_mask(), s, A.shift_grid(s, 0.25, 0.5), s
    if name == 'rotated':
        return small_mask(), s, A.grid_of(A.true_coef((67, 93), 0.7, 1.002, (24.3, 38.9)), (67, 93)), (67, 93)
    if name == 'scene':
        return small_mask((A.RNY, A.RNX), 3), (A.RNY, A.RNX), A.grid_of(A.true_coef(), SHAPE), SHAPE
    if name == 'four_sides':
        return small_mask(), s, A.shift_grid((120, 150), -30.4, -35.7), (120, 150)
    if name == 'nan_node':
        g = A.grid_of(A.true_coef((67, 93), 0.7, 1.002, (24.3, 38.9)), (67, 93))
        g[1, 1, 0] = np.nan
        return small_mask(), s, g, (67, 93)
    if name == 'no_mask':
        return None, s, A.grid_of(A.true_coef((67, 93), 0.7, 1.002, (24.3, 38.9)), (67, 93)), (67, 93)
    raise KeyError(name)


@pytest.mark.parametrize('name', ['identity', 'integer', 'fraction', 'rotated', 'scene', 'four_sides', 'nan_node', 'no_mask'])
def test_remap_mask_equals_the_restatement(ctx, name):
    mask, in_shape, grid, out_shape = remap_case(name)
    want, n_want = A.remap_mask_ref(mask, in_shape, grid, out_shape)
    out, nedge = host(ctx, *G.remap_mask(ctx, None if mask is None else dev(ctx, mask), in_shape, dev(ctx, grid), out_shape))
    print('%s: %s -> %s, %d edge pixels (restatement %d), %d pixels differ' % (name, in_shape, out_shape, nedge[0], n_want, (out != want).sum()))
    assert out.dtype == np.uint8 and out.shape == tuple(out_shape)
    assert np.array_equal(out, want) and int(nedge[0]) == n_want
    if name == 'identity':
        assert np.array_equal(out & ~np.uint8(A.EDGE), mask)
    if name == 'four_sides':
        e = (out & A.EDGE) != 0
        assert e[0].all() and e[-1].all() and e[:, 0].all() and e[:, -1].all() and not e.all()
    if name == 'nan_node':
        assert ((out & A.EDGE) != 0)[:64, :64].all()


def test_remap_mask_arguments(ctx):
    mask, in_shape, grid, out_shape = remap_case('rotated')
    d_grid = dev(ctx, grid)
    out = torch.zeros(out_shape, dtype=torch.uint8, device=ctx.device)
    n = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    gny, gnx = grid.shape[:2]
    call = lambda gy, gx, step: lib.bbx_remap_mask(ctx.h, in_shape[0], in_shape[1], None, out_shape[0], out_shape[1], d_grid.data_ptr(), gy, gx,   # noqa: E731
                                                   step, 32, out.data_ptr(), n.data_ptr(), None)
    assert call(gny, gnx, 32) == 0
    assert call(gny - 1, gnx, 32) == -1 and call(gny, gnx - 1, 32) == -1          # a lattice one node too short
    assert call(gny, gnx, 0) == -1
    ctx.sync()
    with pytest.raises(ValueError):
        G.remap_mask(ctx, dev(ctx, mask)[:-1].contiguous(), in_shape, d_grid, out_shape)
    with pytest.raises(ValueError):
        G.remap_mask(ctx, None, in_shape, d_grid.to(torch.float32), out_shape)
    with pytest.raises(G._lib_BBXError):
        G.remap_mask(ctx, None, in_shape, d_grid[:-1].contiguous(), out_shape)


# ---- RefStars and align_reference ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def device_catalogues(ctx, scene):
    """both frames' star lists made on the device, each on its own grid: the reference's 320 x 600 pixels are 2 x 5 tiles of
    120 and a strip of 80 rows whose peaks take the last tile row's PSF plane"""
    sc = scene[0]
    out = []
    for img, sky, psf in ((sc['new'], H.SKY_NEW, sc['psf_new']), (sc['ref'], H.SKY_REF, sc['psf_ref'])):
        d_img = dev(ctx, img)
        nsy, nsx = img.shape[0] // H.SIZE, img.shape[1] // H.SIZE
        stamps = G.subimage_psfs(ctx, dev(ctx, psf), nsy, nsx, H.SIZE)
        sigma = torch.full(d_img.shape, float(sky), dtype=torch.float32, device=ctx.device)
        out.append(G.RefStars(ctx, d_img, sigma, None, stamps, nsy, nsx, H.SIZE, cat_nsigma=H.CAT_NSIGMA, sigma_median=sky))
    ctx.sync()
    return out


def test_ref_stars_on_the_references_own_grid(ctx, scene, device_catalogues):
    _, _, b = scene
    rs = device_catalogues[1]
    ys, xs, off, flux, err = host(ctx, *rs.lists())
    print('reference: %d sources on the device, %d in the host catalogue; %d of them below row %d' % (rs.n, len(b[0]), (ys >= 240).sum(), 240))
    assert rs.n == len(b[0]) and np.array_equal(ys, b[0]) and np.array_equal(xs, b[1])
    assert (ys >= 2 * H.SIZE).sum() > 20                               # the strip below the last whole tile row holds sources
    assert np.nanmax(np.abs(off - b[2])) <= 2e-5 and np.array_equal(np.isnan(off), np.isnan(b[2]))
    assert np.allclose(flux, b[3], rtol=1e-4) and np.allclose(err, b[4], rtol=1e-4)
    assert rs.matches(rs.ref) and not rs.matches(rs.ref.clone())


@pytest.mark.parametrize('poldeg', [1, 2])
def test_align_reference_on_the_scene(ctx, scene, device_catalogues, poldeg):
    sc = scene[0]
    new_stars, ref_stars = device_catalogues
    mask = small_mask((A.RNY, A.RNX), 3)
    res = G.align_reference(ctx, new_stars.lists(), ref_stars, SHAPE, (A.RNY, A.RNX), dev(ctx, mask), poldeg=poldeg)
    a, b = host(ctx, *new_stars.lists()), host(ctx, *ref_stars.lists())
    want = A.align_ref(a, b, SHAPE, poldeg)
    fit = res['fit']
    err, bound = A.corner_errors(res['coef'], sc['coef']), A.corner_bound(fit, poldeg)
    chain = A.corner_errors(res['coef'], want['coef'])
    print('degree %d: flags %d, vote %s, n_used %d (restatement %d), rms (%.4f, %.4f); corner errors %s px, bound %.4f; against the '
          'restatement on the same lists %s px' % (poldeg, res['flags'], fit['info'].tolist(), fit['n_used'], want['n_used'], fit['rms_x'],
                                                   fit['rms_y'], np.round(err, 4).tolist(), bound, chain.tolist()))
    assert res['flags'] == 0 and want['flags'] == 0
    assert (err <= bound).all()
    assert (chain <= 1e-6).all() and fit['n_used'] == want['n_used']
    assert np.array_equal(fit['info'], want['vote']['info'])
    # the lattice and the mask are those of the fitted transform
    grid, out = host(ctx, res['grid'], res['mask'])
    assert np.abs(grid - A.grid_of(res['coef'], SHAPE)).max() <= 1e-9
    w_mask, w_n = A.remap_mask_ref(mask, (A.RNY, A.RNX), grid, SHAPE)
    assert np.array_equal(out, w_mask) and res['n_edge'] == w_n
    h = res['header']
    dy, dx, rot = A.true_shift()
    assert h['A-P'][0] is True and h['A-FLAGS'][0] == 0 and h['A-PLDG'][0] == poldeg and h['A-NEDGE'][0] == w_n
    assert abs(h['A-DX'][0] - dx) < 0.1 and abs(h['A-DY'][0] - dy) < 0.1 and abs(h['A-ROT'][0] - rot) < 0.02


def test_align_reference_refuses_unrelated_fields(ctx):
    a, b = dev_list(ctx, A.list_case(seed=21)[0]), dev_list(ctx, A.list_case(seed=22)[1])
    res = G.align_reference(ctx, a, b, SHAPE, (A.RNY, A.RNX), None)
    print('unrelated fields: flags %d, vote %s' % (res['flags'], res['fit']['info'].tolist()))
    assert res['flags'] & 1 and res['grid'] is None and res['mask'] is None and res['n_edge'] is None
    assert res['header']['A-P'][0] is False and res['header']['A-DX'][0] == 'None' and res['header']['A-FLAGS'][0] == res['flags']


# ---- optimal_subtraction(ref_align=True) ------------------------------------------------------------------------------
INJ_FLUX = 4000.0                # S/N of the PSF flux on the new frame's sky: 4000 / (14 sqrt(4 pi 1.53^2)) = 53 >= 15


def injected_scene():
    """the toy scene with six point sources in the new frame only, clear of the scene's stars: four where the reference covers
    the new frame, two where it does not"""
    sc = A.make_align_scene()
    edge = A.remap_mask_ref(None, (A.RNY, A.RNX), A.grid_of(A.true_coef(), SHAPE), SHAPE)[0] != 0
    st = sc['stars']
    on, off = [], []
    for y in range(30, A.NY - 30, 17):
        for x in range(30, A.NX - 30, 19):
            if np.hypot(st['ny'] - y, st['nx'] - x).min() < 14 or any(np.hypot(p[0] - y, p[1] - x) < 40 for p in on + off):
                continue
            win = edge[y - 12:y + 13, x - 12:x + 13]
            if not win.any() and len(on) < 4:
                on.append((y + 0.3, x - 0.2))
            elif edge[y - 6:y + 7, x - 6:x + 7].all() and len(off) < 2:
                off.append((y - 0.1, x + 0.4))
    assert len(on) == 4 and len(off) == 2
    pos = np.array(on + off)
    new = sc['new'] + H.render(A.NY, A.NX, pos[:, 0], pos[:, 1], np.full(6, INJ_FLUX), H.FWHM_NEW).astype(F)
    return dict(sc, new=new.astype(F), injected=pos, edge_true=edge)


def sub_inputs(ctx, sc, ref=None):
    new = dev(ctx, sc['new'] + F(300.0))
    new_mask = torch.zeros(new.shape, dtype=torch.uint8, device=ctx.device)
    ref = dev(ctx, sc['ref'] if ref is None else ref)
    kw = dict(ref_mask=torch.zeros(ref.shape, dtype=torch.uint8, device=ctx.device), psf_new=dev(ctx, sc['psf_new']),
              psf_ref=dev(ctx, sc['psf_ref']), subimage_size=H.SIZE, subimage_border=BORDER, bkg_boxsize=BOX, ref_is_bkgsub=True,
              ref_bkg_std_mini=np.full((A.RNY // BOX, A.RNX // BOX), H.SKY_REF, F), match=True)
    return new, new_mask, ref, kw


def near_any(y, x, pos, r=2.0):
    return bool(len(pos)) and np.hypot(pos[:, 0] - y, pos[:, 1] - x).min() <= r


@pytest.fixture(scope='module')
def e2e(ctx):
    sc = injected_scene()
    new, new_mask, ref, kw = sub_inputs(ctx, sc)
    n0 = G.RefStars.builds
    reg = G.optimal_subtraction(ctx, new, ref, new_mask, ref_align=True, **kw)
    ctx.sync()
    again = G.optimal_subtraction(ctx, new, ref, new_mask, ref_align=True, ref_stars=reg['ref_stars'], **kw)
    ctx.sync()
    builds = G.RefStars.builds - n0
    given = G.optimal_subtraction(ctx, new, ref, new_mask, ref_grid=A.grid_of(A.true_coef(), SHAPE), **kw)
    ctx.sync()
    return dict(sc=sc, reg=reg, again=again, given=given, builds=builds, inputs=(new, new_mask, ref, kw))


def test_subtraction_with_the_registration(ctx, e2e):
    sc, reg, given = e2e['sc'], e2e['reg'], e2e['given']
    ht = reg['header_trans']
    dy, dx, rot = A.true_shift()
    print('registered: %s' % {k: v[0] for k, v in ht.items() if k.startswith('A-') or k in ('T-NOFFR', 'T-NTRANS')})
    assert ht['A-P'][0] is True and ht['A-FLAGS'][0] == 0
    assert abs(ht['A-DX'][0] - dx) <= 0.1 and abs(ht['A-DY'][0] - dy) <= 0.1 and abs(ht['A-ROT'][0] - rot) <= 0.02
    assert sorted(k for k in ht if k.startswith('A-')) == sorted(['A-P', 'A-PLDG', 'A-NVOTE', 'A-NRUN', 'A-NFAR', 'A-NPAIR', 'A-RMSX', 'A-RMSY',
                                                                    'A-DX', 'A-DY', 'A-ROT', 'A-SCALE', 'A-FLAGS', 'A-NEDGE'])
    al = reg['align']
    grid, rmask = host(ctx, al['grid'], reg['ref_mask_remapped'])
    w_mask, w_n = A.remap_mask_ref(np.zeros((A.RNY, A.RNX), np.uint8), (A.RNY, A.RNX), grid, SHAPE)
    assert ht['A-NEDGE'][0] == w_n == al['n_edge'] and np.array_equal(rmask, w_mask)
    assert reg['D'].shape == SHAPE and reg['ref_bkgsub'].shape == SHAPE
    cand = np.array([(t['y'], t['x']) for t in reg['transients']]).reshape(-1, 2)
    inj = sc['injected']
    for y, x in inj[:4]:
        assert near_any(y, x, cand), (y, x)                          # the four under the reference are found
    assert not any(rmask[t['y'], t['x']] & A.EDGE for t in reg['transients'])
    assert ht['T-NOFFR'][0] >= 2 and ht['T-NTRANS'][0] == len(reg['transients']) + ht['T-NOFFR'][0]
    for y, x in inj[4:]:
        assert not near_any(y, x, cand)                              # ... and the two beside it are not candidates
    # spurious candidates against the same call with the scene's true lattice
    n_reg = sum(1 for t in reg['transients'] if not near_any(t['y'], t['x'], inj))
    n_giv = sum(1 for t in given['transients'] if not e2e['sc']['edge_true'][t['y'], t['x']] and not near_any(t['y'], t['x'], inj))
    print('candidates that are no injected source, under the reference: %d registered, %d with the true lattice (bound %d + %.1f)'
          % (n_reg, n_giv, n_giv, 3 * np.sqrt(n_giv) + 1))
    assert n_reg <= n_giv + 3 * np.sqrt(n_giv) + 1
    assert 'A-P' not in given['header_trans'] and 'T-NOFFR' not in given['header_trans'] and 'align' not in given
    # the reference's star list is made once and taken back
    assert e2e['builds'] == 1 and e2e['again']['ref_stars'] is reg['ref_stars']
    assert torch.equal(e2e['again']['D'], reg['D']) and e2e['again']['header_trans'] == ht


def test_a_reference_of_another_field_is_not_subtracted(ctx, e2e):
    sc = e2e['sc']
    other = A.make_align_scene(seed=9)['ref']
    new, new_mask, ref, kw = sub_inputs(ctx, sc, ref=other)
    res = G.optimal_subtraction(ctx, new, ref, new_mask, ref_align=True, cat_extract=True, **kw)
    ctx.sync()
    ht = res['header_trans']
    print('another field: %s' % {k: v[0] for k, v in ht.items() if k.startswith('A-')})
    assert ht['A-P'][0] is False and ht['A-DX'][0] == 'None' and res['align']['flags'] & 1
    assert 'D' not in res and res['transients'] == [] and res['header_new']['Z-P'][0] is False and 'match' not in res
    assert res['catalog'] is not None and len(res['catalog']['X_POS']) > 100      # the new frame's own products are there
    assert res['header_new']['A-P'][0] is False
    with pytest.raises(ValueError):
        G.optimal_subtraction(ctx, new, ref, new_mask, ref_align=True, ref_grid=A.grid_of(A.true_coef(), SHAPE), **kw)


# ---- command line ----------------------------------------------------------------------------------------------------
VOLATILE = ('BB-START',)


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = os.path.join(d, f)
    return out


def test_cli_registers_the_reference(tmp_path, ctx):
    import logging
    import bbx_oracle as O
    import test_gpu_operator as OP
    from blackbox_amd import fitsio, synth
    cli = OP.load_cli()
    case = synth.make_case(OP.YS, OP.XS, 77, tel=OP.TEL, os_y=20, os_x=45, n_stars=150, n_sat=2, n_cr=40)
    raw = str(tmp_path / 'ML1_raw0.fits')
    fitsio.write_image(raw, case['raw'], {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q', 'DATE-OBS': '2024-01-02T03:04:00'})
    fitsio.write_image(str(tmp_path / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp_path / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp_path / 'xtalk.dat'), case['xtalk'])
    d0 = R.reduce_object(ctx, dev(ctx, case['raw']), {}, OP.TEL, mflat=dev(ctx, case['flat']), bpm=dev(ctx, case['bpm']),
                         xtalk_coeffs=O.xtalk_coeffs(case['xtalk']), exptime=60.0, ysize_chan=OP.YS, xsize_chan=OP.XS,
                         log=logging.getLogger('t'))[0]
    rs = np.random.RandomState(3)
    # the reference: the reduced frame seen 4 rows down and 6 columns to the left, on a frame of another shape
    d0 = d0.cpu().numpy()
    ny, nx = d0.shape
    ref = rs.normal(0, 4, (ny + 30, nx + 60)).astype(F)
    ref[9:9 + ny, 1:1 + nx] += (d0 - 100.0).astype(F)                # new (y, x) -> ref (y + 9, x + 1): A-DY = -9, A-DX = -1
    fitsio.write_image(str(tmp_path / 'ref.fits'), ref)
    fitsio.write_image(str(tmp_path / 'psf.fits'), OP.moffat(15, 3.5))
    common = ['--telescope', OP.TEL, '--mflat', str(tmp_path / 'flat.fits'), '--bpm', str(tmp_path / 'bpm.fits'),
              '--crosstalk', str(tmp_path / 'xtalk.dat'), '--ysize_chan', str(OP.YS), '--xsize_chan', str(OP.XS),
              '--trans_extract', 'True', '--psf_new', str(tmp_path / 'psf.fits'), '--psf_ref', str(tmp_path / 'psf.fits'),
              '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30', '--image', raw]
    cli.main(common + ['--ref', str(tmp_path / 'ref.fits'), '--red_dir', str(tmp_path / 'on'), '--ref_align', 'True'])
    h = fitsio.read_hdus(str(tmp_path / 'on' / 'ML1_20240102_030400_red_trans_hdr.fits'))[0][0]
    keys = ['A-P', 'A-PLDG', 'A-NVOTE', 'A-NRUN', 'A-NFAR', 'A-NPAIR', 'A-RMSX', 'A-RMSY', 'A-DX', 'A-DY', 'A-ROT', 'A-SCALE', 'A-FLAGS', 'A-NEDGE',
            'T-NOFFR']
    print('command line, switch on:', {k: R.hval(h, k) for k in keys if k in h})
    for k in keys:
        assert k in h, k
    assert bool(R.hval(h, 'A-P')) is True and abs(R.hval(h, 'A-DX') + 1.0) <= 0.1 and abs(R.hval(h, 'A-DY') + 9.0) <= 0.1
    # switched off the products are those of the command without the flag (a reference on the new frame's grid)
    fitsio.write_image(str(tmp_path / 'ref0.fits'), ref[9:9 + ny, 1:1 + nx].copy())
    cli.main(common + ['--ref', str(tmp_path / 'ref0.fits'), '--red_dir', str(tmp_path / 'plain')])
    cli.main(common + ['--ref', str(tmp_path / 'ref0.fits'), '--red_dir', str(tmp_path / 'off'), '--ref_align', 'False'])
    plain, off = tree(str(tmp_path / 'plain')), tree(str(tmp_path / 'off'))
    assert sorted(plain) == sorted(off) and any(k.endswith('_trans_hdr.fits') for k in plain)
    for name in sorted(plain):
        if not name.endswith('.fits'):
            continue
        for (ha, da), (hb, db) in zip(fitsio.read_hdus(plain[name]), fitsio.read_hdus(off[name])):
            assert list(ha) == list(hb), name
            assert not [k for k in ha if k.startswith('A-') or k == 'T-NOFFR'], name
            for k in ha:
                if k not in VOLATILE:
                    assert R.hval(ha, k) == R.hval(hb, k) or (R.hval(ha, k) != R.hval(ha, k) and R.hval(hb, k) != R.hval(hb, k)), (name, k)
            assert (da is None) == (db is None) and (da is None or np.asarray(da).tobytes() == np.asarray(db).tobytes()), name


# ---- pipeline --------------------------------------------------------------------------------------------------------
def test_pipeline_equals_serial_calls(ctx):
    """three frames of one field through a two-lane FramePipeline with ref_align=True against a reference of another shape:
    header_trans of every frame is that of a serial call, and the reference's star list is made once and kept for the run"""
    import bbx_oracle as O
    from blackbox_amd import synth
    from blackbox_amd.pipeline import FramePipeline, HostPool
    tel, ys, xs, nframes, lanes = 'ML1', 124, 124, 3, 2
    size, border, box, S = 124, 8, 31, 11
    case = synth.make_case(ys, xs, 300, tel=tel, os_y=20, os_x=45, n_stars=150, n_sat=2, n_cr=30)
    rs = np.random.RandomState(2)
    flat, bpm = dev(ctx, case['flat']), dev(ctx, case['bpm'])
    coeffs = O.xtalk_coeffs(case['xtalk'])
    raws = [dev(ctx, np.clip(case['raw'].astype(np.int64) + rs.randint(-3, 4, case['raw'].shape), 0, 65535).astype(case['raw'].dtype))
            for _ in range(nframes)]
    geom = R.geometry(raws[0].shape, ys, xs)
    red = [R.reduce_object(ctx, raw, {}, tel, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, ysize_chan=ys, xsize_chan=xs,
                           detect_sats=False)[:2] for raw in raws]
    d0 = red[0][0].cpu().numpy()
    ny, nx = d0.shape
    ref_np = rs.normal(0, 4, (ny + 2 * box, nx + box)).astype(F)
    ref_np[7:7 + ny, 12:12 + nx] += (d0 - np.median(d0)).astype(F)   # new (y, x) -> ref (y + 7, x + 12)
    ref = dev(ctx, ref_np)
    nsub = (ny // size) * (nx // size)
    g = np.arange(S) - S // 2
    psf = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2 * 1.5 ** 2))
    psf = dev(ctx, np.repeat((psf / psf.sum()).astype(F)[None], nsub, 0))
    sig = 1.4826 * np.median(np.abs(d0 - np.median(d0))) + 4.0
    sub_kw = dict(ref=ref, ref_mask=torch.zeros(ref.shape, dtype=torch.uint8, device=ctx.device), psf_new=psf, psf_ref=psf, fratio=1.0,
                  ref_is_bkgsub=True, ref_bkg_std_mini=np.full((ref.shape[0] // box, ref.shape[1] // box), sig, F), subimage_size=size,
                  subimage_border=border, bkg_boxsize=box, ref_align=True)
    serial = []
    for data, mask in red:
        res = G.optimal_subtraction(ctx, data, new_mask=mask, **sub_kw)
        ctx.sync()
        serial.append(res['header_trans'])
    print('serial: %s' % [{k: h[k][0] for k in ('A-P', 'A-NVOTE', 'A-NPAIR', 'A-DX', 'A-DY', 'T-NOFFR')} for h in serial])
    assert all(h['A-P'][0] is True and abs(h['A-DX'][0] + 12) < 0.1 and abs(h['A-DY'][0] + 7) < 0.1 for h in serial)
    pool = HostPool(4)
    pipe = FramePipeline(ctx, tel, geom, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, pool=pool, depth=3, do_finish=True,
                         keep_outputs=True, lanes=lanes, subtract=sub_kw)
    got = {}

    def done(idx, f):
        assert not f.failed, f.failed
        got[idx] = f.sub['header_trans']
    n0 = G.RefStars.builds
    try:
        n = pipe.run([(r, {}) for r in raws], on_done=done)
        assert pipe.ref_stars is not None and pipe.ref_stars.matches(ref) and pipe.ref_bkg_std is None
    finally:
        pipe.close()
        pool.close()
    assert pipe.ref_stars is None                                    # dropped with the run's other reference products
    assert n == nframes and sorted(got) == list(range(nframes))
    assert 1 <= G.RefStars.builds - n0 <= lanes                      # (two lanes may both start before either has one to hand over)
    for k in range(nframes):
        assert got[k] == serial[k], k
