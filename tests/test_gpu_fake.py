"""GPU: fake stars (bbx_fake.hip; include/bbx.h: bbx_fake_inject, bbx_fake_recover) against the numpy restatement of fake_ref.py on
that file's cases; optimal_subtraction(fake_stars=N) end to end on the scene of test_psfbuild_host.py with a PSF model for the new
frame and a stamp for the reference; the command line with the switch on."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import fake_ref as FR                         # noqa: E402
import psfphot_ref as PR                      # noqa: E402
import test_psfbuild_host as P                # noqa: E402  (the scene)
import test_gpu_match as M                    # noqa: E402
import test_gpu_psfphot as GP                 # noqa: E402  (truth_model)
from test_gpu_match import ctx                # noqa: E402,F401  (fixture)
from test_gpu_transfit import same            # noqa: E402  (the comparison of two results)
from blackbox_amd import _args                # noqa: E402
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402
from blackbox_amd._lib import lib, ptr        # noqa: E402

F = np.float32
dev = M.dev
BORDER, BOX = 12, 20
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23


# ---- bbx_fake_inject ------------------------------------------------------------------------------------------------------------
def device_sigma(ctx, case, g):
    if case['sig_form'] == 'frame':
        return dev(ctx, g['sigma'])
    return G.MiniImage(ctx, case['mini'], FR.BOX, interp_Xchan=case['sig_form'] == 'mini_x')


def gpu_inject(ctx, case, g, noise=False, seed=0, frame=None, ref=True, masks=True):
    """one launch of the entry itself (the PSF planes and terms are the case's, not a frame's tiling) -> dict like inject_ref's"""
    ny, nx, S = case['ny'], case['nx'], case['S']
    n = len(g['ys'])
    d_frame = dev(ctx, g['frame'] if frame is None else frame).clone()
    d_sigma = device_sigma(ctx, case, g)                                # (named: the pointer below must not outlive it)
    sig = _args.sigma_map(d_sigma, (ny, nx))
    d_ref, d_mn, d_mr = dev(ctx, g['ref']) if ref else None, dev(ctx, g['mask_new']) if masks else None, dev(ctx, g['mask_ref']) if masks else None
    cube = dev(ctx, case['cube'])
    terms = dev(ctx, g['terms']) if g['terms'] is not None else None
    idx = dev(ctx, g['idx']) if g['idx'] is not None else None
    d_ys, d_xs, d_off, d_s2n = dev(ctx, g['ys']), dev(ctx, g['xs']), dev(ctx, g['off']), dev(ctx, g['s2n'])
    flux, real, snr = (torch.full((n,), -1.0, dtype=torch.float32, device=ctx.device) for _ in range(3))
    flags = torch.full((n,), 255, dtype=torch.uint8, device=ctx.device)
    rc = lib.bbx_fake_inject(ctx.h, ny, nx, ptr(d_frame), ptr(d_ref), *sig, ptr(d_mn), ptr(d_mr), S, int(cube.shape[0]), ptr(cube), ptr(terms), ptr(idx),
                             n, ptr(d_ys), ptr(d_xs), ptr(d_off), ptr(d_s2n), FR.CLEAR_HALF, FR.CLEAR_NSIGMA, int(noise), seed, ptr(flux), ptr(real),
                             ptr(snr), ptr(flags), ctx.stream())
    assert rc == 0
    ctx.sync()
    return dict(out=d_frame.cpu().numpy(), flux=flux.cpu().numpy(), real=real.cpu().numpy(), snr_sky=snr.cpu().numpy(), flags=flags.cpu().numpy())


def noisy_frame_meets(got, base, want, ys, xs, S):
    """a frame with the stars' own noise against the restatement's: per star, inside its stamp, 4 x (D32_ADD F max P + D32_NOISE
    sqrt(F max P)) -- the two measured distances of fake_ref.py, each on its own scale -- plus the rounding of the frame; outside the
    unflagged stamps the bits of the frame as it was.  -> the largest deviation in units of its bound"""
    h = S // 2
    inside = np.zeros(got.shape, bool)
    worst = 0.0
    for k in np.nonzero(want['flags'] == 0)[0]:
        sl = np.s_[ys[k] - h:ys[k] + h + 1, xs[k] - h:xs[k] + h + 1]
        inside[sl] = True
        fp = want['flux'][k] * want['pmax'][k]
        bound = 4 * (FR.D32_ADD * fp + FR.D32_NOISE * np.sqrt(fp)) + EPS24 * np.abs(got[sl])
        d = np.abs(got[sl].astype(np.float64) - want['out'][sl])
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (int(k), float((d / bound).max()))
    assert got[~inside].tobytes() == np.asarray(base, F)[~inside].tobytes()
    return worst


@pytest.mark.parametrize('spec', FR.CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_inject_meets_the_restatement(ctx, spec):
    case = FR.make_case(*spec)
    S, h = case['S'], case['S'] // 2
    tags, worst = [], dict(F=0.0, sn=0.0, add=0.0, real=0.0)
    for g in case['groups']:
        want = FR.run_group(case, g)
        got, again = gpu_inject(ctx, case, g), gpu_inject(ctx, case, g)
        for k in ('out', 'flux', 'real', 'snr_sky', 'flags'):
            assert got[k].tobytes() == again[k].tobytes(), k           # two runs: the same bytes
        assert got['flags'].tolist() == want['flags'].tolist() == [s['want'] for s in g['stars']], [s['tag'] for s in g['stars']]
        inside = np.zeros((case['ny'], case['nx']), bool)
        for k, s in enumerate(g['stars']):
            tags.append(s['tag'])
            if got['flags'][k]:
                assert got['flux'][k] == 0 and got['real'][k] == 0 and got['snr_sky'][k] == 0
                continue
            sl = np.s_[s['y'] - h:s['y'] + h + 1, s['x'] - h:s['x'] + h + 1]
            inside[sl] = True
            Fg, Fw = float(got['flux'][k]), want['flux'][k]
            worst['F'] = max(worst['F'], abs(Fg / Fw - 1))
            # the restatement's S/N at the kernel's own F, on the restatement's own stamp and sigma
            Pm, norm = FR.stamp(case['cube'], g['terms'], g['idx'], k, g['off'], np.float64)
            sn = FR.snr(Fg, Pm / norm, g['sigma'][sl].astype(np.float64) ** 2)
            worst['sn'] = max(worst['sn'], abs(sn / float(g['s2n'][k]) - 1))
            diff = got['out'][sl].astype(np.float64) - g['frame'][sl].astype(np.float64)
            bound = 4 * FR.D32_ADD * Fw * want['pmax'][k] + EPS24 * np.abs(got['out'][sl])
            dev_add = np.abs(diff - want['add'][k])
            worst['add'] = max(worst['add'], float((dev_add / (Fw * want['pmax'][k])).max()))
            assert (dev_add <= bound).all(), (s['tag'], float((dev_add / bound).max()))
            rbound = float(bound.max()) * S * S
            worst['real'] = max(worst['real'], abs(float(got['real'][k]) - diff.sum()) / rbound)
            assert abs(float(got['real'][k]) - diff.sum()) <= rbound + EPS24 * abs(diff.sum())
            assert abs(float(got['snr_sky'][k]) / want['snr_sky'][k] - 1) <= 4 * FR.D32_F + EPS23
        # every pixel outside the unflagged stamps keeps its bits (a flagged star changed nothing)
        assert got['out'][~inside].tobytes() == g['frame'][~inside].tobytes()
    print(spec, '%d launches, %d stars: F %.2e (%.1e), S/N at the kernel\'s F %.2e (%.1e), add / (F max P) %.2e (%.1e + rounding), real %.2e of its bound'
          % (len(case['groups']), len(tags), worst['F'], 4 * FR.D32_F, worst['sn'], 4 * FR.D32_F + EPS23, worst['add'], 4 * FR.D32_ADD, worst['real']))
    assert worst['F'] <= 4 * FR.D32_F and worst['sn'] <= 4 * FR.D32_F + EPS23
    assert len(set(tags)) == len(tags) >= (24 if case['sig_form'] == 'frame' else 23)


def test_wrapper_meets_the_entry(ctx):
    """zogy.fake_inject on a tiling: the planes by tile_index, the terms by psf_poly_terms, the same bits as the restatement asks"""
    ny, nx, size, S = 96, 128, 32, 9
    rs = np.random.RandomState(1)
    sigma = np.full((ny, nx), 10.0, F)
    frame = rs.normal(0, 10, (ny, nx)).astype(F).clip(-40, 40)
    cube = np.stack([FR.wing_stamp(S, 3.0 + 0.1 * q) for q in range(12)]).astype(F)
    lay = G.fake_layout(ny, nx, size, 3, 4, S, 1, (5, 50), 2)
    d_frame = dev(ctx, frame)
    inj, _ = G.fake_inject(ctx, d_frame, None, dev(ctx, sigma), None, None, None, dev(ctx, cube), lay, 4, size, noise=True, seed=5)
    ctx.sync()
    want = FR.inject_ref(frame, None, sigma, None, None, cube, None, lay['sub'], lay['ys'], lay['xs'], lay['off'], lay['s2n'], 3, 5.0, True, 5)
    assert inj[3].cpu().numpy().tolist() == want['flags'].tolist() == [0] * 12
    assert np.abs(inj[0].cpu().numpy() / want['flux'] - 1).max() <= 4 * FR.D32_F
    noisy_frame_meets(d_frame.cpu().numpy(), frame, want, lay['ys'], lay['xs'], S)
    bad = dict(lay, ys=lay['ys'].copy())
    bad['ys'][1], bad['xs'] = lay['ys'][0] + 3, lay['xs'].copy()
    bad['xs'][1] = lay['xs'][0]
    before = d_frame.clone()
    with pytest.raises(ValueError):
        G.fake_inject(ctx, d_frame, None, dev(ctx, sigma), None, None, None, dev(ctx, cube), bad, 4, size)
    ctx.sync()
    assert torch.equal(before, d_frame)                                # refused before anything was queued


# ---- noise ----------------------------------------------------------------------------------------------------------------------
def flat_case(nstar, S=49):
    """nstar flat stamps side by side on a frame of zeros under sigma 1, asked for the S/N that makes F P = 4"""
    ny, nx = S + 2, nstar * S + 2
    cube = np.full((1, S, S), 1.0 / (S * S), F)
    p = cube[0].astype(np.float64) / cube[0].astype(np.float64).sum()
    s2n = F(FR.snr(4.0 * S * S, p, np.ones(S * S)))
    g = dict(frame=np.zeros((ny, nx), F), ref=None, sigma=np.ones((ny, nx), F), mask_new=None, mask_ref=None, terms=None, idx=np.zeros(nstar, np.int32),
             ys=np.full(nstar, 1 + S // 2, np.int32), xs=(1 + S // 2 + S * np.arange(nstar)).astype(np.int32), off=np.zeros((nstar, 2), F),
             s2n=np.full(nstar, s2n, F))
    return dict(ny=ny, nx=nx, S=S, sig_form='frame', cube=cube), g


def test_noise_is_the_generator_of_the_header(ctx):
    nstar, S = 64, 49
    case, g = flat_case(nstar, S)
    a = gpu_inject(ctx, case, g, noise=True, seed=12345, ref=False, masks=False)
    b = gpu_inject(ctx, case, g, noise=True, seed=12345, ref=False, masks=False)
    c = gpu_inject(ctx, case, g, noise=True, seed=12346, ref=False, masks=False)
    d = gpu_inject(ctx, case, g, noise=True, seed=12345 + (1 << 32), ref=False, masks=False)
    assert a['out'].tobytes() == b['out'].tobytes() and a['real'].tobytes() == b['real'].tobytes()
    assert a['out'].tobytes() != c['out'].tobytes() and a['out'].tobytes() != d['out'].tobytes() and a['flux'].tobytes() == c['flux'].tobytes()
    assert not a['flags'].any()
    fp = a['flux'].astype(np.float64) / (S * S)
    assert np.abs(fp - 4.0).max() < 1e-3
    dev_g = np.zeros((nstar, S * S))
    worst = 0.0
    for s in range(nstar):
        st = a['out'][1:1 + S, 1 + s * S:1 + (s + 1) * S].astype(np.float64)
        dev_g[s] = ((st - fp[s]) / np.sqrt(fp[s])).ravel()
        worst = max(worst, np.abs(dev_g[s] - FR.normals(12345, s, S * S)).max())
    print('largest |(out - F P) / sqrt(F P) - g| over %d draws %.3e (tolerance %.1e)' % (dev_g.size, worst, FR.NOISE_TOL))
    assert worst <= FR.NOISE_TOL
    # the moments of the host test, on the device's own draws
    n = dev_g.size
    assert abs(dev_g.mean()) <= 5 / np.sqrt(n) and abs(dev_g.var() - 1) <= 5 * np.sqrt(2.0 / n)
    assert abs((dev_g[:, 1:] * dev_g[:, :-1]).mean()) <= 5 / np.sqrt(n) and abs((dev_g[1:] * dev_g[:-1]).mean()) <= 5 / np.sqrt(n)
    # real: the float64 sum of what was added
    sums = np.array([a['out'][1:1 + S, 1 + s * S:1 + (s + 1) * S].astype(np.float64).sum() for s in range(nstar)])
    assert np.abs(a['real'] - sums).max() <= S * S * EPS24 * 20.0


def test_noise_on_a_case_meets_the_restatement(ctx):
    case = FR.make_case(*FR.CASES[2])
    g = case['groups'][0]
    want = FR.run_group(case, g, noise=True, seed=99)
    got = gpu_inject(ctx, case, g, noise=True, seed=99)
    assert got['flags'].tolist() == want['flags'].tolist()
    worst = noisy_frame_meets(got['out'], g['frame'], want, g['ys'], g['xs'], case['S'])
    print('noise on, %s: largest deviation %.2f of its bound' % (FR.CASES[2], worst))


# ---- bbx_fake_recover -----------------------------------------------------------------------------------------------------------
def test_recover_is_exact(ctx):
    ny, nx = 40, 52
    rs = np.random.RandomState(8)
    sc = rs.normal(0, 1, (ny, nx)).astype(F)
    fp, fe = rs.normal(0, 100, (ny, nx)).astype(F), rs.uniform(5, 10, (ny, nx)).astype(F)
    stars = [(20, 26), (10, 10), (30, 40), (0, 0), (0, 25), (ny - 1, nx - 1), (ny - 1, 0), (15, nx - 1), (1, nx - 2), (25, 8), (33, 20), (12, 44)]
    sc[20, 27] = 50.0                                                    # a unique maximum
    sc[9:12, 9:12] = 7.0                                                 # ties: the lowest row, then the lowest column
    sc[12, 8] = 7.0
    sc[28:33, 38:43] = 3.0
    sc[32, 42], sc[31, 38] = 9.0, 9.0                                    # two equal maxima: the lower row wins
    sc[21:30, 4:13] = np.nan                                             # (25, 8): an all-NaN window at every radius
    sc[33, 20] = np.inf                                                  # not finite: skipped
    sc[12, 44], sc[12, 45] = -0.0, 0.0
    sc[10:15, 42:47][np.isfinite(sc[10:15, 42:47]) & (sc[10:15, 42:47] > 0)] = -1.0          # -0.0 and 0.0 are equal: the first
    ys, xs = np.array([s[0] for s in stars], np.int32), np.array([s[1] for s in stars], np.int32)
    d = [dev(ctx, a) for a in (sc, fp, fe)]
    for radius in (0, 2, 4):
        got = G.fake_recover(ctx, d[0], d[1], d[2], dict(ys=ys, xs=xs), radius)
        ctx.sync()
        got, want = got.cpu().numpy(), FR.recover_ref(sc, fp, fe, ys, xs, radius)
        assert got.dtype == np.float32 and got.shape == (len(stars), 6)
        assert got.tobytes() == want.tobytes(), (radius, got, want)
        assert np.isnan(got[9, :2]).all() and not got[9, 2:].any()
    assert lib.bbx_fake_recover(ctx.h, ny, nx, ptr(d[0]), ptr(d[1]), ptr(d[2]), 1, ptr(dev(ctx, ys)), ptr(dev(ctx, xs)), 5, ptr(d[0]), ctx.stream()) == -1
    assert lib.bbx_fake_recover(ctx.h, ny, nx, None, ptr(d[1]), ptr(d[2]), 1, ptr(dev(ctx, ys)), ptr(dev(ctx, xs)), 2, ptr(d[0]), ctx.stream()) == -1


# ---- optimal_subtraction(fake_stars=N) ------------------------------------------------------------------------------------------
NPER, S2N = 4, (2.0, 9.0, 30.0)


@pytest.fixture(scope='module')
def e2e(ctx):
    sc, ref = P.make_scene(), P.make_scene(fwhm_ref=3.0)
    new, rimg = np.nan_to_num(sc['img']).astype(np.float64), np.nan_to_num(ref['img']).astype(np.float64)
    model = GP.truth_model(ctx)
    mask = dev(ctx, sc['mask'])
    d_new, d_ref = dev(ctx, (new + 300.0).astype(F)), dev(ctx, rimg.astype(F))
    psf_ref = dev(ctx, PR.moffat_stamp(P.V, 3.0).astype(F))
    calls = []
    orig = (G._fake_launch, G._fake_recover)

    def counted(f):
        def w(*a, **k):
            calls.append(f.__name__)
            return f(*a, **k)
        return w
    G._fake_launch, G._fake_recover = counted(orig[0]), counted(orig[1])
    new_before = d_new.clone()

    def call(psf_new=model, **kw):
        n0 = len(calls)
        res = G.optimal_subtraction(ctx, d_new, d_ref, mask, torch.zeros_like(mask), psf_new, psf_ref, subimage_size=P.SIZE, subimage_border=BORDER,
                                    bkg_boxsize=BOX, ref_is_bkgsub=True, ref_bkg_std_mini=np.full((P.NY // BOX, P.NX // BOX), P.SKY, F),
                                    trans_extract=True, cat_extract=True, fratio=1.0, thumbnails=True, thumbnail_size=16, **kw)
        ctx.sync()
        return res, calls[n0:]
    try:
        out = dict(plain=call(), off=call(fake_stars=0), on=call(fake_stars=NPER, fake_s2n=S2N), again=call(fake_stars=NPER, fake_s2n=S2N),
                   quiet=call(fake_stars=NPER, fake_s2n=S2N, fake_noise=False),
                   vet=call(fake_stars=NPER, fake_s2n=S2N, trans_psffit=True, trans_chi2_max=2.0),
                   big=call(fake_stars=17, fake_s2n=S2N))
        # the stages in front of the injection, each once without and once with the stars: the PSF build, the star match, the registration
        for name, kw in (('build', dict(psf_new=None, psf_build=True)), ('match', dict(match=True)), ('align', dict(ref_align=True))):
            out[name + '_off'], out[name + '_on'] = call(**kw), call(fake_stars=NPER, fake_s2n=S2N, **kw)
    finally:
        G._fake_launch, G._fake_recover = orig
    out.update(sc=sc, model=model, new_untouched=torch.equal(new_before, d_new))
    return out


def test_switch_off_changes_nothing(e2e):
    (a, ca), (b, cb) = e2e['plain'], e2e['off']
    assert ca == [] and cb == []                                         # no new entry is called
    assert list(a) == list(b)
    same(a, b)
    assert 'fakestars' not in a and not any(k.startswith(('T-FK', 'T-NFAKE', 'T-FAKESN', 'T-NFKTR')) for k in a['header_trans'])
    assert all('fake_star' not in t for t in a['transients'])


def frame_of(ctx, s):
    return (s.frame(ctx) if isinstance(s, G.MiniImage) else s).cpu().numpy()


def test_switch_on_plants_and_finds_the_stars(ctx, e2e):
    (on, con), (off, _), (again, _) = e2e['on'], e2e['off'], e2e['again']
    assert con == ['fake_launch', 'fake_recover'] and e2e['new_untouched']
    # what is made before the injection is the off run's
    for k in ('catalog', 'header_new', 'bkg_mini_new', 'bkg_std_mini_new', 'ref_bkgsub'):
        same(off[k], on[k], k)
    # the PSF build, the star match and the registration never see a fake star: their results are the off run's, and the stars go in
    for name, key in (('build', 'psf'), ('match', 'match'), ('align', 'align')):
        (a, ca), (b, cb) = e2e[name + '_off'], e2e[name + '_on']
        assert key in a and key in b and ca == [] and cb == ['fake_launch', 'fake_recover'], (name, list(a), ca, cb)
        for k in (key, 'catalog', 'header_new', 'ref_bkgsub') + (('ref_mask_remapped',) if name == 'align' else ()):
            same(a[k], b[k], name + '/' + k)
        assert b['header_trans']['T-FKP'][0] is True and b['header_trans']['T-NFAKE'][0] > 0 and not torch.equal(a['data_bkgsub'], b['data_bkgsub'])
        print('%s: %s; %d stars planted behind it' % (name, {k: v for k, v in a[key].items() if isinstance(v, (bool, int, float))} if isinstance(a[key], dict)
                                                      else type(a[key]).__name__, b['header_trans']['T-NFAKE'][0]))
    # two runs: the same bytes
    for k in ('data_bkgsub', 'Scorr', 'Fpsf'):
        same(on[k], again[k], k)
    same(on['fakestars']['table'], again['fakestars']['table'])
    fk = on['fakestars']
    lay, tab = fk['layout'], fk['table']
    nstar = P.NSY * P.NSX * NPER
    assert tuple(tab) == G.FAKE_COLS and len(tab['NUMBER']) == nstar and lay['S'] == P.V
    # data_bkgsub differs from the off run by the restatement's stamps
    m = e2e['model']
    terms = G.psf_poly_terms(lay['xs'] + 1.0, lay['ys'] + 1.0, m['polzero'], m['polscal'], m['poldeg'])
    base = off['data_bkgsub'].cpu().numpy()
    want = FR.inject_ref(base, off['ref_bkgsub'].cpu().numpy(), frame_of(ctx, off['bkg_std']), e2e['sc']['mask'], np.zeros_like(e2e['sc']['mask']),
                         m['basis'].cpu().numpy(), terms, None, lay['ys'], lay['xs'], lay['off'], lay['s2n'], 3, 5.0, True, lay['seed'])
    assert tab['FLAGS_IN'].tolist() == want['flags'].tolist()
    ok = want['flags'] == 0
    print('%d of %d stars injected, flags %s' % (ok.sum(), nstar, np.bincount(want['flags'], minlength=17).nonzero()[0].tolist()))
    assert ok.sum() >= nstar * 2 // 3
    assert np.abs(tab['E_FLUX_IN'][ok] / want['flux'][ok] - 1).max() <= 4 * FR.D32_F
    got = on['data_bkgsub'].cpu().numpy()
    worst = noisy_frame_meets(got, base, want, lay['ys'], lay['xs'], P.V)
    print('data_bkgsub against the restatement: largest deviation %.2f of its per-star bound' % worst)
    assert (got != base).sum() > 0 and np.abs(tab['E_FLUX_REAL'][ok] / want['real'][ok] - 1).max() <= 1e-5
    # the recovery columns: the restatement on the GPU's own frames, exactly
    rec = FR.recover_ref(on['Scorr'].cpu().numpy(), on['Fpsf'].cpu().numpy(), on['Fpsferr'].cpu().numpy(), lay['ys'], lay['xs'], 2)
    for j, col in ((2, 'SCORR_OUT'), (3, 'E_FLUX_OUT'), (4, 'E_FLUXERR_OUT'), (5, 'E_FLUX_OUT_AT')):
        assert tab[col].tobytes() == rec[:, j].tobytes(), col
    assert np.array_equal(tab['Y_PEAK'], (lay['ys'] + 1 + rec[:, 0]).astype(F)) and np.array_equal(tab['X_PEAK'], (lay['xs'] + 1 + rec[:, 1]).astype(F))
    # found or not
    rows = on['transients']
    star_of = np.array([t['fake_star'] for t in rows])
    bright, faint, mid = (ok & (tab['SNR_IN'] == s) for s in (30.0, 2.0, 9.0))
    assert bright.sum() >= 8 and ((tab['FOUND'][bright] & 3) == 3).all()
    for k in np.nonzero(bright)[0]:
        j = np.nonzero(star_of == k + 1)[0]
        assert j.size >= 1 and max(abs(rows[j[0]]['y'] - lay['ys'][k]), abs(rows[j[0]]['x'] - lay['xs'][k])) <= 2 and tab['NUMBER_TRANS'][k] == j[0] + 1
    assert int(((tab['FOUND'][faint] & 3) != 0).sum()) <= 1
    ht = on['header_trans']
    print('S/N 9: %d of %d found as candidates; T-FKFRAT %s T-FKFSTD %s T-FKPULL %s T-FKSCRT %s' % (
        int(((tab['FOUND'][mid] & 2) != 0).sum()), int(mid.sum()), ht['T-FKFRAT'][0], ht['T-FKFSTD'][0], ht['T-FKPULL'][0], ht['T-FKSCRT'][0]))
    # the off run's candidates away from every star are still there
    far, near = [], []
    for t in off['transients']:
        d = np.maximum(np.abs(lay['ys'][ok] - t['y']), np.abs(lay['xs'][ok] - t['x'])).min()
        (far if d > P.V else near).append(t)
    at = {(t['y'], t['x']): t for t in rows}
    worst = np.zeros(3)
    for t in far:
        u = at.get((t['y'], t['x']))
        assert u is not None and u['fake_star'] == 0, t
        # no bit identity: the float32 transforms of the sub-image round differently with other input.  Four times the measured
        # changes of fake_ref.py, each in its own unit
        d = (abs(u['scorr'] - t['scorr']), abs(u['fpsf'] - t['fpsf']) / t['fpsferr'], abs(u['fpsferr'] / t['fpsferr'] - 1))
        worst = np.maximum(worst, d)
        assert d[0] <= 4 * FR.FAR_DSCORR and d[1] <= 4 * FR.FAR_DFPSF and d[2] <= 4 * FR.FAR_DFPSFERR, (t, u, d)
    print('%d candidates of the off run beyond a stamp of every star: largest change of Scorr %.3e, of Fpsf %.3e Fpsferr, of Fpsferr %.3e (module: '
          '%.1e %.1e %.1e); %d within one: %s' % (len(far), worst[0], worst[1], worst[2], FR.FAR_DSCORR, FR.FAR_DFPSF, FR.FAR_DFPSFERR, len(near),
                                                  [(t['y'], t['x']) for t in near]))
    assert len(far) >= 5                                               # (the scene has seventeen candidates of its own)
    n_off, n_on, nfk = off['header_trans']['T-NTRANS'][0], ht['T-NTRANS'][0], ht['T-NFKTR'][0]
    assert n_on == len(rows) and nfk == int((star_of > 0).sum()) and abs(n_on - (n_off + nfk)) <= len(near)
    # the keys
    keys = ['T-FKP', 'T-NFAKE', 'T-FAKESN', 'T-FKNASK', 'T-FKNREJ', 'T-FKSEED', 'T-FKNOIS', 'T-FKRAD', 'T-NFKTR'] + \
        ['T-FK%s%d' % (a, k) for k in (1, 2, 3) for a in ('SN', 'N', 'EF', 'VT')] + ['T-FKFRAT', 'T-FKFSTD', 'T-FKPULL', 'T-FKSCRT']
    assert [k for k in ht if k.startswith(('T-FK', 'T-NFAKE', 'T-FAKESN', 'T-NFKTR'))] == keys
    assert {k: v for k, v in ht.items() if k not in keys and k != 'T-NTRANS' and not k.startswith('Z-')} == \
        {k: v for k, v in off['header_trans'].items() if k != 'T-NTRANS' and not k.startswith('Z-')}
    assert ht['T-FKP'][0] is True and ht['T-NFAKE'][0] == int(ok.sum()) and ht['T-FAKESN'][0] == 2.0 and ht['T-FKNASK'][0] == nstar
    assert ht['T-FKNREJ'][0] == nstar - int(ok.sum()) and ht['T-FKSEED'][0] == 0 and ht['T-FKNOIS'][0] is True and ht['T-FKRAD'][0] == 2
    assert [ht['T-FKSN%d' % k][0] for k in (1, 2, 3)] == list(S2N) and ht['T-FKEF3'][0] == 1.0 and ht['T-FKVT3'][0] == 1.0
    assert ht['T-FKN3'][0] == int(bright.sum()) and isinstance(ht['T-FKFRAT'][0], float) and isinstance(ht['T-FKPULL'][0], float)
    # the thumbnails follow the rows
    assert on['thumbnails'].shape[0] == len(rows)
    # noise off: another frame, the same stars
    quiet = e2e['quiet'][0]
    assert quiet['header_trans']['T-FKNOIS'][0] is False and quiet['fakestars']['table']['E_FLUX_IN'].tobytes() == tab['E_FLUX_IN'].tobytes()
    qok = quiet['fakestars']['table']['FLAGS_IN'] == 0
    assert np.abs(quiet['fakestars']['table']['E_FLUX_REAL'][qok] / tab['E_FLUX_IN'][qok] - 1).max() <= 1e-5
    assert not torch.equal(quiet['data_bkgsub'], on['data_bkgsub'])


def test_vetting_carries_the_flag(e2e):
    vet, calls = e2e['vet']
    rows, tab = vet['transients'], vet['fakestars']['table']
    assert calls == ['fake_launch', 'fake_recover'] and 'T-NVET' in vet['header_trans'] and vet['header_trans']['T-NVET'][0] == len(rows)
    assert len(rows) < vet['header_trans']['T-NTRANS'][0]                 # the bound dropped rows
    star_of = np.array([t['fake_star'] for t in rows])
    for k in range(len(tab['NUMBER'])):
        j = np.nonzero(star_of == k + 1)[0]
        assert bool(tab['FOUND'][k] & 4) == (j.size > 0) and tab['NUMBER_TRANS'][k] == (j[0] + 1 if j.size else 0)
        assert not (tab['FOUND'][k] & 4) or tab['FOUND'][k] & 2
    dropped = ((tab['FOUND'] & 2) != 0) & ((tab['FOUND'] & 4) == 0)
    print('vetting at chi2 <= 2: %d fake stars with a row, %d of them dropped' % (int(((tab['FOUND'] & 2) != 0).sum()), int(dropped.sum())))
    ht = vet['header_trans']
    assert ht['T-FKVT3'][0] <= ht['T-FKEF3'][0]
    assert vet['thumbnails'].shape[0] == len(rows)


def test_a_layout_that_does_not_fit_leaves_the_frame_alone(e2e):
    (big, calls), (off, _) = e2e['big'], e2e['off']
    assert calls == []                                                   # the layout fails before either entry
    ht = big['header_trans']
    assert ht['T-FKP'][0] is False and ht['T-NFAKE'][0] == 0 and ht['T-FAKESN'][0] == 'None' and 'fakestars' not in big
    assert {k: v for k, v in ht.items() if k not in ('T-FKP', 'T-NFAKE', 'T-FAKESN')} == dict(off['header_trans'])
    for k in ('data_bkgsub', 'D', 'Scorr', 'Fpsf', 'Fpsferr', 'transients', 'catalog', 'thumbnails'):
        same(off[k], big[k], k)


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_table_the_column_and_the_keys(tmp_path, ctx):
    """blackbox.py --fake_stars 2 --fake_s2n 30 through --image and --image_list on the raw frame of test_gpu_thumbs' command-line test
    (PSF stamps of 15, --subimage_size 120); without the switch today's files"""
    import test_gpu_thumbs as TT
    from blackbox_amd import fitsio, synth
    import bbx_oracle as O
    cli = TT.load_cli()
    YS, XS, TEL = TT.YS, TT.XS, TT.TEL
    case = synth.make_case(YS, XS, 77, tel=TEL, os_y=20, os_x=45, n_stars=60, n_sat=2, n_cr=40)
    hdr = {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q'}
    raws = []
    for k in range(2):
        raws.append(str(tmp_path / ('ML1_raw%d.fits' % k)))
        fitsio.write_image(raws[-1], case['raw'], dict(hdr, **{'DATE-OBS': '2024-01-02T03:04:0%d' % k}))
    fitsio.write_image(str(tmp_path / 'flat.fits'), case['flat'])
    fitsio.write_image(str(tmp_path / 'bpm.fits'), case['bpm'])
    synth.write_xtalk(str(tmp_path / 'xtalk.dat'), case['xtalk'])
    d0 = R.reduce_object(ctx, dev(ctx, case['raw']), {}, TEL, mflat=dev(ctx, case['flat']), bpm=dev(ctx, case['bpm']),
                         xtalk_coeffs=O.xtalk_coeffs(case['xtalk']), exptime=60.0, ysize_chan=YS, xsize_chan=XS, log=logging.getLogger('t'))[0]
    ref = (d0.cpu().numpy() - 100.0 + np.random.RandomState(3).normal(0, 4, d0.shape)).astype(F)
    fitsio.write_image(str(tmp_path / 'ref.fits'), ref)
    fitsio.write_image(str(tmp_path / 'psf.fits'), TT.moffat_stamp(15, 3.5))
    common = ['--telescope', TEL, '--mflat', str(tmp_path / 'flat.fits'), '--bpm', str(tmp_path / 'bpm.fits'),
              '--crosstalk', str(tmp_path / 'xtalk.dat'), '--ysize_chan', str(YS), '--xsize_chan', str(XS),
              '--cat_extract', 'True', '--trans_extract', 'True', '--ref', str(tmp_path / 'ref.fits'),
              '--psf_new', str(tmp_path / 'psf.fits'), '--psf_ref', str(tmp_path / 'psf.fits'),
              '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30']
    on = ['--fake_stars', '2', '--fake_s2n', '30']
    name = 'ML1_20240102_030400_red'

    def files(sub):
        return sorted(os.listdir(str(tmp_path / sub)))

    def product(sub, nm, tail):
        hit = [f for f in files(sub) if f.startswith(nm + tail)]
        assert len(hit) == 1, (sub, nm, tail, files(sub))
        return str(tmp_path / sub / hit[0])
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'off')])
    t_off, h_off = fitsio.read_table(product('off', name, '_trans.fits'))
    assert not any('fakestars' in f for f in files('off')) and 'FAKE_STAR' not in t_off
    assert not any(k.startswith(('T-FK', 'T-NFAKE', 'T-FAKESN', 'T-NFKTR')) for k in fitsio.read_hdus(product('off', name, '_trans_hdr.fits'), headers_only=True)[0][0])
    cli.main(common + on + ['--image', raws[0], '--red_dir', str(tmp_path / 'on')])
    assert files('on') == sorted(files('off') + [name + '_trans_fakestars.fits'])
    t_on, h_on = fitsio.read_table(product('on', name, '_trans.fits'))
    fk, h_fk = fitsio.read_table(product('on', name, '_trans_fakestars.fits'))
    assert tuple(fk) == G.FAKE_COLS and [c for c in t_on if c != 'FAKE_STAR'] == list(t_off) and t_on['FAKE_STAR'].dtype.kind == 'i'
    hh = fitsio.read_hdus(product('on', name, '_trans_hdr.fits'), headers_only=True)[0][0]
    ok = fk['FLAGS_IN'] == 0
    assert R.hval(hh, 'T-NFAKE') == ok.sum() > 0 and R.hval(hh, 'T-FAKESN') == 30 and R.hval(hh, 'T-FKP') is True and R.hval(h_on, 'T-NFAKE') == ok.sum()
    assert ((fk['FOUND'][ok] & 3) == 3).all() and (t_on['FAKE_STAR'] > 0).sum() == R.hval(hh, 'T-NFKTR') >= ok.sum()
    for tail in ('.fits', '_cat.fits'):
        assert open(product('on', name, tail), 'rb').read() == open(product('off', name, tail), 'rb').read(), tail
    # the list run: the same tables for either frame (the same field twice)
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(raws) + '\n')
    outs = cli.main(common + on + ['--image_list', lst, '--red_dir', str(tmp_path / 'lst')])
    assert len(outs) == 2 and all(outs)
    for k in range(2):
        nm = 'ML1_20240102_03040%d_red' % k
        tb, _ = fitsio.read_table(product('lst', nm, '_trans.fits'))
        fb, _ = fitsio.read_table(product('lst', nm, '_trans_fakestars.fits'))
        assert list(tb) == list(t_on) and list(fb) == list(fk)
        for col in t_on:
            assert tb[col].tobytes() == t_on[col].tobytes(), (k, col)
        for col in fk:
            assert fb[col].tobytes() == fk[col].tobytes(), (k, col)
