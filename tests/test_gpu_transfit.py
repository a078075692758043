"""GPU: transient vetting (bbx_transfit.hip; include/bbx.h: bbx_zogy_pd_stamps, bbx_trans_psffit) against the numpy restatement of
transfit_ref.py on that file's cases; optimal_subtraction(trans_psffit=True) end to end on the scene of test_psfbuild_host.py with
transients, spikes and a dipole injected; the command line.

Tolerances.  P_D: transfit_ref.PD_TOL of the stamp's peak (kernel and restatement both work in float64; the stamp is rounded to
float32).  The fit: 4 x transfit_ref.D32_*, the float32 restatement's own largest distance from the float64 one on these very cases
(test_transfit_host.test_float32_follows_float64), relative to the float64 value (dy, dx: absolute, in pixels); flags exactly."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import psfphot_ref as PR                      # noqa: E402
import transfit_ref as T                      # noqa: E402
import test_transfit_host as TH               # noqa: E402
import test_psfbuild_host as P                # noqa: E402  (the scene)
import test_gpu_match as M                    # noqa: E402
import test_gpu_psfphot as GP                 # noqa: E402  (truth_model)
from test_gpu_match import ctx                # noqa: E402,F401  (fixture)
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402
from blackbox_amd._lib import lib             # noqa: E402

F = np.float32
dev = M.dev
BORDER, BOX = 12, 20
OUT = ('flux', 'err', 'dy', 'dx', 'chi2', 'flags')


# ---- bbx_zogy_pd_stamps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', T.PD_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_pd_stamps_meet_the_restatement(ctx, spec):
    S, Mg, nsub = spec
    c = T.make_pd_case(*spec)
    want, wfold = T.pd_stamps_ref(c['pn'], c['pr'], c['scal'], Mg)
    runs = []
    for _ in range(2):
        pd, fold = G.pd_stamps(ctx, dev(ctx, c['pn']), dev(ctx, c['pr']), c['scal'], M=Mg)
        ctx.sync()
        runs.append((pd.cpu().numpy(), fold.cpu().numpy()))
    (pd, fold), (pd2, fold2) = runs
    assert pd.dtype == np.float32 and pd.shape == (nsub, S, S) and fold.shape == (nsub,)
    assert pd.tobytes() == pd2.tobytes() and fold.tobytes() == fold2.tobytes()
    dead = [k for k in range(nsub) if not want[k].any()]
    assert len(dead) == (2 if nsub > 1 else 0)
    worst = 0.0
    for k in range(nsub):
        if k in dead:
            assert not pd[k].any() and fold[k] == 1.0
            continue
        worst = max(worst, float(np.abs(pd[k] - want[k]).max() / want[k].max()))
        assert abs(fold[k] - wfold[k]) <= T.FOLD_TOL * wfold[k] + 1e-12, (k, fold[k], wfold[k])
    print(spec, 'largest |P_D - restatement| / peak %.2e (tolerance %.1e)' % (worst, T.PD_TOL))
    assert worst <= T.PD_TOL


def test_pd_entry_checks_its_arguments(ctx):
    p = torch.zeros(12 * 49 * 49, dtype=torch.float32, device=ctx.device).data_ptr()
    sc = np.ones((12, 6), F)
    hs = sc.ctypes.data_as(G.C.POINTER(G.C.c_float))

    def call(nsub=12, S_=21, Mg=128, pn=p, scal=hs):
        return lib.bbx_zogy_pd_stamps(ctx.h, nsub, S_, Mg, pn, p, scal, p, p, ctx.stream())
    assert call(S_=20) == -1 and call(S_=51) == -1 and call(Mg=80) == -1 and call(Mg=129) == -1 and call(Mg=1024) == -1
    assert call(pn=None) == -1 and call(scal=None) == -1 and call(nsub=-1) == -1
    assert call(nsub=0) == 0
    ctx.sync()


# ---- bbx_trans_psffit -----------------------------------------------------------------------------------------------------------
def device_sigmas(ctx, case, frames):
    if case['sig_form'] == 'frame':
        return dev(ctx, frames[0]), dev(ctx, frames[1])
    x = case['sig_form'] == 'mini_x'
    return G.MiniImage(ctx, case['mini_n'], T.BOX, interp_Xchan=x), G.MiniImage(ctx, case['mini_r'], T.BOX, interp_Xchan=x)


def gpu_fit(ctx, case, sigmas):
    mask = dev(ctx, case['mask']) if case['mask'] is not None else None
    out = G.trans_psffit(ctx, dev(ctx, case['D']), dev(ctx, case['N']), dev(ctx, case['R']), sigmas[0], sigmas[1], mask, dev(ctx, case['pd']),
                         case['ys'], case['xs'], case['scal'], T.SIZE, T.NSX, fit_size=case['W'], niter=T.NITER, maxshift=T.MAXSHIFT)
    ctx.sync()
    return dict(zip(OUT, [o.cpu().numpy() for o in out]))


@pytest.mark.parametrize('spec', T.CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_fit_meets_the_restatement(ctx, spec):
    case, want, _ = TH.case_runs(spec)
    sigmas = device_sigmas(ctx, case, T.sigma_frames(case))
    got, again = gpu_fit(ctx, case, sigmas), gpu_fit(ctx, case, sigmas)
    for k in OUT:
        assert got[k].dtype == (np.uint8 if k == 'flags' else np.float32)
        assert got[k].tobytes() == again[k].tobytes(), k             # two runs, the same bits
    assert np.array_equal(got['flags'], want['flags'])
    ok = (want['flags'] & T.NO_FIT) == 0
    for k in OUT[:5]:
        assert not got[k][~ok].any()
    d = {k: float(np.abs(got[k][ok].astype(np.float64) / want[k][ok] - 1).max()) for k in ('flux', 'err', 'chi2')}
    d['pos'] = max(float(np.abs(got['dy'] - want['dy']).max()), float(np.abs(got['dx'] - want['dx']).max()))
    print(spec, 'flux %.2e (%.1e) err %.2e (%.1e) chi2 %.2e (%.1e) dy, dx %.2e px (%.1e)'
          % (d['flux'], 4 * T.D32_FLUX, d['err'], 4 * T.D32_ERR, d['chi2'], 4 * T.D32_CHI2, d['pos'], 4 * T.D32_POS))
    assert d['flux'] <= 4 * T.D32_FLUX and d['err'] <= 4 * T.D32_ERR and d['chi2'] <= 4 * T.D32_CHI2 and d['pos'] <= 4 * T.D32_POS


def test_fit_entry_checks_its_arguments(ctx):
    n = None
    p = torch.zeros(96 * 128, dtype=torch.float32, device=ctx.device).data_ptr()
    sc = np.ones((12, 6), F)
    hs = sc.ctypes.data_as(G.C.POINTER(G.C.c_float))

    def call(S_=21, W=11, D=p, ncand=3, sig_r=p, niter=8, maxshift=2.0, nsx=4):
        return lib.bbx_trans_psffit(ctx.h, 96, 128, D, p, p, p, sig_r, n, n, n, S_, 12, p, 32, nsx, hs, ncand, p, p, W, niter, maxshift,
                                    p, p, p, p, p, p, ctx.stream())
    assert call(W=10) == -1 and call(W=13) == -1 and call(W=1) == -1 and call(S_=51) == -1 and call(S_=20) == -1
    assert call(D=n) == -1 and call(ncand=-1) == -1 and call(sig_r=n) == -1 and call(niter=0) == -1 and call(maxshift=0.0) == -1
    assert call(nsx=5) == -1
    assert call(ncand=0) == 0
    ctx.sync()


# ---- optimal_subtraction(trans_psffit=True) -------------------------------------------------------------------------------------
def free_spots(sc, imgs, n, rs, gap=14, apart=32):
    """n integer positions at least [gap] px from every star of the scene, [apart] px from each other (the region above the
    threshold around a source of 10^5 e- is some 10 px wide, and two regions that touch make one row), 20 px from the frame's edge,
    with nothing above 6 sigma of the sky within 10 px in either frame (the scene's hand-made sources)"""
    out = []
    sy, sx = np.asarray(sc['sy']), np.asarray(sc['sx'])
    for y, x in rs.permutation([(y, x) for y in range(20, P.NY - 20, 7) for x in range(20, P.NX - 20, 7)]):
        if any(np.abs(im[y - 10:y + 11, x - 10:x + 11]).max() >= 6 * P.SKY for im in imgs):
            continue
        if np.hypot(sy - y, sx - x).min() >= gap and all(max(abs(y - a), abs(x - b)) >= apart for a, b in out):
            out.append((int(y), int(x)))
            if len(out) == n:
                return out
    raise AssertionError('scene too crowded')


@pytest.fixture(scope='module')
def e2e(ctx):
    rs = np.random.RandomState(5)
    sc, ref = P.make_scene(), P.make_scene(fwhm_ref=3.0)
    new, rimg = np.nan_to_num(sc['img']).astype(np.float64), np.nan_to_num(ref['img']).astype(np.float64)
    spots = free_spots(sc, (new, rimg), 14, rs)
    g = np.arange(P.V) - P.V // 2
    points, spikes, dipoles = [], [], []
    for k, (y, x) in enumerate(spots):
        sl = np.s_[y - P.V // 2:y + P.V // 2 + 1, x - P.V // 2:x + P.V // 2 + 1]
        if k < 8:                                                    # point sources of the new frame's own PSF, both signs
            oy, ox = rs.uniform(-0.5, 0.5, 2)
            f = rs.uniform(1.5e4, 6e4)
            if k % 2:
                rimg[sl] += f * PR.moffat(3.0, g[:, None] - oy, g[None, :] - ox)     # a star of the reference that is gone
            else:
                new[sl] += f * P.truth_stamp(x, P.V, oy, ox)
            points.append((y + oy, x + ox, -f if k % 2 else f))
        elif k < 11:
            new[y, x] += rs.uniform(6000, 12000)                    # single-pixel spikes, 600 sigma and up
            spikes.append((y, x))
        else:                                                        # a star 0.7 px apart in the two frames
            f = rs.uniform(1e5, 2e5)
            new[sl] += f * P.truth_stamp(x, P.V, 0.35, -0.35 * (k % 2))
            rimg[sl] += f * PR.moffat(3.0, g[:, None] + 0.35, g[None, :] - 0.35 * (k % 2)) / PR.moffat(3.0, g[:, None], g[None, :]).sum()
            dipoles.append((y, x))
    model = GP.truth_model(ctx)
    mask = dev(ctx, sc['mask'])
    d_new, d_ref = dev(ctx, (new + 300.0).astype(F)), dev(ctx, rimg.astype(F))
    psf_ref = dev(ctx, PR.moffat_stamp(P.V, 3.0).astype(F))
    calls = []
    orig = (G.pd_stamps, G._trans_psffit)

    def counted(f):
        def w(*a, **k):
            calls.append(f.__name__)
            return f(*a, **k)
        return w
    G.pd_stamps, G._trans_psffit = counted(orig[0]), counted(orig[1])

    def call(**kw):
        res = G.optimal_subtraction(ctx, d_new, d_ref, mask, torch.zeros_like(mask), model, psf_ref, subimage_size=P.SIZE, subimage_border=BORDER,
                                    bkg_boxsize=BOX, ref_is_bkgsub=True, ref_bkg_std_mini=np.full((P.NY // BOX, P.NX // BOX), P.SKY, F),
                                    trans_extract=True, fratio=1.0, thumbnails=True, thumbnail_size=16, **kw)
        ctx.sync()
        return res
    try:
        plain = call()
        off = call(trans_psffit=False)
        n_off = len(calls)
        on = call(trans_psffit=True)
        n_on = len(calls) - n_off
        vet = call(trans_psffit=True, trans_chi2_max=4.0)
    finally:
        G.pd_stamps, G._trans_psffit = orig
    return dict(sc=sc, model=model, psf_ref=psf_ref, plain=plain, off=off, on=on, vet=vet, n_off=n_off, n_on=n_on, points=points, spikes=spikes,
                dipoles=dipoles)


def same(a, b, key=''):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), key
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    elif isinstance(a, dict):
        assert list(a) == list(b), key
        for k in a:
            same(a[k], b[k], key + '/' + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, key + '/' + str(i))
    elif isinstance(a, (int, float, str, bool, type(None), np.generic)):
        assert a == b or (a != a and b != b), key
    # (objects that hold device state -- MiniImage, RefCatalog -- carry nothing a product is made of)


def test_switch_off_changes_nothing(e2e):
    a, b = e2e['plain'], e2e['off']
    assert e2e['n_off'] == 0 and e2e['n_on'] == 2                    # one call of each entry with the switch on, none without
    assert list(a) == list(b)
    same(a, b)
    assert 'T-PSFD' not in a['header_trans'] and all('chi2_psf_d' not in t for t in a['transients'])


def rows_at(res, pos, dmax=2.0):
    ys, xs = [t['y'] for t in res['transients']], [t['x'] for t in res['transients']]
    out = []
    for p in pos:
        j = P.nearest(ys, xs, p[0], p[1], dmax)
        assert j >= 0, (p, float(np.hypot(np.asarray(ys) - p[0], np.asarray(xs) - p[1]).min()))
        out.append(j)
    return out


def test_switch_on_fits_the_candidates(ctx, e2e):
    on, off = e2e['on'], e2e['off']
    for k in ('D', 'Scorr', 'Fpsf', 'Fpsferr', 'data_bkgsub', 'ref_bkgsub', 'thumbnails'):
        same(off[k], on[k], k)
    ht = on['header_trans']
    assert ht['T-NTRANS'] == off['header_trans']['T-NTRANS'] and ht['T-PSFD'][0] is True and ht['T-FITSZ'][0] == 11
    assert {k: v for k, v in ht.items() if k not in ('T-PSFD', 'T-FITSZ', 'T-NFIT', 'T-PDFOLD', 'T-CHI2MD')} == dict(off['header_trans'])
    base = [{k: t[k] for k in off['transients'][0]} for t in on['transients']]
    assert base == off['transients'] and len(base) >= 14
    # the restatement on the frames the kernel saw
    nsub = P.NSY * P.NSX
    sub_pn = G.subimage_psfs(ctx, e2e['model'], P.NSY, P.NSX, P.SIZE).cpu().numpy()
    sub_pr = np.repeat(e2e['psf_ref'].cpu().numpy()[None], nsub, 0)
    pd, fold = T.pd_stamps_ref(sub_pn, sub_pr, on['scal'], 256, np.float32)
    assert ht['T-PDFOLD'][0] == pytest.approx(float(fold.max()), rel=1e-5) and ht['T-PDFOLD'][0] < T.PD_FOLD_WARN

    def frame(s):
        return (s.frame(ctx) if isinstance(s, G.MiniImage) else s).cpu().numpy()
    rows = on['transients']
    ys, xs = np.array([t['y'] for t in rows]), np.array([t['x'] for t in rows])
    want = T.trans_psffit_ref(on['D'].cpu().numpy(), on['data_bkgsub'].cpu().numpy(), on['ref_bkgsub'].cpu().numpy(), frame(on['bkg_std']),
                              frame(on['bkg_std_ref']), e2e['sc']['mask'], pd, ys, xs, on['scal'], P.SIZE, P.NSX, 11, 8, 2.0, np.float32)
    got = {k: np.array([t[k] for t in rows]) for k in ('y_psf_d', 'x_psf_d', 'flux_psf_d', 'fluxerr_psf_d', 'chi2_psf_d', 'flags_psf_d')}
    jp = rows_at(on, e2e['points'])
    good = np.array([j for j in jp])
    assert not got['flags_psf_d'][good].any() and not want['flags'][good].any()
    dpos = max(np.abs(got['y_psf_d'][good] - (ys[good] + want['dy'][good])).max(), np.abs(got['x_psf_d'][good] - (xs[good] + want['dx'][good])).max())
    dflux = np.abs(got['flux_psf_d'][good] / want['flux'][good] - 1).max()
    dchi = np.abs(got['chi2_psf_d'][good] / want['chi2'][good] - 1).max()
    print('GPU against the restatement on the GPU\'s own D at %d point sources: position %.2e px, flux %.2e, chi2 %.2e' % (len(good), dpos, dflux, dchi))
    # the same inputs but for the sigma maps (the kernel reads them off their mini images: 3e-7) and the order of the sums
    assert dpos <= 1e-4 and dflux <= 1e-5 and dchi <= 1e-4
    # truth: positions within 5 of the restatement's own errors (test_transfit_host.K_SIGMA), the sign of the flux
    for j, (y, x, f) in zip(jp, e2e['points']):
        assert abs(got['y_psf_d'][j] - y) <= TH.K_SIGMA * want['dy_err'][j] + 0.02 and abs(got['x_psf_d'][j] - x) <= TH.K_SIGMA * want['dx_err'][j] + 0.02
        assert np.sign(got['flux_psf_d'][j]) == np.sign(f)
    # the chi2 ordering of the host test
    top = got['chi2_psf_d'][good].max()
    art = got['chi2_psf_d'][rows_at(on, e2e['spikes']) + rows_at(on, e2e['dipoles'], 6.0)]       # (a dipole's lobes peak some 3 px from its centre in Scorr)
    print('largest chi2 of a point source %.2f; spikes and dipoles %s; T-CHI2MD %s T-NFIT %s' % (top, np.round(art, 1), ht['T-CHI2MD'][0], ht['T-NFIT'][0]))
    assert art.min() > top
    nfit = int(((got['flags_psf_d'] & 12) == 0).sum())
    assert ht['T-NFIT'][0] == nfit and ht['T-CHI2MD'][0] == pytest.approx(float(np.median(got['chi2_psf_d'][(got['flags_psf_d'] & 12) == 0])))


def test_chi2_bound_drops_rows_and_thumbnails(e2e):
    on, vet = e2e['on'], e2e['vet']
    keep = [i for i, t in enumerate(on['transients']) if not t['flags_psf_d'] & 4 and t['chi2_psf_d'] <= 4.0]
    assert 0 < len(keep) < len(on['transients'])
    assert vet['transients'] == [on['transients'][i] for i in keep]
    assert vet['header_trans']['T-NVET'][0] == len(keep) and vet['header_trans']['T-NTRANS'] == on['header_trans']['T-NTRANS']
    assert vet['thumbnails'].shape[0] == len(keep) and torch.equal(vet['thumbnails'], on['thumbnails'][keep])
    assert 'T-NVET' not in on['header_trans']


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_columns_and_keys(tmp_path, ctx):
    """blackbox.py --trans_psffit True through --image and --image_list on the raw frame of test_gpu_thumbs' command-line test
    (PSF stamps of 15: --trans_fit_size 5); --trans_chi2_max drops rows and their thumbnails; without the switch today's files"""
    import test_gpu_thumbs as TT
    from blackbox_amd import catalogs, fitsio, synth
    import bbx_oracle as O
    cli = TT.load_cli()
    YS, XS, TEL = TT.YS, TT.XS, TT.TEL
    case = synth.make_case(YS, XS, 77, tel=TEL, os_y=20, os_x=45, n_stars=60, n_sat=2, n_cr=40)
    hdr = {'EXPTIME': 60.0, 'IMAGETYP': 'object', 'FILTER': 'q'}
    raw_new = case['raw'].astype(np.float64)
    dx = raw_new.shape[1] // 8
    star = TT.moffat_stamp(15, 3.5).astype(np.float64)
    for y, x, peak in ((60, 100, 1500.0), (30, dx + 200, 800.0), (9, 3 * dx + 40, 2500.0), (100, 5 * dx + 290, 1200.0), (75, 7 * dx + 150, 600.0)):
        raw_new[y - 7:y + 8, x - 7:x + 8] += peak * star / star.max()
    raw_new[50, 2 * dx + 100] += 20000.0                             # a single-pixel spike
    raw_new = np.clip(np.rint(raw_new), 0, 65535).astype(case['raw'].dtype)
    raws = []
    for k in range(2):
        raws.append(str(tmp_path / ('ML1_raw%d.fits' % k)))
        fitsio.write_image(raws[-1], raw_new, dict(hdr, **{'DATE-OBS': '2024-01-02T03:04:0%d' % k}))
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
              '--subimage_size', '120', '--subimage_border', '10', '--bkg_boxsize', '30', '--save_thumbnails', 'True']
    on = ['--trans_psffit', 'True', '--trans_fit_size', '5']
    name = 'ML1_20240102_030400_red'
    new_cols = [c[0] for c in catalogs.TRANSFIT_COLUMNS]

    def read(sub, nm=name):
        t, h = fitsio.read_table(str(tmp_path / sub / (nm + '_trans.fits')))
        return t, h, h
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'off')])
    t_off, h_off, _ = read('off')
    assert not set(new_cols) & set(t_off) and 'T-PSFD' not in h_off
    cli.main(common + on + ['--image', raws[0], '--red_dir', str(tmp_path / 'on')])
    t_on, h_on, _ = read('on')
    n = len(t_on['NUMBER'])
    thumbs = [c for c in t_off if c.startswith('THUMBNAIL_')]
    assert n >= 5 and [c for c in t_on if c not in new_cols] == list(t_off) and [c for c in t_on if c in new_cols] == new_cols
    for k in t_off:
        assert t_on[k].tobytes() == t_off[k].tobytes(), k
    assert R.hval(h_on, 'T-PSFD') is True and R.hval(h_on, 'T-FITSZ') == 5 and R.hval(h_on, 'T-NTRANS') == n
    assert 0 < R.hval(h_on, 'T-NFIT') <= n and R.hval(h_on, 'T-PDFOLD') < T.PD_FOLD_WARN and R.hval(h_on, 'T-CHI2MD') > 0
    fitted = (t_on['FLAGS_PSF_D'] & 4) == 0
    assert fitted.sum() >= 5 and np.abs(t_on['X_PSF_D'] - t_on['X_PEAK'])[fitted].max() <= 2.0 and (np.abs(t_on['X_PSF_D'] - np.rint(t_on['X_PSF_D'])) > 1e-3).any()
    # the bound: between the chi2 of the injected stars and the spike's
    chi = np.sort(t_on['CHI2_PSF_D'][fitted])
    bound = float(np.sqrt(chi[len(chi) // 2] * chi[-1]))
    keep = fitted & (t_on['CHI2_PSF_D'] <= bound)
    assert 0 < keep.sum() < n
    cli.main(common + on + ['--trans_chi2_max', repr(bound), '--image', raws[0], '--red_dir', str(tmp_path / 'vet')])
    t_v, h_v, _ = read('vet')
    assert len(t_v['NUMBER']) == keep.sum() and R.hval(h_v, 'T-NVET') == keep.sum() and R.hval(h_v, 'T-NTRANS') == n
    for k in t_on:
        if k != 'NUMBER':
            assert t_v[k].tobytes() == t_on[k][keep].tobytes(), k
    assert thumbs and t_v[thumbs[0]].shape[0] == keep.sum()
    # the list run: the same table for either frame (the same field twice)
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(raws) + '\n')
    outs = cli.main(common + on + ['--image_list', lst, '--red_dir', str(tmp_path / 'lst')])
    assert len(outs) == 2 and all(outs)
    for k in range(2):
        tb, hb, _ = read('lst', 'ML1_20240102_03040%d_red' % k)
        assert list(tb) == list(t_on) and R.hval(hb, 'T-PSFD') is True
        for col in t_on:
            assert tb[col].tobytes() == t_on[col].tobytes(), (k, col)
