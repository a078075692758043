"""GPU: the transient shape fits (bbx_transfit.hip; include/bbx.h: bbx_trans_shapefit) against the numpy restatement of
transshape_ref.py on that file's cases; optimal_subtraction(trans_shapefit=True) end to end on the scene of test_gpu_transfit.py,
with and without trans_psffit; the command line.

Tolerances.  Kernel and restatement both work in float64 on the same float32 window; they differ in the order of their 36 sums and
in the float32 rounding of the kernel's outputs: max(4 x transshape_ref.ORD_*, 2^-22), relative but for positions (absolute, in
units of W / 2 pixels), on the rows both mark converged; flags 1, 2, 4 exactly, flags 8 and 16 on all but 1 % of a case's rows."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import psfphot_ref as PR                      # noqa: E402
import transfit_ref as T                      # noqa: E402
import transshape_ref as TS                   # noqa: E402
import test_transshape_host as TH             # noqa: E402
import test_psfbuild_host as P                # noqa: E402  (the scene)
import test_gpu_match as M                    # noqa: E402
import test_gpu_psfphot as GP                 # noqa: E402  (truth_model)
import test_gpu_transfit as GT                # noqa: E402  (free_spots, same, rows_at, device_sigmas)
from test_gpu_match import ctx                # noqa: E402,F401  (fixture)
from blackbox_amd import reduce as R          # noqa: E402
from blackbox_amd import zogy as G             # noqa: E402
from blackbox_amd._lib import lib             # noqa: E402

F = np.float32
dev = M.dev
BORDER, BOX = GT.BORDER, GT.BOX
CONV = TS.NO_FIT | TS.NOT_CONVERGED
HARD = TS.AT_BOUND | TS.MASKED | TS.NO_FIT
TOL = dict(pos=max(4 * TS.ORD_POS, TS.OUT_ROUND), err=max(4 * TS.ORD_ERR, TS.OUT_ROUND), fwhm=max(4 * TS.ORD_FWHM, TS.OUT_ROUND),
           elong=max(4 * TS.ORD_ELONG, TS.OUT_ROUND), chi2=max(4 * TS.ORD_CHI2, TS.OUT_ROUND))


# ---- bbx_trans_shapefit ---------------------------------------------------------------------------------------------------------
def gpu_fit(ctx, case, sigmas):
    mask = dev(ctx, case['mask']) if case['mask'] is not None else None
    out, flags = G.trans_shapefit(ctx, dev(ctx, case['D']), dev(ctx, case['N']), dev(ctx, case['R']), sigmas[0], sigmas[1], mask,
                                  dev(ctx, case['fwhm0']), case['ys'], case['xs'], case['scal'], TS.SIZE, TS.NSX, fit_size=case['W'],
                                  niter=case['niter'], maxshift=TS.MAXSHIFT, models=case['models'], beta=TS.BETA, fwhm_lo=TS.FWHM_LO)
    ctx.sync()
    return dict(out=out.cpu().numpy(), flags=flags.cpu().numpy())


@pytest.mark.parametrize('spec', TS.CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_fit_meets_the_restatement(ctx, spec):
    case, want = TS.case_run(spec)
    n = len(case['ys'])
    sigmas = GT.device_sigmas(ctx, case, TS.case_of(spec)[1])
    got, again = gpu_fit(ctx, case, sigmas), gpu_fit(ctx, case, sigmas)
    assert got['out'].dtype == np.float32 and got['out'].shape == (2, 7, n) and got['flags'].dtype == np.uint8 and got['flags'].shape == (2, n)
    assert got['out'].tobytes() == again['out'].tobytes() and got['flags'].tobytes() == again['flags'].tobytes()      # two runs, the same bits
    assert np.array_equal(got['flags'] & HARD, want['flags'] & HARD)
    soft = ((got['flags'] ^ want['flags']) & (TS.NOT_CONVERGED | TS.SHAPE_REFUSED)) != 0
    assert soft.sum(axis=1).max() <= 0.01 * n, soft.sum(axis=1)
    fitted = (want['flags'] & TS.NO_FIT) == 0
    assert not got['out'][~np.broadcast_to(fitted[:, None, :], got['out'].shape)].any()
    both = ((got['flags'] & CONV) == 0) & ((want['flags'] & CONV) == 0)
    assert both.sum() >= 0.95 * fitted.sum(), (both.sum(), fitted.sum())
    d = TH.order_distance(want, got, case['W'], both)
    print(spec, '%d fits, %d converged on both sides; ' % (fitted.sum(), both.sum()) + ' '.join('%s %.2e (%.1e)' % (k, d[k], TOL[k]) for k in d))
    for k in d:
        assert d[k] <= TOL[k], (k, d[k], TOL[k])


def test_entry_checks_its_arguments(ctx):
    n = None
    p = torch.zeros(96 * 128, dtype=torch.float32, device=ctx.device).data_ptr()
    sc = np.ones((12, 6), F)
    hs = sc.ctypes.data_as(G.C.POINTER(G.C.c_float))
    m = G.MiniImage(ctx, np.full((6, 8), 5.0, F), 16).ref()

    def call(W=11, ncand=3, sig_n=p, mini_n=n, mini_r=n, niter=32, models=3, beta=2.5, lo=0.5, hi=22.0, maxshift=2.0, D=p, nsx=4):
        return lib.bbx_trans_shapefit(ctx.h, 96, 128, D, p, p, sig_n, p, mini_n, mini_r, n, 12, 32, nsx, hs, p, ncand, p, p, W, niter, maxshift,
                                      models, beta, lo, hi, p, p, ctx.stream())
    assert call(W=10) == -1 and call(W=3) == -1 and call(W=41) == -1 and call(niter=0) == -1 and call(niter=129) == -1
    assert call(mini_n=m, mini_r=m) == -1                            # both sigma forms at once
    assert call(models=-1) == -1 and call(models=4) == -1 and call(beta=1.0) == -1 and call(beta=0.5) == -1
    assert call(lo=3.0, hi=3.0) == -1 and call(lo=4.0, hi=3.0) == -1
    assert call(D=n) == -1 and call(ncand=-1) == -1 and call(maxshift=0.0) == -1 and call(nsx=5) == -1 and call(sig_n=n) == -1
    assert call(ncand=0) == 0 and call(W=39, ncand=0) == 0 and call(niter=128, ncand=0) == 0 and call(models=0) == 0
    ctx.sync()


# ---- optimal_subtraction(trans_shapefit=True) ---------------------------------------------------------------------------------
SHAPE_HDR = ('T-SHAPE', 'T-SHPSZ', 'T-MBETA', 'T-NGAUS', 'T-NMOFF', 'T-FWGMD', 'T-ELGMD')
FIT_HDR = ('T-PSFD', 'T-FITSZ', 'T-NFIT', 'T-PDFOLD', 'T-CHI2MD')
W_E2E = 11


@pytest.fixture(scope='module')
def e2e(ctx):
    """the scene of test_gpu_transfit's end-to-end test: eight point sources of either sign, three single-pixel spikes, three dipoles"""
    rs = np.random.RandomState(5)
    sc, ref = P.make_scene(), P.make_scene(fwhm_ref=3.0)
    new, rimg = np.nan_to_num(sc['img']).astype(np.float64), np.nan_to_num(ref['img']).astype(np.float64)
    spots = GT.free_spots(sc, (new, rimg), 14, rs)
    g = np.arange(P.V) - P.V // 2
    points, spikes, dipoles = [], [], []
    for k, (y, x) in enumerate(spots):
        sl = np.s_[y - P.V // 2:y + P.V // 2 + 1, x - P.V // 2:x + P.V // 2 + 1]
        if k < 8:
            oy, ox = rs.uniform(-0.5, 0.5, 2)
            f = rs.uniform(1.5e4, 6e4)
            if k % 2:
                rimg[sl] += f * PR.moffat(3.0, g[:, None] - oy, g[None, :] - ox)
            else:
                new[sl] += f * P.truth_stamp(x, P.V, oy, ox)
            points.append((y + oy, x + ox, -f if k % 2 else f))
        elif k < 11:
            new[y, x] += rs.uniform(6000, 12000)
            spikes.append((y, x))
        else:
            f = rs.uniform(1e5, 2e5)
            new[sl] += f * P.truth_stamp(x, P.V, 0.35, -0.35 * (k % 2))
            rimg[sl] += f * PR.moffat(3.0, g[:, None] + 0.35, g[None, :] - 0.35 * (k % 2)) / PR.moffat(3.0, g[:, None], g[None, :]).sum()
            dipoles.append((y, x))
    model = GP.truth_model(ctx)
    mask = dev(ctx, sc['mask'])
    d_new, d_ref = dev(ctx, (new + 300.0).astype(F)), dev(ctx, rimg.astype(F))
    psf_ref = dev(ctx, PR.moffat_stamp(P.V, 3.0).astype(F))
    calls = []
    orig = (G.pd_stamps, G._trans_psffit, G._trans_shapefit)

    def counted(f):
        def w(*a, **k):
            calls.append(f.__name__)
            return f(*a, **k)
        return w
    G.pd_stamps, G._trans_psffit, G._trans_shapefit = (counted(f) for f in orig)

    def call(**kw):
        n0 = len(calls)
        res = G.optimal_subtraction(ctx, d_new, d_ref, mask, torch.zeros_like(mask), model, psf_ref, subimage_size=P.SIZE, subimage_border=BORDER,
                                    bkg_boxsize=BOX, ref_is_bkgsub=True, ref_bkg_std_mini=np.full((P.NY // BOX, P.NX // BOX), P.SKY, F),
                                    trans_extract=True, fratio=1.0, thumbnails=True, thumbnail_size=16, **kw)
        ctx.sync()
        return res, calls[n0:]
    try:
        out = dict(plain=call(), off=call(trans_shapefit=False), on=call(trans_shapefit=True), psf=call(trans_psffit=True),
                   both=call(trans_psffit=True, trans_shapefit=True))
        # the bound of the vetting, from the on leg: above the broadest spike, in the gap below the next row
        rows = out['on'][0]['transients']
        ys, xs = [t['y'] for t in rows], [t['x'] for t in rows]
        fw = np.array([t['fwhm_gauss_d'] for t in rows])
        sp = fw[[P.nearest(ys, xs, p[0], p[1], 2.0) for p in spikes]]
        pt = fw[[P.nearest(ys, xs, p[0], p[1], 2.0) for p in points]]
        bound = float(0.5 * (sp.max() + fw[fw > sp.max()].min()))
        out['vet'] = call(trans_shapefit=True, trans_fwhm_gauss_min=bound)
    finally:
        G.pd_stamps, G._trans_psffit, G._trans_shapefit = orig
    out.update(sc=sc, model=model, psf_ref=psf_ref, points=points, spikes=spikes, dipoles=dipoles, bound=bound, fw_spikes=sp, fw_points=pt)
    return out


def test_switch_off_changes_nothing(e2e):
    (a, ca), (b, cb) = e2e['plain'], e2e['off']
    assert ca == [] and cb == []                                     # no kernel of bbx_transfit.hip without the switches
    assert list(a) == list(b)
    GT.same(a, b)
    assert not set(SHAPE_HDR) & set(a['header_trans']) and all('chi2_gauss_d' not in t for t in a['transients'])
    assert e2e['on'][1] == ['trans_shapefit'] and e2e['psf'][1] == ['pd_stamps', 'trans_psffit']
    assert e2e['both'][1] == ['pd_stamps', 'trans_psffit', 'trans_shapefit']    # queued behind the fit of P_D
    # the fit of P_D is what it is without the shape fits
    p, q = e2e['psf'][0], e2e['both'][0]
    assert [{k: v for k, v in t.items() if not k.endswith(('_gauss_d', '_moffat_d'))} for t in q['transients']] == p['transients']
    assert {k: v for k, v in q['header_trans'].items() if k not in SHAPE_HDR} == dict(p['header_trans'])


def test_switch_on_fits_the_candidates(ctx, e2e):
    on, off, both = e2e['on'][0], e2e['off'][0], e2e['both'][0]
    for k in ('D', 'Scorr', 'Fpsf', 'Fpsferr', 'data_bkgsub', 'ref_bkgsub', 'thumbnails'):
        GT.same(off[k], on[k], k)
    ht = on['header_trans']
    assert ht['T-NTRANS'] == off['header_trans']['T-NTRANS'] and ht['T-SHAPE'][0] is True and ht['T-SHPSZ'][0] == W_E2E and ht['T-MBETA'][0] == 2.5
    assert {k: v for k, v in ht.items() if k not in SHAPE_HDR} == dict(off['header_trans']) and not set(FIT_HDR) & set(ht)
    rows = on['transients']
    base = [{k: t[k] for k in off['transients'][0]} for t in rows]
    assert base == off['transients'] and len(base) >= 14
    keys = [n + '_' + m + '_d' for m in ('gauss', 'moffat') for n in ('x', 'xerr', 'y', 'yerr', 'fwhm', 'elong', 'chi2', 'flags')]
    assert list(rows[0])[len(base[0]):] == keys
    # with the fit of P_D queued in front: the same shape fits
    assert [{k: t[k] for k in keys} for t in both['transients']] == [{k: t[k] for k in keys} for t in rows]
    # the restatement on the frames the kernel saw
    nsub = P.NSY * P.NSX
    sub_pn = G.subimage_psfs(ctx, e2e['model'], P.NSY, P.NSX, P.SIZE).cpu().numpy()
    sub_pr = np.repeat(e2e['psf_ref'].cpu().numpy()[None], nsub, 0)
    fwhm0 = np.maximum(TS.fwhm0_of(sub_pn), TS.fwhm0_of(sub_pr))

    def frame(s):
        return (s.frame(ctx) if isinstance(s, G.MiniImage) else s).cpu().numpy()
    ys, xs = np.array([t['y'] for t in rows]), np.array([t['x'] for t in rows])
    want = TS.trans_shapefit_ref(on['D'].cpu().numpy(), on['data_bkgsub'].cpu().numpy(), on['ref_bkgsub'].cpu().numpy(), frame(on['bkg_std']),
                                 frame(on['bkg_std_ref']), e2e['sc']['mask'], ys, xs, on['scal'], fwhm0, P.SIZE, P.NSX, W_E2E)
    jp = np.array(GT.rows_at(on, e2e['points']))
    worst = dict(pos=0.0, fwhm=0.0, elong=0.0, chi2=0.0)
    for mi, m in enumerate(('gauss', 'moffat')):
        got = {k: np.array([t['%s_%s_d' % (k, m)] for t in rows]) for k in ('x', 'xerr', 'y', 'yerr', 'fwhm', 'elong', 'chi2', 'flags')}
        assert np.array_equal(got['flags'] & HARD, want['flags'][mi] & HARD)
        assert not (got['flags'][jp] & CONV).any() and not (want['flags'][mi][jp] & CONV).any()
        o = want['out'][mi][:, jp]
        worst['pos'] = max(worst['pos'], np.abs(got['y'][jp] - (ys[jp] + o[0])).max(), np.abs(got['x'][jp] - (xs[jp] + o[1])).max())
        for k, i in (('fwhm', 4), ('elong', 5), ('chi2', 6)):
            worst[k] = max(worst[k], np.abs(got[k][jp] / o[i] - 1).max())
        # truth: positions within K_SIGMA of the fit's own errors and 0.02 px (the PSF is not the model), the sign of the amplitude
        for j, (y, x, f) in zip(jp, e2e['points']):
            assert abs(got['y'][j] - y) <= TH.K_SIGMA * got['yerr'][j] + 0.02 and abs(got['x'][j] - x) <= TH.K_SIGMA * got['xerr'][j] + 0.02
            assert np.sign(want['amp'][mi][j]) == np.sign(f)
        conv = (got['flags'] & CONV) == 0
        key = 'T-NGAUS' if mi == 0 else 'T-NMOFF'
        assert ht[key][0] == int(conv.sum())
        if mi == 0:
            assert ht['T-FWGMD'][0] == pytest.approx(float(np.median(got['fwhm'][conv]))) and ht['T-ELGMD'][0] == pytest.approx(float(np.median(got['elong'][conv])))
    print('GPU against the restatement on the GPU\'s own D at %d point sources: position %.2e px, FWHM %.2e, ELONG %.2e, chi2 %.2e'
          % (len(jp), worst['pos'], worst['fwhm'], worst['elong'], worst['chi2']))
    # the same inputs but for the sigma maps (the kernel reads them off their mini images: 3e-7) and the order of the sums: the
    # bounds of test_gpu_transfit's end-to-end test
    assert worst['pos'] <= 1e-4 and worst['fwhm'] <= 1e-4 and worst['elong'] <= 1e-4 and worst['chi2'] <= 1e-4
    print('FWHM_GAUSS_D of the spikes %s, of the point sources %s; T-FWGMD %s T-ELGMD %s' % (
        np.round(e2e['fw_spikes'], 2), np.round(e2e['fw_points'], 2), ht['T-FWGMD'][0], ht['T-ELGMD'][0]))


def test_fwhm_bound_drops_spikes_and_thumbnails(e2e):
    """trans_fwhm_gauss_min above the broadest injected spike drops the spikes, the rows without a Gauss fit and whatever else is
    narrower, with their thumbnails.  On this scene that is not a vetting one would use: ZOGY's D gives a single-pixel spike of the
    new frame the shape of the reference's PSF (FWHM 3.0 here) through the same whitening as a point source, and measured on an
    MI355X the three spikes have FWHM_GAUSS_D 2.75, 3.34 and 3.98 against 3.47 .. 4.01 of the eight point sources -- the bound
    that removes the spikes removes seven of those.  The ordering of test_transshape_host.py (spikes 0.56 .. 0.83 against 3.28 ..
    5.17) holds for spikes in D itself, that is for what survives of a cosmic ray under a reference much sharper than the new frame"""
    on, vet = e2e['on'][0], e2e['vet'][0]
    keep = [i for i, t in enumerate(on['transients']) if not t['flags_gauss_d'] & 4 and t['fwhm_gauss_d'] >= e2e['bound']]
    assert 0 < len(keep) < len(on['transients'])
    assert vet['transients'] == [on['transients'][i] for i in keep]
    assert vet['header_trans']['T-NVET'][0] == len(keep) and vet['header_trans']['T-NTRANS'] == on['header_trans']['T-NTRANS']
    assert vet['thumbnails'].shape[0] == len(keep) and torch.equal(vet['thumbnails'], on['thumbnails'][keep])
    assert 'T-NVET' not in on['header_trans']
    ys, xs = [t['y'] for t in vet['transients']], [t['x'] for t in vet['transients']]
    assert all(P.nearest(ys, xs, y, x, 2.0) < 0 for y, x in e2e['spikes'])


# ---- command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_columns_and_keys(tmp_path, ctx):
    """blackbox.py --trans_shapefit True through --image and --image_list on the raw frame of test_gpu_thumbs' command-line test;
    without the switch today's files"""
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
    on = ['--trans_shapefit', 'True', '--trans_shape_size', '9']
    name = 'ML1_20240102_030400_red'
    new_cols = [c[0] for c in catalogs.TRANSSHAPE_COLUMNS]

    def read(sub, nm=name):
        return fitsio.read_table(str(tmp_path / sub / (nm + '_trans.fits')))
    cli.main(common + ['--image', raws[0], '--red_dir', str(tmp_path / 'off')])
    t_off, h_off = read('off')
    assert not set(new_cols) & set(t_off) and not set(SHAPE_HDR) & set(h_off)
    cli.main(common + on + ['--image', raws[0], '--red_dir', str(tmp_path / 'on')])
    t_on, h_on = read('on')
    n = len(t_on['NUMBER'])
    assert n >= 5 and [c for c in t_on if c not in new_cols] == list(t_off) and [c for c in t_on if c in new_cols] == new_cols
    for k in t_off:
        assert t_on[k].tobytes() == t_off[k].tobytes(), k
    assert R.hval(h_on, 'T-SHAPE') is True and R.hval(h_on, 'T-SHPSZ') == 9 and R.hval(h_on, 'T-MBETA') == 2.5 and R.hval(h_on, 'T-NTRANS') == n
    assert 0 < R.hval(h_on, 'T-NGAUS') <= n and 0 < R.hval(h_on, 'T-NMOFF') <= n and R.hval(h_on, 'T-FWGMD') > 0 and R.hval(h_on, 'T-ELGMD') >= 1
    assert 'T-PSFD' not in h_on
    fitted = (t_on['FLAGS_GAUSS_D'] & 4) == 0
    assert fitted.sum() >= 5 and np.abs(t_on['X_GAUSS_D'] - t_on['X_PEAK'])[fitted].max() <= 2.0
    assert (np.abs(t_on['X_GAUSS_D'] - np.rint(t_on['X_GAUSS_D'])) > 1e-3).any() and (t_on['ELONG_GAUSS_D'][fitted] >= 1).all()
    # the list run: the same table for either frame (the same field twice)
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('\n'.join(raws) + '\n')
    outs = cli.main(common + on + ['--image_list', lst, '--red_dir', str(tmp_path / 'lst')])
    assert len(outs) == 2 and all(outs)
    for k in range(2):
        tb, hb = read('lst', 'ML1_20240102_03040%d_red' % k)
        assert list(tb) == list(t_on) and R.hval(hb, 'T-SHAPE') is True
        for col in t_on:
            assert tb[col].tobytes() == t_on[col].tobytes(), (k, col)
