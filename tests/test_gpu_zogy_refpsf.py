"""GPU: prepared reference PSF spectra of bbx_zogy_frame (include/bbx.h, bbx_zogy_refpsf): the spectrum Pr^ of the reference's
PSF stamps made once, into a caller's buffer, beside the prepared rows.  The fill runs the transform the frame call runs on
the same data, and the prepared call does the same arithmetic on the same values, so its five outputs equal those of the
rows-only prepared and of the unprepared call bit for bit -- at the toy sides and at L = 1400 (small grid on and off); spectra
of another stamp tensor, stamp size or geometry, or without rows, are refused; the window guard still fires; and a
FramePipeline makes them once per run."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import test_gpu_zogy_frame as ZF           # noqa: E402  (make, oracle, dev, moffat)
import test_gpu_zogy_refrows as ZR         # noqa: E402  (case, GEOMS: two frames against one reference at the aligned toy sides)
import test_gpu_zogy_spectra as ZS         # noqa: E402  (case: the smallest frame at L = 1400, made once per stamp size)
from blackbox_amd import reduce as R       # noqa: E402
from blackbox_amd import zogy as G          # noqa: E402
from blackbox_amd._lib import lib, BBXError, BBX_OPT_ZOGY_KSMALL_OFF          # noqa: E402

F = np.float32
NAMES = ZR.NAMES
BBX_ERR_ARG = -1


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


def run(ctx, c, k, size, border, rows=None, rpsf=None):
    new, pn, scal = c['frames'][k]
    out = G.run_zogy_frame(ctx, new, c['ref'], c['sn'], c['sr'], pn, c['pr'] if rpsf is None else rpsf.stamps, scal, size, border,
                           want_S=True, ref_rows=rows, ref_psf=rpsf)
    ctx.sync()
    return [o.cpu().numpy() for o in out]


def prepare(ctx, c, size, border):
    ny, nx = c['ref'].shape
    rows = G.RefRows(ctx, c['ref'], c['sr'], size, border)
    rpsf = G.RefPsf(ctx, c['pr'], (ny, nx), size, border)
    assert rpsf.stamps.data_ptr() == c['pr'].data_ptr() and rpsf.S == c['pr'].shape[1]
    assert rpsf.buf.numel() * 4 == lib.bbx_zogy_refpsf_bytes(ny, nx, size, border) > 0
    assert rpsf.matches(c['pr'], (ny, nx), size, border) and not rpsf.matches(c['pr'].clone(), (ny, nx), size, border)
    assert not rpsf.matches(c['pr'], (ny, nx), size, border + 4)
    return rows, rpsf


@pytest.mark.parametrize('form', ['frames', 'mini'])
@pytest.mark.parametrize('geom', ZR.GEOMS)
def test_prepared_psf_equals_rows_only_and_unprepared(ctx, geom, form):
    size, border = geom[0], geom[1]
    c = ZR.case(ctx, geom, form, seed=size + border + 3)
    plain = [run(ctx, c, k, size, border) for k in (0, 1)]
    rows, rpsf = prepare(ctx, c, size, border)
    # two consecutive frames (other pixels, other new PSFs, other scalars) against the one reference
    for k in (0, 1):
        rows_only = run(ctx, c, k, size, border, rows)
        got = run(ctx, c, k, size, border, rows, rpsf)
        for name, g, r, w in zip(NAMES, got, rows_only, plain[k]):
            assert np.array_equal(r, w), (k, name)
            assert np.array_equal(g, w), (k, name, float(np.abs(g - w).max()))
        # and the oracle's run_zogy on every sub-image, at the bound of test_gpu_zogy_refrows.py
        new, pn, scal = c['host'][k]
        want = ZF.oracle(new, c['h_ref'], c['h_sn'], c['h_sr'], pn, c['h_pr'], scal, size, border)
        for name, g, w in zip(NAMES, got, want):
            ok = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), ok), name
            scale = np.abs(w[ok]).max()
            err = np.abs(g[ok] - w[ok]).max()
            print('%s frame %d %s: max |got - oracle| = %.3g = %.3g of max |w|' % (form, k, name, err, err / scale))
            assert err <= 2e-5 * scale, (k, name, err, scale)
    # the setting does not outlive the calls it was made for
    again = run(ctx, c, 0, size, border)
    for g, w in zip(again, plain[0]):
        assert np.array_equal(g, w)


@pytest.mark.parametrize('small', [True, False])
@pytest.mark.parametrize('S', [49, 25])
def test_prepared_psf_equals_unprepared_at_1400(ctx, S, small):
    """the production side: NL = 4 column kernels with 768 threads, the zero-skip of the stamps' transform, and the k_n, k_r
    samples of the 280-point grid (small) or the two inverse transforms of the full grid"""
    at_1400(ctx, ZS.case(ctx, S), small)


def test_prepared_psf_equals_unprepared_at_1400_mini(ctx):
    """the same with the sigma maps read off their mini images: the small grid behind the mini form of the row kernel, unprepared,
    with prepared rows, and with k_img_cols feeding it (prepared PSF)"""
    c = dict(ZS.case(ctx, 25))
    ny, nx, box = ZS.NSY * ZS.SIZE, ZS.NSX * ZS.SIZE, 60
    yy, xx = np.mgrid[0:ny // box, 0:nx // box]
    c['sn'] = G.MiniImage(ctx, (14 + 2 * np.sin(yy / 5.0) * np.cos(xx / 7.0)).astype(F), box, interp_Xchan=True)
    c['sr'] = G.MiniImage(ctx, (6 + np.cos(yy / 6.0 + xx / 9.0)).astype(F), box, interp_Xchan=True)
    assert G.mini_path_supported((ny, nx), ZS.SIZE, ZS.BORDER, box, c['sn'], c['sr'])
    at_1400(ctx, c, True)


def at_1400(ctx, c, small):
    if not small:
        assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KSMALL_OFF, 1) == 0
    try:
        plain = [run(ctx, c, k, ZS.SIZE, ZS.BORDER) for k in (0, 1)]
        rows, rpsf = prepare(ctx, c, ZS.SIZE, ZS.BORDER)
        for k in (0, 1):
            rows_only = run(ctx, c, k, ZS.SIZE, ZS.BORDER, rows)
            got = run(ctx, c, k, ZS.SIZE, ZS.BORDER, rows, rpsf)
            for name, g, r, w in zip(NAMES, got, rows_only, plain[k]):
                assert np.array_equal(r, w, equal_nan=True), (k, name)
                assert np.array_equal(g, w, equal_nan=True), (k, name, float(np.nanmax(np.abs(g - w))))
    finally:
        if not small:
            assert lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KSMALL_OFF, 0) == 0


@pytest.mark.parametrize('form', ['frames', 'mini'])
def test_stale_psf_spectra_are_refused(ctx, form):
    geom = ZR.GEOMS[0]
    size, border, S = geom[0], geom[1], geom[4]
    c = ZR.case(ctx, geom, form, seed=78)
    ny, nx = c['ref'].shape
    plain = run(ctx, c, 0, size, border)
    rows, rpsf = prepare(ctx, c, size, border)
    new, pn, scal = c['frames'][0]
    outs = [torch.empty_like(new) for _ in range(5)]
    sc = np.ascontiguousarray(scal, F)
    MARK = 7.0

    def mark():
        for o in outs:
            o.fill_(MARK)

    def unwritten():
        ctx.sync()
        return all(bool((o == MARK).all()) for o in outs)

    def call(pr, S_=S, border_=border):
        tail = (G._p(pn), G._p(pr), S_, sc.ctypes.data_as(C.POINTER(C.c_float)), *[G._p(o) for o in outs], ctx.stream())
        if form == 'mini':
            return lib.bbx_zogy_frame_mini(ctx.h, ny, nx, size, border_, G._p(new), G._p(c['ref']), c['sn'].ref(), c['sr'].ref(), *tail)
        return lib.bbx_zogy_frame(ctx.h, ny, nx, size, border_, G._p(new), G._p(c['ref']), G._p(c['sn']), G._p(c['sr']), *tail)

    def set_rows(on):
        return lib.bbx_zogy_refrows(ctx.h, G._p(rows.buf) if on else None, ny, nx, size, border, G._p(c['ref']), C.c_void_p(rows.sigma_id()))

    def set_psf(on, size_=size, border_=border, S_=S):
        return lib.bbx_zogy_refpsf(ctx.h, G._p(rpsf.buf) if on else None, ny, nx, size_, border_, G._p(rpsf.stamps), S_)
    other_pr = c['pr'].clone()
    assert set_rows(True) == 0 and set_psf(True) == 0
    try:
        mark()
        assert call(c['pr']) == 0
        ctx.sync()
        for name, g, w in zip(NAMES, outs, plain):
            assert np.array_equal(g.cpu().numpy(), w), name
        mark()
        assert call(other_pr) == BBX_ERR_ARG                              # another stamp tensor (same values)
        assert call(c['pr'], S_=S - 2) == BBX_ERR_ARG                     # another stamp size
        assert call(c['pr'], border_=border + 1) == BBX_ERR_ARG           # another border
        assert unwritten()
        # spectra set for another cut of the frame (56 + 2 * 4 = 64: a supported side with aligned rows) or another stamp size,
        # under rows of the right one: the PSF setting alone refuses the call
        assert set_psf(True, size_=56, border_=4) == 0
        assert call(c['pr']) == BBX_ERR_ARG
        assert set_psf(True, S_=S + 2) == 0
        assert call(c['pr']) == BBX_ERR_ARG
        assert unwritten()
        # a wrong setting is an argument error as well, and leaves nothing set: the call then runs on prepared rows alone
        assert set_psf(True, border_=border + 1) == BBX_ERR_ARG
        assert call(other_pr) == 0
        ctx.sync()
        for name, g, w in zip(NAMES, outs, plain):
            assert np.array_equal(g.cpu().numpy(), w), name
        # a PSF setting without rows
        assert set_psf(True) == 0 and set_rows(False) == 0
        mark()
        assert call(c['pr']) == BBX_ERR_ARG
        assert unwritten()
    finally:
        assert set_psf(False) == 0 and set_rows(False) == 0
    # cleared: any stamp tensor goes, through its own transform
    assert call(other_pr) == 0
    ctx.sync()
    for name, g, w in zip(NAMES, outs, plain):
        assert np.array_equal(g.cpu().numpy(), w), name


def test_small_grid_guard_fires_through_the_prepared_path(ctx):
    """the pair of test_gpu_zogy_spectra.test_small_grid_guard_fires (point-like new PSF, 5 x 5 box reference, very low reference
    noise) with rows and PSF spectra prepared: the step is flagged all the same"""
    S = 5
    c = ZS.case(ctx, 49)
    new, _, scal = c['frames'][0]
    scal = scal.copy()
    nsub = ZS.NSY * ZS.NSX
    pn = np.zeros((nsub, S, S), F); pn[:, 2, 2] = 1.0
    pr = ZF.dev(ctx, np.full((nsub, S, S), 1.0 / 25, F))
    scal[:, 0], scal[:, 1] = 10.0, 0.01
    rows = G.RefRows(ctx, c['ref'], c['sr'], ZS.SIZE, ZS.BORDER)
    rpsf = G.RefPsf(ctx, pr, c['ref'].shape, ZS.SIZE, ZS.BORDER)
    ctx.sync()
    G.run_zogy_frame(ctx, new, c['ref'], c['sn'], c['sr'], ZF.dev(ctx, pn), rpsf.stamps, scal, ZS.SIZE, ZS.BORDER, ref_rows=rows, ref_psf=rpsf)
    with pytest.raises(BBXError) as ei:
        ctx.sync()
    assert ei.value.code == -6
    ctx.sync()                                                   # the flag was cleared


def test_pipeline_makes_the_reference_psf_once(ctx, monkeypatch):
    """the two-lane FramePipeline of test_pipeline_makes_the_reference_rows_once: the reference PSF's spectra are made once for
    the run and shared by the lanes, and every frame's products equal those of a run without them (BBX_REF_PSF=0)"""
    import bbx_oracle as O
    from blackbox_amd import synth
    from blackbox_amd.pipeline import FramePipeline, HostPool
    tel, ys, xs, nframes, lanes = 'ML1', 124, 124, 6, 2
    size, border, box, S = 124, 8, 31, 11
    cases = [synth.make_case(ys, xs, 300 + k, tel=tel, os_y=20, os_x=45, n_stars=40, n_sat=2, n_cr=30) for k in range(nframes)]
    d = ctx.device
    flat = torch.from_numpy(cases[0]['flat']).to(d)
    bpm = torch.from_numpy(cases[0]['bpm']).to(d)
    coeffs = O.xtalk_coeffs(cases[0]['xtalk'])
    raws = [torch.from_numpy(c['raw']).to(d) for c in cases]
    geom = R.geometry(raws[0].shape, ys, xs)
    ny, nx = 2 * ys, 8 * xs
    rs = np.random.RandomState(2)
    ref = ZF.dev(ctx, rs.normal(0, 6, (ny, nx)).astype(F))
    ref_mask = torch.zeros((ny, nx), dtype=torch.uint8, device=d)
    nsub = (ny // size) * (nx // size)
    psf_n = ZF.dev(ctx, np.stack([ZF.moffat(S, 3.4 + 0.02 * k) for k in range(nsub)]))
    psf_r = ZF.dev(ctx, np.stack([ZF.moffat(S, 2.9 + 0.01 * k) for k in range(nsub)]))
    by, bx = np.mgrid[0:ny // box, 0:nx // box]
    sub_kw = dict(ref=ref, ref_mask=ref_mask, psf_new=psf_n, psf_ref=psf_r, fratio=1.0, dx=0.03, dy=0.02, ref_is_bkgsub=True,
                  ref_bkg_std_mini=(6.0 + 0.05 * bx - 0.1 * by).astype(F), subimage_size=size, subimage_border=border, bkg_boxsize=box)
    keys = ('D', 'Scorr', 'Fpsf', 'Fpsferr')

    def pipeline_run(expect_psf):
        pool = HostPool(4)
        fills0 = G.RefPsf.fills
        pipe = FramePipeline(ctx, tel, geom, mflat=flat, bpm=bpm, xtalk_coeffs=coeffs, exptime=60.0, pool=pool, depth=3, do_finish=True,
                             keep_outputs=True, lanes=lanes, subtract=sub_kw)
        got = {}

        def done(idx, f):
            assert not f.failed, f.failed
            got[idx] = {k: f.sub[k].clone() for k in keys}
        try:
            n = pipe.run([(r, {}) for r in raws], on_done=done)
            torch.cuda.synchronize()
            assert pipe.ref_rows is not None
            assert (pipe.ref_psf is not None) == expect_psf
            if expect_psf:
                assert pipe.ref_psf.psf_ref is psf_r and pipe.ref_psf.S == S
        finally:
            pipe.close()
            pool.close()
        assert n == nframes and sorted(got) == list(range(nframes))
        return got, G.RefPsf.fills - fills0
    monkeypatch.setenv('BBX_REF_PSF', '0')
    without, fills = pipeline_run(False)
    assert fills == 0
    monkeypatch.delenv('BBX_REF_PSF')
    with_psf, fills = pipeline_run(True)
    assert fills == 1                                                    # once for the run: not per frame, not per lane
    for k in range(nframes):
        for key in keys:
            assert torch.equal(with_psf[k][key], without[k][key]), (k, key)
