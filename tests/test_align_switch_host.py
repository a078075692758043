"""Registration of the reference from its stars, host side of the switch (no GPU): the clamped tile index, the settings, the
command line's mapping onto the subtraction's keywords, the A-* header keys."""
import importlib.util
import os
import types

import numpy as np
import pytest

import test_align_host as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_cli():
    spec = importlib.util.spec_from_file_location('bbx_cli_align', os.path.join(ROOT, 'blackbox.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def kernel_rule(y, x, size, nsy, nsx):
    """bbx_match.hip, k_win_centroid: ty = min(max(yc / size, 0), nsy - 1), tx likewise (C division, non-negative peaks)"""
    return min(max(int(y) // size, 0), nsy - 1) * nsx + min(max(int(x) // size, 0), nsx - 1)


def test_tile_index_clamps_as_the_kernels_do():
    torch = pytest.importorskip('torch')
    from blackbox_amd import zogy as G
    size = 120
    # a frame that is no multiple of the tile: the reference of the toy scene, 320 x 600 = 2 x 5 tiles and a strip of 80 rows
    ny, nx = A.RNY, A.RNX
    nsy, nsx = ny // size, nx // size
    yy, xx = np.meshgrid(np.arange(0, ny, 7), np.arange(0, nx, 11), indexing='ij')
    ys, xs = np.append(yy.ravel(), [ny - 1, 240, 239]), np.append(xx.ravel(), [nx - 1, 0, 599])
    got = G.tile_index(ys, xs, size, nsy, nsx)
    assert np.array_equal(got, [kernel_rule(y, x, size, nsy, nsx) for y, x in zip(ys, xs)])
    assert got.min() == 0 and got.max() == nsy * nsx - 1                 # never past the stamps
    unclamped = (ys // size) * nsx + xs // size
    assert (unclamped >= nsy * nsx).any() and (got[ys >= nsy * size] == unclamped[ys >= nsy * size] - nsx).all()
    t = G.tile_index(torch.from_numpy(ys.astype(np.int32)), torch.from_numpy(xs.astype(np.int32)), size, nsy, nsx)
    assert np.array_equal(t.numpy(), got)
    # an exact multiple: the index is what it was
    ny, nx = 240, 480
    yy, xx = np.meshgrid(np.arange(ny), np.arange(0, nx, 3), indexing='ij')
    ys, xs = yy.ravel(), xx.ravel()
    assert np.array_equal(G.tile_index(ys, xs, size, 2, 4), (ys // size) * 4 + xs // size)
    t = G.tile_index(torch.from_numpy(ys.astype(np.int32)), torch.from_numpy(xs.astype(np.int32)), size, 2, 4)
    assert np.array_equal(t.numpy(), (ys // size) * 4 + xs // size)
    with pytest.raises(ValueError):
        G.tile_index(ys, xs, size, 0, 4)


def test_settings_defaults():
    from blackbox_amd import settings as S
    assert S.ref_align is False
    assert (S.align_poldeg, S.align_max_shift, S.align_bin, S.align_nbright, S.align_rounds) == (1, 256.0, 4.0, 2048, 3)
    assert (S.align_max_shift, S.align_bin, S.align_nbright, S.align_rounds) == (A.MAX_SHIFT, A.BIN, A.NBRIGHT, A.ROUNDS)


def subtraction_keywords(cli, argv):
    """Reducer._load_subtraction_inputs on a stand-in for the reducer: what the command line hands to optimal_subtraction"""
    a = cli.build_parser().parse_args(argv)
    me = types.SimpleNamespace(args=a, tel='ML1', _load_psf=lambda path: ('psf', path), torch=None, ctx=None, fitsio=None,
                               _build_ref_psf=lambda sub: None)
    return cli.Reducer._load_subtraction_inputs(me, lambda path, dtype, what: (what, path))


BASE = ['--telescope', 'ML1', '--image', 'x.fits', '--trans_extract', 'True', '--ref', 'ref.fits', '--ref_mask', 'refmask.fits',
        '--psf_new', 'pn.fits', '--psf_ref', 'pr.fits']


def test_command_line_passes_the_keywords_only_when_switched_on():
    cli = load_cli()
    off = subtraction_keywords(cli, BASE)
    assert not [k for k in off if k.startswith('align') or k == 'ref_align']
    # the flags alone do not switch it on
    off2 = subtraction_keywords(cli, BASE + ['--align_poldeg', '2', '--align_bin', '16'])
    assert off2 == off
    on = subtraction_keywords(cli, BASE + ['--ref_align', 'True'])
    assert {k: v for k, v in on.items() if k not in off} == dict(ref_align=True, align_poldeg=1, align_max_shift=256.0, align_bin=4.0,
                                                                 align_nbright=2048, align_rounds=3)
    assert {k: on[k] for k in off} == off
    on = subtraction_keywords(cli, BASE + ['--ref_align', 'True', '--align_poldeg', '2', '--align_max_shift', '100', '--align_bin', '16'])
    assert (on['align_poldeg'], on['align_max_shift'], on['align_bin']) == (2, 100.0, 16.0)
    # without a reference there is nothing to register
    none = subtraction_keywords(cli, ['--telescope', 'ML1', '--image', 'x.fits', '--trans_extract', 'True', '--ref_align', 'True'])
    assert 'ref_align' not in none


def test_degree_three_is_refused():
    cli = load_cli()
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(BASE + ['--ref_align', 'True', '--align_poldeg', '3'])
    from blackbox_amd import settings as S
    with pytest.raises(ValueError):
        cli.align_keywords(types.SimpleNamespace(align_poldeg=3, align_max_shift=None, align_bin=None), S, 'ML1')


def test_header_of_a_fit():
    from blackbox_amd import zogy as G
    fit = dict(coef=A.true_coef(), n_used=153, rms_x=0.085, rms_y=0.087, flags=0, info=np.array([167, 62, 58, 73, 167, 0, 167, 30]))
    h = G.align_header(fit, (A.NY, A.NX), 1, 4321)
    dy, dx, rot = A.true_shift()
    assert h['A-P'][0] is True
    assert abs(h['A-DX'][0] - dx) <= 1e-9 and abs(h['A-DY'][0] - dy) <= 1e-9
    assert abs(h['A-ROT'][0] - A.ROT_DEG) <= 1e-9 and abs(h['A-ROT'][0] - rot) <= 1e-9 and abs(h['A-SCALE'][0] - A.SCALE) <= 1e-9
    assert [h[k][0] for k in ('A-PLDG', 'A-NVOTE', 'A-NRUN', 'A-NFAR', 'A-NPAIR', 'A-RMSX', 'A-RMSY', 'A-FLAGS', 'A-NEDGE')] == \
        [1, 167, 62, 30, 153, 0.085, 0.087, 0, 4321]
    assert list(h) == ['A-P', 'A-PLDG', 'A-NVOTE', 'A-NRUN', 'A-NFAR', 'A-NPAIR', 'A-RMSX', 'A-RMSY', 'A-DX', 'A-DY', 'A-ROT', 'A-SCALE',
                       'A-FLAGS', 'A-NEDGE']
    # a non-square frame, another rotation and scale: the linear part is read in pixels, not in the basis' units
    shape = (300, 700)
    h = G.align_header(dict(fit, coef=A.true_coef(shape, -1.3, 0.98, (160.0, 340.0))), shape, 1, 0)
    assert abs(h['A-ROT'][0] + 1.3) <= 1e-9 and abs(h['A-SCALE'][0] - 0.98) <= 1e-9
    assert abs(h['A-DX'][0] - 10.0) <= 1e-9 and abs(h['A-DY'][0] + 10.0) <= 1e-9


def test_header_of_a_failed_registration():
    from blackbox_amd import zogy as G
    keys = ['A-PLDG', 'A-NVOTE', 'A-NRUN', 'A-NFAR', 'A-NPAIR', 'A-RMSX', 'A-RMSY', 'A-DX', 'A-DY', 'A-ROT', 'A-SCALE', 'A-FLAGS', 'A-NEDGE']
    h = G.align_header(None)
    assert h['A-P'][0] is False and [h[k][0] for k in keys] == ['None'] * len(keys)
    bad = dict(coef=np.full(12, np.nan), n_used=3, rms_x=np.nan, rms_y=np.nan, flags=3, info=np.zeros(8, int))
    h = G.align_header(bad, (A.NY, A.NX), 1, None)
    assert h['A-P'][0] is False and h['A-FLAGS'][0] == 3
    assert [h[k][0] for k in keys if k != 'A-FLAGS'] == ['None'] * (len(keys) - 1)
    for v, c in h.values():
        assert isinstance(c, str) and len(c) <= 47                   # a FITS comment that fits its card


def test_library_rejects_bad_arguments_without_gpu():
    from blackbox_amd import _lib
    L = _lib.lib
    assert L.bbx_align_vote_bytes(2048, 256.0, 4.0, 8192) > 129 * 129 * 4 and L.bbx_align_vote_bytes(0, 256.0, 4.0, 8192) == 0
    assert L.bbx_align_vote(None, 0, None, None, None, None, 0, None, None, None, None, 2048, 256.0, 4.0, 15, 8, 8192, None, 0, None, None, None,
                            None) == -1
    assert L.bbx_align_fit(None, 0, None, None, None, None, None, 0, None, None, None, None, None, 0, None, 240, 480, 1, 20.0, 3.0, 15, None,
                           None, None, None) == -1
    assert L.bbx_align_apply(None, 0, None, None, None, None, 240, 480, 1, None, None, None, None) == -1
    assert L.bbx_align_grid(None, None, 240, 480, 32, 9, 16, None, None) == -1
    assert L.bbx_remap_mask(None, 50, 81, None, 50, 81, None, 3, 4, 32, 32, None, None, None) == -1
