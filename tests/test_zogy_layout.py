"""The layout of the subtraction code: one module per stage under blackbox_amd/, zogy the facade over them.  Every name the
one-file zogy.py had still resolves on blackbox_amd.zogy, to the very object that lives in its new home; every stage module
imports on its own; the pointer and tensor checks have one definition."""
import importlib
import inspect
import os
import re
import subprocess
import sys

import pytest

from blackbox_amd import _lib, reduce, zogy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'blackbox_amd')

# vars(blackbox_amd.zogy) of the one-file module, without dunders and standard-library module objects other than C
NAMES = ['ALIGN_CLIP', 'ALIGN_DET', 'ALIGN_FAR', 'ALIGN_FEW_PAIRS', 'ALIGN_NMIN', 'ALIGN_NOT_PD', 'ALIGN_PAIR_CAP', 'ALIGN_VOTE_FAILED',
         'BBX_ERR_NOTCONV', 'BBX_ERR_OVERFLOW', 'BBX_ERR_PSFWIN', 'BBX_OPT_ZOGY_KSMALL_OFF', 'BBX_OPT_ZOGY_KWIN_OFF', 'C', 'MATCH_COLS',
         'MiniImage', 'NPAD', 'PD_FOLD_WARN', 'PHOT_MASKED', 'PHOT_NO_CENTROID', 'PHOT_NO_SUM', 'PSF_REASONS', 'RefCatalog', 'RefPsf', 'RefRows',
         'RefStars', 'SHAPE_COLS', 'SHAPE_GAUSS', 'SHAPE_MOFFAT', 'SHAPE_OUT', 'SHAPE_STAT_COLS', 'SPLINE_POLE', 'StreamGate', 'TRANS_AT_BOUND',
         'TRANS_MASKED', 'TRANS_NOT_CONVERGED', 'TRANS_NO_FIT', 'TRANS_SHAPE_REFUSED', '_HeaderView', '_MATCH_HDR', '_MC', '_NoGate', '_PSF_HDR',
         '_SC', '_SHAPE_HDR', '_SplineImage', '_axis_map', '_bspline_weights', '_device_taps', '_expect_list', '_lib_BBXError', '_objmask_counts',
         '_objmask_stage', '_optimal_subtraction', '_p', '_source_sigma', '_tap_tables', '_trans_psffit', '_trans_shapefit', 'align_apply',
         'align_fit', 'align_grid', 'align_grid_host', 'align_grid_shape', 'align_header', 'align_reference', 'align_sort', 'align_vote',
         'build_psf', 'check', 'cut_subimages', 'device_zoom_coefficients', 'embed_psfs', 'empty_match_table', 'empty_shape_table', 'fetch',
         'find_peaks_arrays', 'find_peaks_collect', 'find_peaks_enqueue', 'find_transients', 'format_cat', 'frame_clipped_stats',
         'frame_clipped_stats_enqueue', 'frame_path_supported', 'get_back', 'lib', 'match_enqueue', 'match_mutual', 'match_scalars',
         'match_stats', 'mini2back', 'mini_path_supported', 'ndimage', 'np', 'object_mask', 'object_mask_enqueue', 'optimal_subtraction',
         'pd_stamps', 'psf_chi2', 'psf_chi2_median', 'psf_fit', 'psf_header', 'psf_model_stamps', 'psf_ncoef', 'psf_optflux',
         'psf_optflux_centroid', 'psf_poly_terms', 'psf_select', 'psf_stamps', 'push', 'remap_mask', 'remap_mini', 'resample_psf_basis',
         'run_zogy', 'run_zogy_frame', 'settings', 'shape_columns', 'shape_header', 'shape_start_fwhm', 'shape_stats', 'source_psfs',
         'src_shapes', 'stitch_subimages', 'subimage_psfs', 'thumbnail_stamps', 'tile_index', 'torch', 'trans_fit_header', 'trans_psffit',
         'trans_shape_header', 'trans_shapefit', 'transient_table', 'variance', 'vet_transients', 'win_centroid', 'window_sigma',
         'zogy_frame_outputs', 'zoom_coefficients', 'zoom_plan']

# where every moved definition lives now
HOMES = {
    'zoom': ['_bspline_weights', '_axis_map', '_tap_tables', 'zoom_coefficients', 'zoom_plan', '_device_taps', 'SPLINE_POLE', 'NPAD',
             'device_zoom_coefficients', 'mini2back', 'MiniImage', 'remap_mini'],
    'background': ['get_back', 'object_mask_enqueue', '_objmask_counts', 'object_mask', '_objmask_stage', 'variance',
                   'frame_clipped_stats_enqueue', 'frame_clipped_stats'],
    'peaks': ['find_transients', 'find_peaks_enqueue', 'find_peaks_collect', 'find_peaks_arrays', 'window_sigma', 'win_centroid'],
    'shapes': ['SHAPE_COLS', 'SHAPE_STAT_COLS', '_SC', 'src_shapes', 'empty_shape_table', 'shape_stats', 'shape_columns', '_SHAPE_HDR',
               'shape_header'],
    'psfphot': ['psf_poly_terms', 'resample_psf_basis', 'psf_model_stamps', 'embed_psfs', 'subimage_psfs', 'tile_index', 'source_psfs',
                '_source_sigma', 'psf_optflux', 'PHOT_NO_CENTROID', 'PHOT_MASKED', 'PHOT_NO_SUM', 'psf_optflux_centroid'],
    'transients': ['PD_FOLD_WARN', 'TRANS_AT_BOUND', 'TRANS_MASKED', 'TRANS_NO_FIT', 'TRANS_NOT_CONVERGED', 'TRANS_SHAPE_REFUSED', 'SHAPE_GAUSS',
                   'SHAPE_MOFFAT', 'SHAPE_OUT', 'pd_stamps', 'trans_psffit', 'trans_fit_header', 'trans_shapefit', 'shape_start_fwhm',
                   'trans_shape_header', 'vet_transients', 'thumbnail_stamps'],
    'subtract': ['mini_path_supported', 'cut_subimages', 'stitch_subimages', 'run_zogy', 'frame_path_supported', 'zogy_frame_outputs', 'RefRows',
                 'RefPsf', 'run_zogy_frame', 'StreamGate', '_NoGate'],
    'starmatch': ['MATCH_COLS', '_MC', 'match_mutual', 'empty_match_table', 'match_stats', '_MATCH_HDR', 'match_scalars', 'RefCatalog',
                  'match_enqueue'],
    'psfbuild': ['BBX_ERR_NOTCONV', 'PSF_REASONS', '_PSF_HDR', 'psf_ncoef', 'psf_select', 'psf_stamps', 'psf_fit', 'psf_chi2', 'psf_chi2_median',
                 'psf_header', 'build_psf'],
    'align': ['ALIGN_PAIR_CAP', 'ALIGN_NMIN', 'ALIGN_FAR', 'ALIGN_CLIP', 'ALIGN_VOTE_FAILED', 'ALIGN_FEW_PAIRS', 'ALIGN_NOT_PD', 'ALIGN_DET',
              '_expect_list', 'align_vote', 'align_fit', 'align_apply', 'align_sort', 'align_grid_shape', 'align_grid', 'align_grid_host',
              'remap_mask', 'RefStars', 'align_header', 'align_reference'],
}
STAYS = ['optimal_subtraction', '_optimal_subtraction', '_HeaderView']
MODULES = ['_args'] + sorted(HOMES) + ['zogy']


def test_every_old_name_resolves():
    missing = [n for n in NAMES if not hasattr(zogy, n)]
    assert not missing, missing


def test_home_table_covers_the_old_definitions():
    """the table leaves nothing out: every old name is in a home, stays in zogy, or is an import zogy always had"""
    imports = {'C', 'np', 'torch', 'ndimage', 'settings', 'lib', 'check', 'fetch', 'push', '_p', '_lib_BBXError', '_SplineImage', 'format_cat',
               'transient_table', 'BBX_OPT_ZOGY_KSMALL_OFF', 'BBX_ERR_OVERFLOW', 'BBX_ERR_PSFWIN', 'BBX_OPT_ZOGY_KWIN_OFF', '_trans_psffit',
               '_trans_shapefit'}
    moved = [n for names in HOMES.values() for n in names]
    assert len(moved) == len(set(moved))
    assert set(moved) | set(STAYS) | imports == set(NAMES)


@pytest.mark.parametrize('module', sorted(HOMES))
def test_home(module):
    mod = importlib.import_module('blackbox_amd.' + module)
    for name in HOMES[module]:
        obj = getattr(mod, name)
        assert getattr(zogy, name) is obj, name
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__ == 'blackbox_amd.' + module, name


def test_orchestration_stays():
    for name in STAYS:
        assert getattr(zogy, name).__module__ == 'blackbox_amd.zogy'
    # the switches _optimal_subtraction calls by these names (tests that count calls assign them)
    assert zogy._trans_psffit is zogy.trans_psffit and zogy._trans_shapefit is zogy.trans_shapefit
    assert '_trans_psffit' in vars(zogy) and '_trans_shapefit' in vars(zogy) and 'pd_stamps' in vars(zogy)


def test_orchestration_is_a_list_of_stage_functions():
    """_optimal_subtraction calls module-level functions of zogy.py that share one state object: no closure, no nonlocal"""
    import ast
    import textwrap
    assert 'nonlocal' not in open(os.path.join(PKG, 'zogy.py')).read()
    tree = ast.parse(textwrap.dedent(inspect.getsource(zogy._optimal_subtraction)))
    nested = [getattr(n, 'name', 'lambda') for n in ast.walk(tree.body[0])
              if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)) and n is not tree.body[0]]
    assert nested == []


@pytest.mark.parametrize('module', MODULES)
def test_imports_alone(module):
    """no hidden cycle or order dependence: each module imports first in a fresh interpreter"""
    r = subprocess.run([sys.executable, '-c', 'import blackbox_amd.' + module], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_one_definition():
    assert reduce._ptr is zogy._p is _lib.ptr
    assert reduce._expect is _lib.expect
    sources = {f: open(os.path.join(PKG, f)).read() for f in sorted(os.listdir(PKG)) if f.endswith('.py')}
    for f, text in sources.items():
        assert not re.search(r'^\s+from \.reduce import .*\b_expect\b', text, re.M), f + ': function-level import of _expect'
        if f != '_lib.py':
            assert not re.search(r'^def (_?ptr|_p|_?expect)\(', text, re.M), f + ': a second definition'
