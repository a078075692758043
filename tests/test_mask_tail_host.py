"""Host: the scenes of tests/mask_tail_ref.py take the paths of bbx_mask_finish they are meant to take.

Everything here is asserted on the oracle's result alone (O.mask_init on the frame that tests/test_gpu_mask_tail.py
sends through the GPU, same builder call, same seed); mask_tail_ref.Decomposition restates the kernel's 64 x 64 tile
decomposition to say which tiles the coarse stage (k_coarse_cc / k_coarse_flood) must leave to the pixel flood
(k_fine_flood).  These are conditions, not measurements: a scene that misses one at a geometry has to change."""
import numpy as np
import pytest
from scipy import ndimage

import bbx_oracle as O
import mask_tail_ref as M

ALL = sorted(M.GEOMS)


@pytest.fixture(scope='module')
def decomp():
    cache = {}

    def get(name):
        if name not in cache:
            cs = M.case(name)
            cache[name] = M.Decomposition(cs['mask'], cs['bpm'])
        return cache[name]
    return get


@pytest.mark.parametrize('name', ALL)
def test_geometry_conditions(name, decomp):
    ny, nx = M.shape_of(name)
    W, TH = (nx + 63) // 64, (ny + 63) // 64
    assert (W, TH) == M.TILES[name] == (decomp(name).W, decomp(name).TH)
    assert W * TH <= M.COARSE_MAX                                  # bbx_mask_finish: (size_t)W * TH > COARSE_MAX -> BBX_ERR_ARG
    assert M.OS_Y > 10 and M.OS_X > 6                              # bbx_make_dims
    if name == 'A':
        assert 64 < W <= 128 and nx % 64 == 32                     # two-word tile rows, half last word
    if name == 'B':
        assert W == M.CF_MAX and (W + 63) // 64 == 4 and nx % 64 and ny % 64     # four words, partial last word and tile row
    if name == 'C':
        assert 128 < TH <= 192                                     # three waves of 64 tile rows in the run-id scan
    if name == 'D':
        assert W > 64 and TH > 64
    if name in 'ABCD':
        assert W <= M.CF_MAX and TH <= M.CF_MAX                    # k_coarse_cc
    if name == 'E':
        assert W > M.CF_MAX and TH <= M.CF_MAX                     # k_coarse_flood, wide
    if name == 'F':
        assert TH > M.CF_MAX and W <= M.CF_MAX                     # k_coarse_flood, tall


@pytest.mark.parametrize('name', ALL)
def test_queue_capacity(name):
    cs = M.case(name)
    nsat = int(((cs['mask'] & 4) != 0).sum())
    assert nsat == int(cs['planted'].sum())
    npix = cs['planted'].size
    assert nsat <= npix // 8 + 4096                                # bbx_calibrate's saturated-pixel queue
    assert nsat < 2 ** 22                                          # bbx_cc_count_list's cap in bbx_mask_finish
    assert cs['nobj'] > 100


@pytest.mark.parametrize('name', ALL)
def test_structures_do_not_overlap(name):
    """no two scenes come within 4 px of each other: the closing (reach 2 px from each side) never joins them"""
    parts = M.case(name)['parts']
    ids = np.zeros(M.shape_of(name), np.int8)
    for k, p in enumerate(parts.values()):
        assert not ids[p].any()
        ids[p] = k + 1
    hi = ndimage.maximum_filter(ids, size=5)                        # the scenes within 2 px of a pixel: all the same one
    lo = ndimage.minimum_filter(np.where(ids > 0, ids, np.int8(127)), size=5)
    assert not ((hi > 0) & (lo != hi)).any()
    assert set(parts) == set(M.SCENES)


@pytest.mark.parametrize('name', ALL)
def test_each_scene_takes_its_path(name, decomp):
    D = decomp(name)
    boxes = M.boxes(M.shape_of(name))
    st = {k: D.stats(b) for k, b in boxes.items()}
    for k in sorted(st):
        print(name, k, boxes[k], st[k])
    # big_rings and the sealed serpentine: a coarse stage that resolves a tile it must not leaves a hole unfilled
    rings = [k for k in st if k.startswith('ring_')]
    assert {'ring_nested', 'ring_edge'} <= set(rings)
    for k in rings + ['serp_shut']:
        assert st[k]['unresolved_empty'] >= 1 and st[k]['holes'] > 10 ** 4, k
    # the open serpentine: nothing inside is a hole; one free-tile component winds through it
    assert st['serp_open']['holes'] == 0 and st['serp_open']['free_span'] >= 6
    assert st['serp_shut']['free_span'] >= 6
    # the pinholes: empty tiles the coarse stage cannot resolve, and not a hole: the pixel flood has to get in
    for k in ('pinhole_x', 'pinhole_y'):
        assert st[k]['holes'] == 0 and st[k]['unresolved_empty'] >= 1, k
    # their twins: the closing seals the gap, at the seam, and the interior is a hole
    for k, seam in (('pinhole_x_shut', 'added_x_seam'), ('pinhole_y_shut', 'added_y_seam')):
        assert st[k]['holes'] > 10 ** 4 and st[k]['unresolved_empty'] >= 1 and st[k][seam] > 0, k
    # sparse: bad pixels inside holes (they keep their 1)
    assert st['sparse']['bad_in_hole'] >= 1 and st['sparse']['holes'] > 0
    # where the rings lie (mask_tail_ref's docstring)
    ny, nx = M.shape_of(name)
    if name == 'D':
        y0, y1, x0, x1 = boxes['ring_edge']
        assert x0 < 4095 and x1 > 4097 and y0 // 64 != y1 // 64
    if max(ny, nx) >= 8800:
        y0, y1, x0, x1 = boxes['ring_word']
        assert (x0 < 8191 and x1 > 8193) or (y0 < 8191 and y1 > 8193)
    if name == 'C':                                                # holes with empty tiles in each wave of the run-id scan
        un = (~D.outside & ~D.occ).any(axis=1)
        assert un[:64].any() and un[64:128].any() and un[128:].any()
    if name == 'B':                                                # holes with empty tiles in every word of a free-tile row
        un = (~D.outside & ~D.occ).any(axis=0)                     # (A, D: tile column 64 is the border column, never in a hole)
        assert un[:64].any() and un[64:128].any() and un[128:192].any() and un[192:].any()
    # the whole frame: far below the pixel flood's iteration bound, every count as the sum of its parts
    allst = D.stats()
    assert allst['holes'] >= sum(s['holes'] for s in st.values())
    assert 0 < allst['unresolved'] < D.W * D.TH


@pytest.mark.parametrize('name', ALL)
def test_seams_join_across_words_and_tiles(name):
    """the seams scene alone: the closing adds pixels at X % 64 in {0, 63} and at Y % 64 in {0, 63}, and leaves the
    pairs that are 6 px apart alone"""
    p = M.case(name)['parts']['seams']
    m = ndimage.binary_dilation(p, structure=M.STRUCT8)
    closed = ndimage.binary_closing(m, structure=M.STRUCT8)
    ys, xs = np.nonzero(closed & ~m)
    assert np.isin(xs % 64, (0, 63)).sum() > 0 and np.isin(ys % 64, (0, 63)).sum() > 0
    for off in (0, 63):
        assert (xs % 64 == off).any() and (ys % 64 == off).any(), off
    ny, nx = p.shape
    # next to the first word / tile, the last word / tile row and the borders
    assert ((xs > 56) & (xs < 76)).any() and ((ys > 56) & (ys < 76)).any()
    assert (xs >= nx - 8).any() and (ys >= ny - 8).any()
    if nx % 64:
        assert ((xs >= nx - nx % 64 - 4) & (xs < nx - nx % 64 + 8)).any()
    if ny % 64:
        assert ((ys >= ny - ny % 64 - 4) & (ys < ny - ny % 64 + 8)).any()
    if nx > 4200:
        assert ((xs > 4088) & (xs < 4108)).any()
    # every first-member offset 60..67 is there, in X and in Y
    py, px = np.nonzero(p)
    assert set(range(60, 68)) <= set(px.tolist()) and set(range(60, 68)) <= set(py.tolist())
    # some pairs are joined, some are not: the number of objects drops, but not to one per pair
    n_before = ndimage.label(m, structure=M.STRUCT8)[1]
    n_after = ndimage.label(closed, structure=M.STRUCT8)[1]
    assert n_after < n_before


@pytest.mark.parametrize('name', ALL)
def test_oracle_is_consistent_with_its_own_prefill_mask(name):
    """O.mask_init == O.fill_sat_holes applied to its own pre-fill mask; without the crosstalk flags that pre-fill
    mask is the planted plane (4) and its ring (8) over the bad-pixel mask, i.e. frame() plants what it says"""
    cs = M.case(name)
    mask = cs['mask']
    sat = (mask & 4) != 0
    ring = ndimage.binary_dilation(sat, structure=M.STRUCT8) & ~sat
    pre = mask.copy()
    pre[(mask == 8) & ~ring] = 0
    assert np.array_equal(pre & 0xBF, M.prefill_mask(cs['planted'], cs['bpm']))
    again = pre.copy()
    O.fill_sat_holes(again)
    assert np.array_equal(again, mask)
    # bad pixels inside holes keep their value
    bad_in_hole = (cs['bpm'] == 1) & ndimage.binary_fill_holes(ndimage.binary_closing(sat | ring, structure=M.STRUCT8),
                                                               structure=M.STRUCT8) & ~sat & ~ring
    assert bad_in_hole.sum() > 0 and ((mask[bad_in_hole] & 8) == 0).all() and ((mask[bad_in_hole] & 1) == 1).all()


@pytest.mark.parametrize('name', ['A', 'E'])
@pytest.mark.parametrize('scene', ['empty', 'single'])
def test_nothing_to_fill(name, scene):
    """empty: every tile is resolved by the coarse stage, the tile list is empty and k_fine_flood / k_fill_apply see a
    zero work count.  single: the one occupied tile is the whole list (an occupied tile is never resolved), nothing is
    added by the closing and nothing is a hole."""
    cs = M.case(name, scene)
    D = M.Decomposition(cs['mask'])
    st = D.stats()
    assert cs['nobj'] == (0 if scene == 'empty' else 1) == int(cs['planted'].sum())
    assert st['unresolved'] == (0 if scene == 'empty' else 1)
    assert st['unresolved_empty'] == 0 and st['holes'] == 0 and not D.added.any()
    assert int(((cs['mask'] & 8) != 0).sum()) == (0 if scene == 'empty' else 8)


def test_frame_plants_what_it_is_given():
    ysz, xsz = 40, 24
    rs = np.random.RandomState(5)
    planted = rs.random_sample((2 * ysz, 8 * xsz)) < 0.02
    raw, got = M.frame(ysz, xsz, M.OS_Y, M.OS_X, planted)
    assert raw.dtype == np.float32 and raw.shape == (2 * (ysz + M.OS_Y), 8 * (xsz + M.OS_X))
    assert np.array_equal(got, planted) and (raw > 0).sum() == planted.sum()
    secs = O.define_sections(raw.shape, ysz, xsz)
    for c in range(16):
        assert np.array_equal(raw[secs[1][c]] > 0, planted[secs[4][c]])
        assert not raw[secs[2][c]].any() and not raw[secs[3][c]].any()        # overscan strips stay zero
    assert np.array_equal(M.reduced(raw, ysz, xsz) > 9e5, planted)
    with pytest.raises(ValueError):
        M.frame(ysz, xsz, 10, M.OS_X, planted)
    with pytest.raises(ValueError):
        M.frame(ysz, xsz, M.OS_Y, 6, planted)
