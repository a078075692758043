"""CPU: the scenes of tests/lacosmic_paths.py are on the paths they are meant for.  The oracle alone says
what is flagged; the host model of k_lac_cand_v4's queue discipline says which tile, which queue and which
list every raw candidate goes through.  A recipe (or a retuned constant) that drifts off its path fails
here, before anyone needs a GPU for tests/test_gpu_lacosmic_paths.py."""
import numpy as np
import pytest

import lacosmic_paths as P

PARAMS = list(P.PARAMS)


def test_tiling_constants_are_the_ones_the_scenes_were_laid_out_for():
    assert P.device_constants() == {'CAND_SPAN': 248, 'CAND_ROWS': 16, 'CAND_TILECAP': 64, 'CAND_WQ': 512}
    # the spill test of the kernel, `wcand + 256 > CAND_WQ`, as the model states it
    assert P.CAND_WQ - 256 == P.CAND_ROWMAX


def test_prune_threshold():
    assert P.prune_threshold(15.0) == np.float32(2) * np.float32(15) * np.sqrt(np.float32(np.float32(8.2) * np.float32(8.2))) \
        * (np.float32(1) - np.float32(1e-5))
    assert 245.9 < P.prune_threshold(15.0) < 246.0 and 73.79 < P.prune_threshold(4.5) < 73.8


def test_model_on_a_hand_made_tile():
    """three rows of 100 candidates in one tile: the queue holds 300 > 256 after the third and is spilled;
    a fourth row of 70 stays: q = 0 first, 64 to the segment, 6 to the overflow list"""
    img = np.full((16, 248), 100, np.float32)
    for j in (3, 5, 7):
        img[j, 4:204:2] += 3000
    img[9, 8:148:2] += 3000
    path = P.travel(img, 15.0)
    assert (path[[3, 5, 7]] == P.SPILLED).sum() == 300 and (path == P.SPILLED).sum() == 300
    assert (path[9] == P.SEGMENT).sum() == 64 and (path[9] == P.OVERFLOW).sum() == 6
    # even columns: q = 0 (35 pixels) before q = 2; the last six of q = 2 overflow
    assert all(path[9, i] == P.SEGMENT for i in range(8, 148, 4))
    assert [i for i in range(10, 148, 4) if path[9, i] == P.OVERFLOW] == list(range(126, 148, 4))
    assert P.tile_counts(path, 0, 0) == {'spilled': 300, 'segment': 64, 'overflow': 6}


@pytest.mark.parametrize('sigclip,sigfrac', PARAMS)
@pytest.mark.parametrize('name', P.SCENES)
def test_planted_pixels_are_flagged(name, sigclip, sigfrac):
    niter = 6 if name == 'bars' else 3
    cr = P.oracle(name, sigclip, sigfrac, niter, masked=False)[0]
    assert cr.shape == P.SHAPES[name] and cr.sum() > 0
    for p in P.PLANTED[name]:
        assert cr[p], p
    # with the mask the GPU frames carry: the same, but for the hit under the masked columns 0..2
    mask = P.make_mask(name)
    assert (mask[:, :3] & 32).all() and (mask & 1).sum() >= 2 and not (mask[:, 3:] & 32).any()
    crm = P.oracle(name, sigclip, sigfrac, niter)[0]
    assert crm.sum() > 0 and not (crm & (mask != 0)).any()
    for p in P.PLANTED[name]:
        assert mask[p] in (0, 32) and crm[p] == (mask[p] == 0), p
    # every planted pixel is a raw candidate of the dense pass, masked or not
    raw = P.raw_candidates(P.make_scene(name), sigclip)
    assert all(raw[p] for p in P.PLANTED[name])


@pytest.mark.parametrize('sigclip,sigfrac', PARAMS)
def test_frame_rule_and_ragged_tiles(sigclip, sigfrac):
    """hits on the first legal row / column of every border; last tile row of one row, last wave of 4 columns"""
    assert P.SHAPES['tiny'] == (8, 8)                                    # the smallest frame the entry point takes
    ny, nx = P.SHAPES['one_tile']
    assert (ny, nx) == (P.CAND_ROWS, P.CAND_SPAN) and nx % 4 == 0
    assert {(2, 2), (ny - 3, nx - 3)} <= set(P.PLANTED['one_tile'])       # rows 2 and ny-3, columns 2 and nx-3
    ny, nx = P.SHAPES['sliver']
    assert ny - P.CAND_ROWS == 1 and nx - P.CAND_SPAN == 4 and nx % 4 == 0
    path = P.travel(P.make_scene('sliver'), sigclip)
    assert not path[P.CAND_ROWS:].any()                                  # the second tile row is border only
    assert P.tile_counts(path, 0, 1)['segment'] >= 3                     # (14,248), (14,249), (2,249): the 4-column wave
    assert path[14, 248] and path[14, 249] and path[2, 249] and path[8, 247]
    assert {(2, 2), (14, 249), (2, 249)} <= set(P.PLANTED['sliver'])     # nx - 3 = 249, ny - 3 = 14
    # a hit in the frame itself is no candidate, whatever its height
    img = P.make_scene('tiny')
    img[1, 4] += 30000; img[4, 6] += 30000; img[6, 3] += 30000; img[3, 1] += 30000
    assert P.raw_candidates(img, sigclip).sum() == len(P.PLANTED['tiny'])


@pytest.mark.parametrize('sigclip,sigfrac', PARAMS)
def test_seams_hits_sit_on_both_sides_of_every_seam(sigclip, sigfrac):
    ny, nx = P.SHAPES['seams']
    assert ny == 3 * P.CAND_ROWS and nx == 3 * P.CAND_SPAN and nx % 4 == 0
    hits = set(P.PLANTED['seams'])
    # pairs across a tile corner (last row and lane of one tile, first of the next), and pairs one pixel
    # inside the last / first producing lane on either side of both wave seams
    for k in (1, 2):
        y, x = k * P.CAND_ROWS, k * P.CAND_SPAN
        assert {(y - 1, x - 1), (y, x)} <= hits
        assert any({(j, x - 2), (j, x + 1)} <= hits for j in range(ny))
    assert {(2, 2), (ny - 3, nx - 3)} <= hits
    tiles = {P.tile_of(*p) for p in P.PLANTED['seams']}
    assert {(0, 0), (1, 1), (1, 2), (2, 2), (1, 0)} <= tiles
    cols = {i % P.CAND_SPAN for (_, i) in P.PLANTED['seams']}
    assert {P.CAND_SPAN - 1, 0, 1, P.CAND_SPAN - 2} <= cols              # last / first producing lanes of a wave
    rows = {j % P.CAND_ROWS for (j, _) in P.PLANTED['seams']}
    assert {P.CAND_ROWS - 1, 0} <= rows
    path = P.travel(P.make_scene('seams'), sigclip)
    assert all(path[p] == P.SEGMENT for p in P.PLANTED['seams'])
    assert not (path == P.SPILLED).any() and not (path == P.OVERFLOW).any()


@pytest.mark.parametrize('sigclip,sigfrac', PARAMS)
def test_dense_tile_spills_fills_its_segment_and_overflows(sigclip, sigfrac):
    ny, nx = P.SHAPES['dense']
    assert ny % P.CAND_ROWS == 8 and nx % 4 == 0 and nx > 2 * P.CAND_SPAN       # ragged last tile row of 8 rows
    assert all(P.tile_of(j, i) == P.DENSE_TILE for j in P.DENSE_ROWS for i in P.DENSE_COLS)
    img = P.make_scene('dense')
    path = P.travel(img, sigclip)
    cr = P.oracle('dense', sigclip, sigfrac, 3)[0]
    n = P.tile_counts(path, *P.DENSE_TILE)
    print('dense, sigclip %g: raw candidates of the tile %r, CR pixels %d' % (sigclip, n, cr.sum()))
    assert sum(n.values()) >= 567 and n['spilled'] > P.CAND_ROWMAX and n['segment'] == P.CAND_TILECAP and n['overflow'] >= 20
    ncr = P.tile_counts(path, *P.DENSE_TILE, within=cr)
    assert min(ncr.values()) >= 20, ncr
    assert cr.sum() >= 500
    # candidates (and CR pixels) in the ragged tile row and in a second and third wave
    assert path[2 * P.CAND_ROWS:].any() and cr[2 * P.CAND_ROWS:].any()
    assert path[:, P.CAND_SPAN:2 * P.CAND_SPAN].any() and path[:, 2 * P.CAND_SPAN:].any()


@pytest.mark.parametrize('sigclip,sigfrac', PARAMS)
@pytest.mark.parametrize('name', ['bars', 'streaks'])
def test_bars_flag_new_pixels_in_every_iteration(name, sigclip, sigfrac):
    """what drives k_lac_cand_sparse up to the sixth iteration"""
    cr, _, iters, _ = P.oracle(name, sigclip, sigfrac, 6)
    print(name, sigclip, iters)
    assert len(iters) == 6 and all(n > 0 for n in iters)
    assert P.oracle(name, sigclip, sigfrac, 1)[2] == iters[:1]
    path = P.travel(P.make_scene(name), sigclip)
    assert (path == P.SPILLED).any() and (path == P.OVERFLOW).any()
    if name == 'streaks':
        # same shape as `dense`; streaks inside the lattice's tile, one across column 248 and row 32
        assert P.SHAPES['streaks'] == P.SHAPES['dense']
        assert sum(P.tile_of(r0, c0) == P.DENSE_TILE == P.tile_of(r0 + 4, c1 - 1) for (r0, c0, c1) in P.STREAKS) >= 2
        assert any(c0 < P.CAND_SPAN < c1 and r0 < 2 * P.CAND_ROWS <= r0 + 4 for (r0, c0, c1) in P.STREAKS)
        for tj, ti in ((1, 0), (1, 1), (2, 0), (2, 1)):
            assert min(P.tile_counts(path, tj, ti, within=cr)[k] for k in ('segment', 'overflow')) > 0


def test_chain_pixels_can_only_be_queued_by_the_sparse_pass():
    """the B pixels of `chain<k>` are no candidates of the dense pass and are flagged in the second iteration,
    and no pixel next to one can be a stage-2 pixel of the first (s <= sigclip there, and sp <= s): iteration 1
    neither sets nor clears their byte of the flag plane.  Over the phases every pixel of the region is a B
    exactly once."""
    sigclip, sigfrac = 15.0, 0.01
    cover = np.zeros(P.SHAPES['bars'], int)
    for k in range(P.NCHAIN):
        name = 'chain%d' % k
        assert P.SHAPES[name] == P.SHAPES['bars']
        B = P.chain_pixels(k)
        raw = P.raw_candidates(P.make_scene(name), sigclip)
        s = P.first_iteration_s(name)
        cr1 = P.oracle(name, sigclip, sigfrac, 1)[0]
        cr3, _, iters, _ = P.oracle(name, sigclip, sigfrac, 3)
        assert len(B) == 4 and iters[0] > 0 and iters[1] >= len(B) and iters[2] == 0
        for (j, i) in B:
            cover[j, i] += 1
            assert not raw[j, i] and not cr1[j, i] and cr3[j, i], (name, j, i)
            assert cr1[j, i - 1] and cr1[j, i + 1] and cr1[j, i - 2] and cr1[j, i + 2]
            assert s[j - 1:j + 2, i - 1:i + 2].max() < sigclip - 1
    region = cover[P.CHAIN_ROWS.start:P.CHAIN_ROWS.stop, P.CHAIN_COLS.start:P.CHAIN_COLS.stop]
    assert (region == 1).all() and cover.sum() == region.size
    # the region holds the left end of the bar of `bars`, where its later iterations queue their candidates
    cr = P.oracle('bars', sigclip, sigfrac, 6)[0]
    assert cr[P.CHAIN_ROWS.start:P.CHAIN_ROWS.stop, P.CHAIN_COLS.start:P.CHAIN_COLS.stop].sum() >= 20
    assert not cr[:, :P.CHAIN_COLS.start].any()
