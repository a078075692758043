"""CPU: the scenes of tests/sattrail_paths.py are on the paths they are meant for.  The oracle's `info` says how far
a frame gets (votes, refinement, support, segment, make_mask's windows); what it does not record -- the runs of the
winning cell's voters, the rotated frame -- is computed here the way the oracle computes it.  A recipe that drifts
off its path fails here, before anyone needs a GPU for tests/test_gpu_sattrail_paths.py.

The theta classes are those of S.THETA_DEG[k], the angle of the line's normal: a trail that runs along y has theta near
0 or 180.  `theta_le45` is the frame whose k is 6 (5 deg), `theta_ge135` the one whose k is 346 (175 deg)."""
import numpy as np
import pytest

import sattrail as S
import sattrail_paths as P

# name -> (votes lo, votes hi, how far the oracle gets: 'votes' | 'support' | 'mask')
EXPECT = {
    'votes_low': (150, S.MIN_VOTES - 1, 'votes'),
    'votes_just': (S.MIN_VOTES, 230, 'mask'),
    'support_in': (S.MIN_VOTES + 20, 400, 'mask'),
    'support_out': (S.MIN_VOTES + 20, 400, 'support'),
    'gap_small': (400, 700, 'mask'),
    'gap_wide': (400, 700, 'mask'),
    'walk_stops': (400, 700, 'mask'),
    'theta_le45': (300, 450, 'mask'),
    'theta_ge135': (300, 450, 'mask'),
    'level': (300, 450, 'mask'),
    'diag': (450, 700, 'mask'),
    'anti_diag': (300, 700, 'mask'),
    'below_grid': (30, 150, 'votes'),
    'top_edge': (S.MIN_VOTES + 20, 450, 'mask'),
    'bottom_edge': (S.MIN_VOTES + 20, 450, 'mask'),
    'two_trails': (300, 450, 'mask'),
    'wide': (S.MIN_VOTES + 20, 450, 'mask'),
    'crowded': (S.MIN_VOTES + 20, 450, 'mask'),
    'no_edges': (0, 0, 'votes'),
    'neg_sky': (0, 0, 'votes'),
    'neg_pixel': (S.MIN_VOTES + 20, 450, 'mask'),
    'tail_minmax': (S.MIN_VOTES + 20, 450, 'mask'),
}


def test_every_scene_has_its_expectation():
    assert sorted(EXPECT) == sorted(P.NAMES)
    assert sorted(n for n in P.SCENES if EXPECT[n][2] == 'mask') == sorted(P.ACCEPTED)
    assert P.SAT_BANDH == P.device_constants()['SAT_BANDH'] == 96
    assert P.device_constants()['SAT_SUBLEN'] == 5 and P.device_constants()['SAT_SUBW'] == 200
    for name in P.SCENES:
        img = P.make_scene(name)
        assert img.dtype == np.float32 and img.size <= 600 * 1400 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0


def gaps(info):
    tmin, tmax, span = info['support']
    return tmin - span[0], span[1] - tmax


def trail_distance(name, which):
    """distance [full-resolution px] of every pixel from the whole line of trail [which]"""
    spec = P.SCENES[P.resolve(name)]
    (xa, ya, xb, yb, _, width, _) = spec['trails'][which]
    ny, nx = spec.get('shape', (600, 900))
    yy, xx = np.mgrid[0:ny, 0:nx]
    return np.abs(((xx - xa) * (yb - ya) - (yy - ya) * (xb - xa)) / np.hypot(xb - xa, yb - ya)), width


@pytest.mark.parametrize('name', P.NAMES)
def test_scene_gets_as_far_as_meant(name):
    lo, hi, stage = EXPECT[name]
    rec = P.oracle(name)
    info = rec.info
    print('%s: votes %d, k %d (%.1f deg), rho %g, bmin %g, bmax %g, %s' % (
        name, info['votes'], info['k'], S.THETA_DEG[info['k']], info['rho'], info['bmin'], info['bmax'],
        ', '.join(k for k in ('refine', 'support', 'segment', 'windows', 'make_mask_error') if k in info)))
    assert lo <= info['votes'] <= hi
    assert 'make_mask_error' not in info
    if stage == 'votes':
        assert not any(k in info for k in ('refine', 'support', 'segment', 'windows'))
    elif stage == 'support':
        assert 'refine' in info and 'support' in info and 'segment' not in info and 'windows' not in info
    else:
        assert all(k in info for k in ('refine', 'support', 'segment', 'windows'))
        assert max(gaps(info)) <= S.BUF
    if stage != 'mask':
        assert rec.nsats == 0 and not rec.mask.any() and not rec.accept and not rec.seg_ok and not rec.found
        return
    # the trail is masked, and nothing else: the strip of a window lies within the window's 10 binned rows = 20 px, un-binning
    # and the bilinear rotation back add 2 px each; a trail wider than that (`wide`: FWHM 20 px) up to 1.5 FWHM
    assert rec.nsats == 1 and rec.accept and rec.seg_ok and rec.found
    which = 1 if name == 'two_trails' else 0
    dist, width = trail_distance(name, which)
    got = rec.mask != 0
    assert set(np.unique(rec.mask)) == {0, 1}
    assert dist[got].max() <= max(24.0, 1.5 * width)
    centre = (dist <= 1) & P.truth(name, which)
    cover = (got & centre).sum() / centre.sum()
    print('  centre line covered %.3f, masked fraction %.4f, furthest masked pixel %.1f px' % (cover, got.mean(), dist[got].max()))
    # `wide`: the window is no higher than the trail's FWHM in binned rows, the rows above the window's mean are its brighter part
    assert cover >= (0.5 if name == 'wide' else 0.95)
    assert len(rec.painted) >= 5 and len(rec.painted) == sum(1 for w in rec.windows if w['z'])


def test_vote_threshold_pair():
    lo, just = P.oracle('votes_low').info, P.oracle('votes_just').info
    assert lo['votes'] < S.MIN_VOTES <= just['votes'] <= S.MIN_VOTES + 20
    assert lo['k'] == just['k']                                         # the same line, a shorter piece of it


def test_support_pair_straddles_buf():
    """both members get to the support test with the same line; the gap at the far end is either side of BUF"""
    a, b = P.oracle('support_in').info, P.oracle('support_out').info
    assert (a['k'], a['rho']) == (b['k'], b['rho'])
    ga, gb = gaps(a), gaps(b)
    print('support gaps: in %r, out %r' % (ga, gb))
    assert min(a['votes'], b['votes']) >= S.MIN_VOTES + 20              # it is not the vote count that decides
    assert S.BUF - 15 < max(ga) <= S.BUF < max(gb) < S.BUF + 15
    assert min(ga) < 5 and min(gb) < 5                                  # the other end reaches the border
    assert 'segment' in a and 'segment' not in b


def test_gap_pair_straddles_line_gap():
    """the voters of the winning cell, ordered along the line as S.trail_segment orders them: one run, or two"""
    ts, runs_s, ks = P.voters(P.make_scene('gap_small'))
    tw, runs_w, kw = P.voters(P.make_scene('gap_wide'))
    a, b = P.oracle('gap_small').info, P.oracle('gap_wide').info
    assert ks == a['k'] == kw == b['k'] and ts.size == a['votes'] and tw.size == b['votes']
    print('largest gaps between voters: %r, %r' % (np.sort(np.diff(ts))[-2:], np.sort(np.diff(tw))[-2:]))
    assert runs_s == 1 and S.LINE_GAP - 25 < np.diff(ts).max() <= S.LINE_GAP
    assert runs_w == 2 and S.LINE_GAP < np.diff(tw).max() < S.LINE_GAP + 40
    # one run: the segment spans the frame; two: it is the longer, second one
    (x0, y0), (x1, y1) = a['segment']
    assert x0 < 10 and x1 > 690
    (x0, y0), (x1, y1) = b['segment']
    assert 380 < x0 < 400 and x1 > 690
    # every other accepted scene but `votes_just` (whose trail ends in mid-frame) is one run
    for name in P.ACCEPTED:
        if name not in ('gap_wide', 'votes_just'):
            assert P.voters(P.make_scene(name))[1] == 1, name


THETA_CLASS = {'theta_le45': 'le45', 'anti_diag': 'le45', 'theta_ge135': 'ge135', 'diag': 'ge135', 'level': 'mid', 'two_trails': 'mid',
               'support_in': 'mid'}


@pytest.mark.parametrize('name', sorted(THETA_CLASS))
def test_orientation_branch(name):
    info = P.oracle(name).info
    theta = S.THETA_DEG[info['k']]
    (x0, y0), (x1, y1) = info['segment']
    cls = 'mid' if 45.0 < theta < 135.0 else ('le45' if theta <= 45.0 else 'ge135')
    print('%s: theta %.1f, segment %r' % (name, theta, info['segment']))
    assert cls == THETA_CLASS[name]
    if cls == 'mid':
        assert x0 < x1
    elif cls == 'le45':
        assert y0 > y1
    else:
        assert y0 < y1
    # the scenes' own places in their class: near the ends of the grid, on the class borders, along x
    want = {'theta_le45': (2.0, 8.0), 'theta_ge135': (172.0, 177.5), 'diag': (135.0, 135.0), 'anti_diag': (45.0, 45.0), 'level': (89.5, 90.5),
            'two_trails': (60.0, 70.0), 'support_in': (108.0, 114.0)}[name]
    assert want[0] <= theta <= want[1]
    if name in ('theta_le45', 'theta_ge135'):
        # both run from the smaller x to the larger x, as the rule of the middle class would have it (along a line of theta < 90
        # x falls as y grows, along one of theta > 90 it grows): the rules of the two outer classes exchanged would turn
        # both segments round, and with them the start of the walk
        assert x0 < x1 and abs(y1 - y0) > 400


def test_below_grid_is_the_first_angle():
    info = P.oracle('below_grid').info
    assert info['k'] == 0 and info['votes'] < S.MIN_VOTES


@pytest.mark.parametrize('name', ['top_edge', 'bottom_edge'])
def test_band_is_cut_by_the_rotated_frame(name):
    """the band of rows that k_sat_rotband interpolates, (int)sy -+ SAT_BANDH, is cut by the first / last row of the rotated
    frame, and the windows lie within a window's height of that row"""
    rec = P.oracle(name)
    sy, rows = rec.start[1], rec.rot_shape[0]
    first = rec.windows[0]['box']
    print('%s: start row %.2f of %d, first window rows %d..%d' % (name, sy, rows, first[2], first[3]))
    if name == 'top_edge':
        assert int(sy) - P.SAT_BANDH < 0 and int(sy) + P.SAT_BANDH < rows
        assert 0 <= first[2] < 2 * S_SUBLEN and min(w['box'][2] for w in rec.windows) < 2 * S_SUBLEN
    else:
        assert int(sy) + P.SAT_BANDH > rows and int(sy) - P.SAT_BANDH > 0
        assert rows - 2 * S_SUBLEN < first[3] <= rows and max(w['box'][3] for w in rec.windows) > rows - 2 * S_SUBLEN
    # every other accepted scene has the whole band inside
    for other in P.ACCEPTED:
        if other not in ('top_edge', 'bottom_edge'):
            r = P.oracle(other)
            assert int(r.start[1]) - P.SAT_BANDH >= 0 and int(r.start[1]) + P.SAT_BANDH <= r.rot_shape[0], other


S_SUBLEN = 5


def test_two_trails_the_stronger_wins():
    rec = P.oracle('two_trails')
    one = P.oracle('support_in').info                                   # (the first trail alone is the line of k = 218)
    assert rec.info['k'] != one['k'] and rec.info['votes'] > one['votes']
    d0, _ = trail_distance('two_trails', 0)
    d1, _ = trail_distance('two_trails', 1)
    got = rec.mask != 0
    assert (got & (d1 <= 1)).sum() >= 0.95 * (d1 <= 1).sum()
    # of the first trail only the crossing is masked
    assert (got & (d0 <= 1)).sum() <= 0.1 * (d0 <= 1).sum()


@pytest.mark.parametrize('name', ['no_edges', 'neg_sky'])
def test_empty_edge_list(name):
    b = S.bin2(P.make_scene(name))
    assert not S.edges(b).any() and P.oracle(name).info['nedge'] == 0
    if name == 'neg_sky':
        assert b.max() < 0                                              # no positive pixel at all
    else:
        assert b.min() == b.max() == 1000.0


def test_negative_binned_pixel():
    """bmin < 0 makes the clip range of the rotation [0, 1]: the `lo <= 0 <= hi` branch; every other accepted scene but
    `tail_minmax` has bmin > 0 and takes the other one"""
    for name in P.ACCEPTED:
        bmin = P.oracle(name).info['bmin']
        assert (bmin < 0) == (name in ('neg_pixel', 'tail_minmax')), name
    b = S.bin2(P.make_scene('neg_pixel'))
    assert b.min() == -1600.0 and (b < 0).sum() == 1
    # the planted block is far from the trail
    assert trail_distance('neg_pixel', 0)[0][40:42, 700:702].min() > 100


def test_tail_of_the_minmax_kernel():
    """k_bin_minmax reads float4s and leaves count % 4 pixels to a scalar tail: the extremes are there and nowhere else"""
    b = S.bin2(P.make_scene('tail_minmax'))
    n = b.size
    assert b.shape == (301, 451) and n % 4 == 3
    flat = b.reshape(-1)
    assert int(np.argmax(flat)) == n - 1 and int(np.argmin(flat)) == n - 2
    assert flat[n - 1] == 1.2e6 and flat[n - 2] == -1600.0
    body = flat[:n - 3]
    assert body.max() < 1e5 and body.min() > 0                          # without the tail: another maximum, a positive minimum
    info = P.oracle('tail_minmax').info
    assert info['bmax'] == 1.2e6 and info['bmin'] == -1600.0


def phase_of(rec, i):
    """which part of the walk looked at window i: 0 the first look, 1 to the right, 2 to the left of the start"""
    if i == 0:
        return 0
    return 1 if rec.windows[i]['box'][0] >= int(rec.start[0]) else 2


def test_walk_stops_at_an_empty_window():
    """`walk_stops` (the frame of `gap_wide`): to the right the walk ends where the frame ends, every window with a trail;
    to the left it goes on for several windows and ends at the one window without a row above the threshold.
    `votes_just`: the walk to the right ends at an empty window, and the walk to the left is still made."""
    rec = P.oracle('walk_stops')
    empty = [i for i, w in enumerate(rec.windows) if not w['z']]
    phases = [phase_of(rec, i) for i in range(len(rec.windows))]
    print('walk_stops: phases %r, empty %r' % (phases, empty))
    assert empty == [len(rec.windows) - 1] and phases[-1] == 2
    assert phases.count(1) >= 3 and phases.count(2) >= 4 and phases == sorted(phases)
    assert len(rec.painted) == len(rec.windows) - 1
    rec = P.oracle('votes_just')
    empty = [i for i, w in enumerate(rec.windows) if not w['z']]
    phases = [phase_of(rec, i) for i in range(len(rec.windows))]
    print('votes_just: phases %r, empty %r' % (phases, empty))
    assert len(empty) == 2 and phases[empty[0]] == 1 and phases[empty[1]] == 2 and empty[1] == empty[0] + 1
    assert len(rec.painted) == len(rec.windows) - 2


def test_no_scene_leaves_the_band():
    """the largest distance of a window from the start row, over all scenes: far inside SAT_BANDH (see
    sattrail_paths.BAND_EXIT_SEARCH for the search beyond these scenes)"""
    drift = {name: P.max_drift(P.oracle(name)) for name in P.ACCEPTED}
    print(drift)
    assert max(drift.values()) < 20 < P.SAT_BANDH
