"""TEST SCAFFOLDING -- small scenes that drive every decision, segment and walk branch of bbx_sat_trails
(blackbox_amd/csrc/bbx_sat.hip), and the oracle's record of each.  Shared by tests/test_sattrail_paths_host.py
(CPU: each scene is on its path, by the `info` of oracle/sattrail.py detect) and tests/test_gpu_sattrail_paths.py
(GPU: the library equals the oracle on them, decision by decision).  No device code depends on anything here.

The recipe is synth.sat_full_scene's (sky + noise 18, Gaussian stars, a Gaussian-profile trail), drawn in the same
order from the same generator, and extended here -- not there: the golden fixtures hash that function's output --
by several trails, trails present on stretches of their length only, a sky level and planted pixels.

The band exit of k_sat_walk (a window more than SAT_BANDH = 96 rows from the start row): see BAND_EXIT_SEARCH.
"""
import functools
import os
import re

import numpy as np

import sattrail as S                                    # oracle/sattrail.py (tests/conftest.py puts oracle/ on the path)

F = np.float32
SEED = 7
NOISE = 18.0
BASE = (0, 120, 900, 470, 120.0, 6.0)                   # the trail of most scenes: corner to corner of a 600 x 900 frame, 21 deg
LONG = (0, 120, 1400, 470, 120.0, 6.0)                  # the same across a 600 x 1400 frame
SAT_BANDH = 96                                          # bbx_sat.hip (test_sattrail_paths_host.py holds it against the source)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'blackbox_amd', 'csrc', 'bbx_sat.hip')


def device_constants():
    """SAT_BANDH, SAT_MAXWIN, SAT_SEG_CAP, SAT_SUBLEN, SAT_SUBW as bbx_sat.hip defines them"""
    text = open(SRC).read()
    out = {}
    for name in ('SAT_BANDH', 'SAT_MAXWIN', 'SAT_SEG_CAP', 'SAT_SUBLEN', 'SAT_SUBW'):
        vals = re.findall(r'^\s*#\s*define\s+%s\s+(\d+)\b' % name, text, flags=re.M)
        assert len(vals) == 1, '%s: expected one #define in bbx_sat.hip, found %r' % (name, vals)
        out[name] = int(vals[0])
    return out


def T(trail, *stretches):
    """a trail (xa, ya, xb, yb, amplitude, FWHM) kept on the stretches [(t_a, t_b), ...] of its length only
    (full-resolution pixels along the trail from (xa, ya)); none: the whole trail"""
    return tuple(trail) + (tuple(stretches) or None,)


# name -> dict(shape=(ny, nx), trails=[T(...)], nstars, sky, const, planted=[(y0, y1, x0, x1, value)])
SCENES = {
    # ---- k_trail_decide: the vote threshold
    'votes_low': dict(trails=[T(BASE, (0, 560))]),
    'votes_just': dict(trails=[T(BASE, (0, 700))]),
    # ---- k_trail_accept: support either side of BUF = 40 px from the border
    'support_in': dict(trails=[T(BASE, (60, 1000))]),
    'support_out': dict(trails=[T(BASE, (80, 1000))]),
    # ---- k_trail_segment: runs either side of LINE_GAP = 75; gap_wide also leaves the walk one empty window
    'gap_small': dict(shape=(600, 1400), trails=[T(LONG, (0, 600), (700, 1500))]),
    'gap_wide': dict(shape=(600, 1400), trails=[T(LONG, (0, 600), (800, 1500))]),
    # ---- k_trail_segment: the orientation of the segment's end points
    # (theta is the angle of the line's normal: 5 deg and 175 deg are trails 5 deg off the y axis; the diagonals are the class borders)
    'theta_le45': dict(shape=(900, 600), trails=[T((330, 0, 250, 900, 120.0, 6.0))]),
    'theta_ge135': dict(shape=(900, 600), trails=[T((250, 0, 330, 900, 120.0, 6.0))]),
    'level': dict(trails=[T((0, 300, 900, 300.5, 120.0, 6.0))]),
    'diag': dict(shape=(700, 700), trails=[T((0, 0, 700, 700, 120.0, 6.0))]),
    'anti_diag': dict(shape=(700, 700), trails=[T((0, 700, 700, 0, 120.0, 6.0))]),
    'below_grid': dict(shape=(900, 600), trails=[T((300, 0, 300.5, 900, 120.0, 6.0))]),
    # ---- k_sat_walk / k_sat_rotband: windows and band clamped by the rotated frame's first / last rows
    'top_edge': dict(trails=[T((0, 30, 900, 34, 150.0, 6.0))]),
    'bottom_edge': dict(trails=[T((0, 585, 900, 570, 150.0, 6.0))]),
    # ---- k_hough_lds: the stronger cell wins
    'two_trails': dict(trails=[T(BASE), T((0, 500, 900, 100, 200.0, 8.0))]),
    'wide': dict(trails=[T((0, 120, 900, 470, 120.0, 20.0))]),
    'crowded': dict(trails=[T((0, 120, 900, 470, 60.0, 4.0))], nstars=400),
    # ---- the empty edge list
    'no_edges': dict(const=250.0),
    'neg_sky': dict(trails=[], nstars=0, sky=-40.0),
    # ---- k_sat_rotband: a negative binned pixel makes clip_lo = 0 (lo <= 0 <= hi)
    'neg_pixel': dict(trails=[T(BASE)], planted=[(40, 42, 700, 702, -400.0)]),
    # ---- k_bin_minmax: 301 x 451 binned pixels, count % 4 == 3; the extremes sit in the last two
    'tail_minmax': dict(shape=(602, 902), trails=[T((0, 120, 902, 470, 120.0, 6.0))],
                        planted=[(600, 602, 900, 902, 3.0e5), (600, 602, 898, 900, -400.0)]),
}
# a path that another scene's frame is on as well
ALIASES = {'walk_stops': 'gap_wide'}
NAMES = list(SCENES) + list(ALIASES)

ACCEPTED = ['votes_just', 'support_in', 'gap_small', 'gap_wide', 'theta_le45', 'theta_ge135', 'level', 'diag', 'anti_diag', 'top_edge',
            'bottom_edge', 'two_trails', 'wide', 'crowded', 'neg_pixel', 'tail_minmax']
REJECTED = ['votes_low', 'support_out', 'below_grid', 'no_edges', 'neg_sky']
assert sorted(ACCEPTED + REJECTED) == sorted(SCENES)

BAND_EXIT_SEARCH = """The band exit of k_sat_walk (BBX_ERR_NOTCONV) needs a frame whose oracle windows move more than
SAT_BANDH = 96 rows from the start row.  No such scene of up to 400 x 4000 pixels was found; search_band_exit() below
is the search (minutes on the CPU, not run by the suite).  What it tried, and the largest distance of a window from
the start row that the oracle reached:
  two trails crossing at 1.5, 3, 6 and 12 deg (the stronger one wins the Hough cell)      8 .. 10 rows
  a trail that bends by 1 .. 6 deg in mid-frame; a parabolic trail, sagitta 40 .. 150 rows    rejected (support test)
  a level trail and a 5 .. 10 times brighter, 24 px wide one that leaves it at the start
  of the walk at 2.6 .. 2.9 deg, laid along the lowest row of the windows                     9 .. 12 rows
Why it is out of reach at this size: the next window's centre is iy0 + ceil(zmin + (zmax - zmin) / 2) against
iy0 + 5 now, so a step of 100 columns moves it by at most 4 rows up or 5 rows down, and only when nothing but the
outermost row of the window is above the threshold.  The rotated frame of a 400 x 4000 frame has at most 2010 columns:
21 steps.  96 rows would take 19 steps in a row at the full 5 rows, i.e. another, brighter feature than the winner of
the Hough cell, inclined by 2.9 deg to it, that starts on the winner at the frame's border and stays in the lowest
row of every window -- while the winner's own edge pixels, which that feature disturbs where the two are close, still
reach the border for the support test and are not split by a gap of more than 75 px.  The third family above is that
construction; the support test or the first windows end it.  The threshold itself is hardly ever missed by every row
(image / max makes the midvariance tiny: any row above the clipped mean counts), so the walk mostly keeps its row.
The exit stays unreached by any test."""


def resolve(name):
    return ALIASES.get(name, name)


@functools.lru_cache(maxsize=None)
def make_scene(name):
    """-> float32 frame (read-only)"""
    spec = SCENES[resolve(name)]
    ny, nx = spec.get('shape', (600, 900))
    assert ny * nx <= 600 * 1400
    if 'const' in spec:
        img = np.full((ny, nx), spec['const'], F)
    else:
        img = render(ny, nx, spec.get('trails', []), spec.get('nstars', 150), spec.get('sky', 250.0), SEED)
    for (y0, y1, x0, x1, v) in spec.get('planted', []):
        img[y0:y1, x0:x1] = v
    img.setflags(write=False)
    return img


def render(ny, nx, trails, nstars, sky, seed, bend=None):
    """synth.sat_full_scene's recipe with its extensions; bend: callable(t, d) -> d' for the band-exit search"""
    rs = np.random.RandomState(seed)
    img = sky + rs.normal(0, NOISE, (ny, nx))
    yy, xx = np.mgrid[0:ny, 0:nx]
    for _ in range(nstars):
        y0, x0, f = rs.uniform(0, ny), rs.uniform(0, nx), 10 ** rs.uniform(3, 5.5)
        r2 = (yy - y0) ** 2 + (xx - x0) ** 2
        sel = r2 < 15 ** 2
        img[sel] += (f / (2 * np.pi * 1.7 ** 2)) * np.exp(-r2[sel] / (2 * 1.7 ** 2))
    for (xa, ya, xb, yb, amp, width, stretches) in trails:
        norm = np.hypot(xb - xa, yb - ya)
        d = ((xx - xa) * (yb - ya) - (yy - ya) * (xb - xa)) / norm
        t = ((xx - xa) * (xb - xa) + (yy - ya) * (yb - ya)) / norm
        if bend is not None:
            d = bend(t, d)
        prof = amp * np.exp(-0.5 * (d / (width / 2.355)) ** 2)
        if stretches is not None:
            on = np.zeros((ny, nx), bool)
            for (ta, tb) in stretches:
                on |= (t >= ta) & (t <= tb)
            prof = np.where(on, prof, 0.0)
        img += prof
    return img.astype(F)


def truth(name, which=0, whole=False):
    """bool plane: the pixels within the FWHM of trail [which] of the scene, on its stretches (whole: all along it)"""
    spec = SCENES[resolve(name)]
    ny, nx = spec.get('shape', (600, 900))
    (xa, ya, xb, yb, amp, width, stretches) = spec['trails'][which]
    yy, xx = np.mgrid[0:ny, 0:nx]
    norm = np.hypot(xb - xa, yb - ya)
    d = ((xx - xa) * (yb - ya) - (yy - ya) * (xb - xa)) / norm
    t = ((xx - xa) * (xb - xa) + (yy - ya) * (yb - ya)) / norm
    on = np.ones((ny, nx), bool)
    if stretches is not None and not whole:
        on = np.zeros((ny, nx), bool)
        for (ta, tb) in stretches:
            on |= (t >= ta) & (t <= tb)
    return (np.abs(d) <= width / 2) & on


class Record:
    """what oracle/sattrail.py decides on a frame, in the terms of the device's sat_state"""

    def __init__(self, img):
        self.mask, self.nsats, self.info = S.detect(img)
        info = self.info
        self.accept = 'segment' in info
        self.seg_ok = 'windows' in info or 'make_mask_error' in info
        self.found = self.nsats > 0
        self.windows, self.rot_shape, self.start = [], None, None
        if self.accept:
            # the start point and the rotated shape are not in `info`: make_mask again on the oracle's segment
            try:
                m, dbg = S.make_mask(S.bin2(img), info['segment'], return_debug=True)
                self.windows, self.rot_shape, self.start = dbg['windows'], tuple(dbg['rot_shape']), tuple(dbg['start'])
                assert np.array_equal(np.kron(m.astype(np.uint8), np.ones((2, 2), np.uint8)), self.mask)
            except ValueError:
                b = S.bin2(img)
                img64 = b / b.max()
                seg = info['segment']
                ddx, ddy = float(seg[1][0] - seg[0][0]), float(seg[1][1] - seg[0][1])
                m, osh = S.rotate_matrix(img64.shape, ddx, ddy)
                self.rot_shape, self.start = tuple(osh), tuple(S.to_output(m, float(seg[0][0]), float(seg[0][1])))
        self.painted = [w for w in self.windows if len(w['z'])] if self.found else []

    def rects(self):
        """the strips as make_mask's paint() turns windows into rows: (r0, r1, c0, c1) in the rotated frame"""
        out = []
        for w in self.painted:
            ix0, ix1, iy0, iy1 = w['box']
            z = np.asarray(w['z'])
            out.append((max(iy0 + int(z.min()), 0), min(iy0 + int(z.max()) + 1, self.rot_shape[0]), ix0, ix1))
        return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> Record of the scene (computed once; leave it unchanged)"""
    return Record(make_scene(resolve(name)))


def voters(img):
    """the edge pixels that voted for the winning cell, ordered along the line as S.trail_segment orders them
    -> (t sorted, number of runs without a gap > S.LINE_GAP, k)"""
    b = S.bin2(img)
    edge = S.edges(b)
    ys, xs = np.nonzero(edge)
    acc, off = S.hough(edge)
    nrho = acc.shape[0]
    k, r = divmod(int(np.argmax(acc.T)), nrho)
    th = np.radians(S.THETA_DEG)
    ct, st = np.cos(th[k]), np.sin(th[k])
    rr = ct * xs + st * ys
    on = (np.where(rr > 0, rr + 0.5, rr - 0.5).astype(np.int64) + off) == r
    t = np.sort(ys[on] * ct - xs[on] * st, kind='stable')
    return t, 1 + int((np.diff(t) > S.LINE_GAP).sum()), k


def max_drift(rec):
    """rows between the start row and the furthest window the oracle looked at"""
    if not rec.windows:
        return 0.0
    sy = rec.start[1]
    return max(max(abs(w['box'][2] - sy), abs(w['box'][3] - sy)) for w in rec.windows)


def search_band_exit():
    """the search for a band-exit scene that BAND_EXIT_SEARCH reports -> [(what, furthest window from the start row)]"""
    out = []
    ny, nx = 400, 4000
    for deg in (1.5, 3.0, 6.0, 12.0):
        dy = np.tan(np.radians(deg)) * nx / 2
        tr = [T((0, 200 - dy / 2, nx, 200 + dy / 2, 150.0, 6.0)), T((0, 200 + dy / 2, nx, 200 - dy / 2, 120.0, 6.0))]
        out.append(('cross %g deg' % deg, max_drift(Record(render(ny, nx, tr, 150, 250.0, SEED)))))
    for deg in (1.0, 2.0, 4.0, 6.0):
        k = np.tan(np.radians(deg))
        out.append(('bend %g deg' % deg, max_drift(Record(render(ny, nx, [T((0, 60, nx, 60, 150.0, 6.0))], 150, 250.0, SEED,
                                                                  bend=lambda t, d, k=k: d - k * np.maximum(t - nx / 2, 0))))))
    for sag in (40.0, 100.0, 150.0):
        out.append(('curve sagitta %g' % sag,
                    max_drift(Record(render(ny, nx, [T((0, 120, nx, 120, 150.0, 6.0))], 150, 250.0, SEED,
                                            bend=lambda t, d, sag=sag: d - sag * (1 - ((t - nx / 2) / (nx / 2)) ** 2))))))
    # a level trail at y = 372 (FWHM 12) and a brighter band of 24 px whose lower edge e0 - slope x leaves it at the border
    yy, xx = np.mgrid[0:ny, 0:nx]
    for (slope, e0, amp) in ((0.05, 369.0, 1500.0), (0.048, 369.0, 2000.0), (0.05, 368.0, 3000.0), (0.046, 369.5, 1500.0)):
        img = 250.0 + np.random.RandomState(SEED).normal(0, NOISE, (ny, nx))
        img += 300.0 * np.exp(-0.5 * ((yy - 372.0) / (12.0 / 2.355)) ** 2)
        e = e0 - slope * xx
        img += amp / (1 + np.exp(yy - e)) / (1 + np.exp(e - 24.0 - yy))
        out.append(('band slope %g from %g, %g e-' % (slope, e0, amp), max_drift(Record(img.astype(F)))))
    return out
