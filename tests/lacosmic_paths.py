"""TEST SCAFFOLDING -- small scenes that drive bbx_lacosmic's queue, spill and seam paths, and a host
model of where a raw candidate travels in the dense vector pass (k_lac_cand_v4).  Shared by
tests/test_lacosmic_paths_host.py (CPU: the scenes are on their paths) and
tests/test_gpu_lacosmic_paths.py (GPU: the library equals the oracle on them).  No device code depends
on anything here.
"""
import os
import re

import numpy as np
from scipy import ndimage

import lacosmic as L                                    # oracle/lacosmic.py (tests/conftest.py puts oracle/ on the path)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'blackbox_amd', 'csrc', 'bbx_lacosmic.hip')


def device_constants():
    """CAND_SPAN, CAND_ROWS, CAND_TILECAP, CAND_WQ as bbx_lacosmic.hip defines them"""
    text = open(SRC).read()
    out = {}
    for name in ('CAND_SPAN', 'CAND_ROWS', 'CAND_TILECAP', 'CAND_WQ'):
        vals = re.findall(r'^\s*#\s*define\s+%s\s+(\d+)\b' % name, text, flags=re.M)
        assert len(vals) == 1, '%s: expected one #define in bbx_lacosmic.hip, found %r' % (name, vals)
        out[name] = int(vals[0])
    return out


_C = device_constants()
CAND_SPAN, CAND_ROWS, CAND_TILECAP, CAND_WQ = _C['CAND_SPAN'], _C['CAND_ROWS'], _C['CAND_TILECAP'], _C['CAND_WQ']
# the scenes below are laid out for exactly this tiling: a retune has to move them with it
assert (CAND_SPAN, CAND_ROWS, CAND_TILECAP, CAND_WQ) == (248, 16, 64, 512), _C
CAND_ROWMAX = 256                                       # the kernel spills when another row of 64 x 4 pixels may not fit

RN, OBJLIM = 8.2, 3.0
PARAMS = ((15.0, 0.01), (4.5, 0.3))                     # (sigclip, sigfrac)
SKY, NOISE, HIT = 100.0, 8.0, 3000.0

NOT_CAND, SPILLED, SEGMENT, OVERFLOW = 0, 1, 2, 3
PATH_NAMES = {SPILLED: 'spilled', SEGMENT: 'segment', OVERFLOW: 'overflow'}


# ---- host model ------------------------------------------------------------------------------------
def prune_threshold(sigclip, rn=RN):
    """T of k_lac_begin, float32 step by step"""
    rn = F(rn)
    return F(F(F(F(2) * F(sigclip)) * np.sqrt(F(rn * rn))) * F(F(1) - F(1e-5)))


def raw_candidates(img, sigclip, rn=RN):
    """bool plane: L+ > T inside the 2-pixel frame (what the dense pass of iteration 1 queues)"""
    c = L.lplus(np.asarray(img, F)) > prune_threshold(sigclip, rn)
    c[:2] = False; c[-2:] = False; c[:, :2] = False; c[:, -2:] = False
    return c


def tile_of(j, i):
    """(tile row, wave along x) of pixel (j, i) in k_lac_cand_v4"""
    return j // CAND_ROWS, i // CAND_SPAN


def travel(img, sigclip, rn=RN):
    """Replay of k_lac_cand_v4's queue discipline -> int8 plane: NOT_CAND, or where the raw candidate
    goes: SPILLED (the wave's LDS queue was written out to the overflow list in mid-tile), SEGMENT (one of
    the first CAND_TILECAP entries left at the end of the tile) or OVERFLOW (the rest at the end of the
    tile).  Queue order within a row: column-in-lane q = 0..3 outermost, then lane."""
    cand = raw_candidates(img, sigclip, rn)
    ny, nx = cand.shape
    out = np.zeros(cand.shape, np.int8)
    for j0 in range(0, ny, CAND_ROWS):
        for x0 in range(0, nx, CAND_SPAN):
            queue = []
            for j in range(j0, min(j0 + CAND_ROWS, ny)):
                cols = x0 + np.nonzero(cand[j, x0:x0 + CAND_SPAN])[0]
                # lane l of the wave holds the columns x0 - 4 + 4l .. + 3: (q, lane) = ((i - x0) % 4, (i - x0) // 4 + 1)
                queue += [(j, i) for i in sorted(cols, key=lambda i: ((i - x0) % 4, (i - x0) // 4))]
                assert len(queue) <= CAND_WQ
                if len(queue) > CAND_ROWMAX:
                    for (jj, ii) in queue:
                        out[jj, ii] = SPILLED
                    queue = []
            for k, (jj, ii) in enumerate(queue):
                out[jj, ii] = SEGMENT if k < CAND_TILECAP else OVERFLOW
    assert np.array_equal(out != NOT_CAND, cand)
    return out


def tile_counts(path, tj, ti, within=None):
    """{path name: number of pixels of tile (tj, ti) that travel it}, optionally only pixels of [within]"""
    sl = (slice(tj * CAND_ROWS, (tj + 1) * CAND_ROWS), slice(ti * CAND_SPAN, (ti + 1) * CAND_SPAN))
    p = path[sl]
    if within is not None:
        p = np.where(within[sl], p, NOT_CAND)
    return {name: int((p == code).sum()) for code, name in PATH_NAMES.items()}


# ---- scenes ------------------------------------------------------------------------------------------
SEEDS = {'tiny': 101, 'one_tile': 102, 'sliver': 103, 'seams': 104, 'dense': 105, 'bars': 106, 'streaks': 107}
SHAPES = {'tiny': (8, 8), 'one_tile': (16, 248), 'sliver': (17, 252), 'seams': (48, 744), 'dense': (40, 504),
          'bars': (72, 260), 'streaks': (40, 504)}
PLANTED = {
    'tiny': [(2, 2), (5, 5), (3, 4)],
    'one_tile': [(2, 2), (13, 245), (8, 124)],
    'sliver': [(2, 2), (14, 248), (14, 249), (8, 247), (2, 249), (13, 100)],
    'seams': [(15, 247), (16, 248), (31, 495), (32, 496), (24, 246), (24, 249), (20, 494), (20, 497), (2, 2), (45, 741)],
    # seam and corner hits around the lattice of `dense`
    'dense': [(15, 247), (16, 248), (31, 247), (32, 248), (24, 246), (24, 249), (2, 2), (37, 501)],
    'bars': [],
    'streaks': [],
}
DENSE_ROWS, DENSE_COLS = range(17, 30, 2), range(3, 246, 3)
DENSE_TILE = (1, 0)                                     # rows 16..31, columns 0..247
BAR_PROFILE = (1500.0, 5000.0, 20000.0, 5000.0, 1500.0)
# `streaks`: the shape of `dense`, bars-style streaks instead of the lattice -- two inside the lattice's tile,
# one across the wave seam at column 248 and the tile seam at row 32
STREAKS = [(18, 10, 120), (25, 130, 240), (29, 200, 300)]   # (first row, first column, end column)

# `chain0` .. `chain17`: the shape of `bars`; five pixels A C B C A along a row (bright, moderate, faint,
# moderate, bright).  L+ of B is suppressed while the C pixels stand (2 b - c < T) and ~2 b once they are
# cleaned, so B is no candidate of the dense pass and only k_lac_cand_sparse can queue it, in iteration 2.
# C is flagged in iteration 1 by the second growth alone (s(C) < sigclip 15: never a stage-2 pixel), so B is
# two pixels from the nearest stage-2 pixel A: nothing of iteration 1 writes or clears B's byte of the flag
# plane.  Over the eighteen phases every pixel of rows 29..34 x columns 18..29 -- the left end of the bar of
# `bars`, where its later iterations queue their candidates -- is a B exactly once.  For sigclip 15 only.
CHAIN_ROWS, CHAIN_COLS = range(29, 35), range(18, 30)
CHAIN_A, CHAIN_C, CHAIN_B = 20000.0, 450.0, 300.0
NCHAIN = 18


def chain_pixels(phase):
    """B pixels of `chain<phase>`"""
    pr, pc = phase // 6, phase % 6
    return [(j, i) for j in CHAIN_ROWS if j % 3 == pr for i in CHAIN_COLS if i % 6 == pc]


for _k in range(NCHAIN):
    SEEDS['chain%d' % _k] = 200 + _k
    SHAPES['chain%d' % _k] = SHAPES['bars']
    PLANTED['chain%d' % _k] = []


def first_iteration_s(name, rn=RN):
    """s = L+ / (2 noise) of the scene as the first iteration sees it (sp <= s everywhere)"""
    img = make_scene(name)
    rn = F(rn)
    m5 = np.maximum(L.medfilt(img, 5), F(0.00001))
    return L.lplus(img) / (F(2.0) * np.sqrt(m5 + F(rn * rn)).astype(F))


SCENES = ('tiny', 'one_tile', 'sliver', 'seams', 'dense', 'bars')


def sky(name):
    rs = np.random.RandomState(SEEDS[name])
    return (SKY + NOISE * rs.standard_normal(SHAPES[name])).astype(F), rs


def make_scene(name):
    """-> float32 image (a fresh array every call)"""
    img, rs = sky(name)
    if name == 'dense':
        amp = rs.uniform(1500.0, 6000.0, (len(DENSE_ROWS), len(DENSE_COLS))).astype(F)
        img[np.ix_(list(DENSE_ROWS), list(DENSE_COLS))] += amp
    if name == 'bars':
        img[30:35, 20:240] += np.array(BAR_PROFILE, F)[:, None]
    if name == 'streaks':
        for (r0, c0, c1) in STREAKS:
            img[r0:r0 + 5, c0:c1] += np.array(BAR_PROFILE, F)[:, None]
    if name.startswith('chain'):
        for (j, i) in chain_pixels(int(name[5:])):
            img[j, i - 2:i + 3] += np.array([CHAIN_A, CHAIN_C, CHAIN_B, CHAIN_C, CHAIN_A], F)
    for (j, i) in PLANTED[name]:
        img[j, i] += F(HIT)
    return img


def make_mask(name):
    """uint8 mask every frame carries: an edge column block and a few scattered bad pixels, none on a
    planted hit"""
    ny, nx = SHAPES[name]
    rs = np.random.RandomState(SEEDS[name] + 1000)
    mask = np.zeros((ny, nx), np.uint8)
    bad = rs.random_sample((ny, nx)) < 4e-3
    # frames this small could draw none: two fixed ones (inside the 2-pixel frame and outside it)
    bad[ny // 2, nx // 2] = True
    bad[0, nx - 1] = True
    for (j, i) in PLANTED[name]:
        bad[j, i] = False
    if name.startswith('chain'):
        for (j, i) in chain_pixels(int(name[5:])):
            bad[j - 2:j + 3, i - 4:i + 5] = False
    mask[bad] |= 1
    mask[:, :3] |= 32
    return mask


_ORACLE = {}


def oracle(name, sigclip, sigfrac, niter, rn=RN, masked=True):
    """L.detect_cosmics(..., return_iters=True) on the scene with its mask (or with none), computed once
    per key and never modified: (crmask, clean, iters, n objects)"""
    key = (name, float(sigclip), float(sigfrac), int(niter), float(F(rn)), bool(masked))
    if key not in _ORACLE:
        mask = make_mask(name) != 0 if masked else np.zeros(SHAPES[name], bool)
        cr, clean, iters = L.detect_cosmics(make_scene(name), mask, sigclip, sigfrac, OBJLIM, niter, F(rn), return_iters=True)
        nobj = ndimage.label(cr, structure=np.ones((3, 3), bool))[1]
        cr.setflags(write=False); clean.setflags(write=False)
        _ORACLE[key] = (cr, clean, list(iters), int(nobj))
    return _ORACLE[key]
