"""Scenes and path conditions for the mask tail (bbx_mask_finish in blackbox_amd/csrc/bbx_mask.hip): numpy only,
no GPU, no torch.

Three parts:

* frame(): a float32 raw frame with zero overscan strips whose data sections hold 1e6 / gain at the planted pixels,
  the way test_gpu_parity.test_fill_holes_shapes drives R.calibrate;
* decompose(): a restatement of the kernel's 64 x 64 tile decomposition.  It does NOT compute the expected mask (that
  is the oracle's job); it says which tiles the coarse stage must leave to the pixel flood, so that a test can assert
  that a scene takes the path it is meant to take;
* seeded scene builders that take the reduced-frame shape and return a boolean plane of saturated pixels, and
  compose(), which puts all of them on one frame without overlap.

The builders draw in a canonical orientation (short axis v, long axis u) and transpose at the end for frames that
are taller than wide, so the same structures exist for tile rows as for tile columns.  Geometry decides some details:

* a frame 192 to 208 px across its short axis cannot hold a circle of radius 100: rings are ellipses there, with the
  short semi-axis set by the frame and the long one 100 to 200 px;
* a ring crosses X = 4095|4096 only where 4096 is not within a ring's width of the frame end (geometry D); the wide
  frames B, E, F have a ring across 8192, the boundary between the second and third word of a free-tile bit row;
* the plane that is closed and filled is the saturated pixels plus their 3x3 ring: a planted 1-px wall is 3 px thick
  there and a gap of g planted pixels is g - 2 px wide.  A 3x3 closing seals a straight gap of up to 2 px and leaves
  one of 3 px, so the open pinhole has 5 planted pixels missing (3 px, the narrowest gap that survives) and its twin
  4 (2 px, the widest that is sealed).  For the same reason two planted pixels are joined when they are up to 5 px
  apart and stay apart at 6."""
import numpy as np
from scipy import ndimage

TILE = 64
CF_MAX = 256                    # k_coarse_cc up to CF_MAX x CF_MAX tiles, k_coarse_flood beyond
COARSE_MAX = 49152              # bbx_mask_finish refuses more tiles
OS_Y, OS_X = 20, 12
TEL = 'ML1'
# name -> (ysz, xsz); reduced frame 2 * ysz by 8 * xsz
GEOMS = {'A': (96, 516), 'B': (104, 2044), 'C': (4200, 24), 'D': (2072, 516), 'E': (96, 2056), 'F': (8224, 24)}
# name -> (W, TH): tile columns, tile rows
TILES = {'A': (65, 3), 'B': (256, 4), 'C': (3, 132), 'D': (65, 65), 'E': (257, 3), 'F': (3, 257)}
LANE = 130                      # serpentine: corridor width (px); > 127, so every lane holds whole tiles
NLANE = 9                       # 8 inner walls = 8 turns
PIN = 2 + 2 * TILE + 2          # pinhole box: wall and ring end at a tile seam, two whole tiles, wall and ring again
STRUCT8 = np.ones((3, 3), bool)
CROSS = ndimage.generate_binary_structure(2, 1)


def shape_of(name):
    ysz, xsz = GEOMS[name]
    return 2 * ysz, 8 * xsz


# ---- frame ------------------------------------------------------------------------------------------------------------
def _sections(raw_shape, ysz, xsz):
    """(data section in the raw frame, section in the reduced frame) of the 16 channels"""
    import bbx_oracle as O
    secs = O.define_sections(raw_shape, ysz, xsz)
    return list(zip(secs[1], secs[4]))


def frame(ysz, xsz, os_y, os_x, sat_pixels, bpm=None):
    """-> (raw float32 [2 (ysz + os_y), 8 (xsz + os_x)], planted bool [2 ysz, 8 xsz]).  Overscan strips zero, data
    sections 1e6 / gain[c] at the planted pixels and 0 elsewhere (far above every channel's saturation level once the
    gain is applied).  bpm, when given, is only checked for shape and type: bad pixels do not change the raw frame."""
    from blackbox_amd import settings
    if not (os_y > 10 and os_x > 6):
        raise ValueError('bbx_make_dims needs os_y > 10 and os_x > 6')
    planted = np.ascontiguousarray(sat_pixels, dtype=bool)
    if planted.shape != (2 * ysz, 8 * xsz):
        raise ValueError('sat_pixels: shape {} expected'.format((2 * ysz, 8 * xsz)))
    if bpm is not None and (bpm.shape != planted.shape or bpm.dtype != np.uint8):
        raise ValueError('bpm: uint8 of the reduced shape expected')
    gain = np.float32(settings.gain[TEL])
    raw = np.zeros((2 * (ysz + os_y), 8 * (xsz + os_x)), np.float32)
    for c, (dsec, rsec) in enumerate(_sections(raw.shape, ysz, xsz)):
        raw[dsec] = np.where(planted[rsec], np.float32(1e6) / gain[c], np.float32(0))
    return raw, planted


def reduced(raw, ysz, xsz):
    """what calibrate makes of frame()'s raw with a zero overscan solution: float32 raw * float32 gain, cropped"""
    from blackbox_amd import settings
    gain = np.float32(settings.gain[TEL])
    data = np.zeros((2 * ysz, 8 * xsz), np.float32)
    for c, (dsec, rsec) in enumerate(_sections(raw.shape, ysz, xsz)):
        data[rsec] = raw[dsec] * gain[c]
    return data


def oracle_mask(planted, bpm, ysz, xsz):
    """O.mask_init on the reduced data of frame(): (mask, NOBJ-SAT)"""
    import bbx_oracle as O
    from blackbox_amd import settings
    raw, _ = frame(ysz, xsz, OS_Y, OS_X, planted, bpm)
    header = {'BIASM%d' % (c + 1): 0.0 for c in range(16)}
    mask, hm = O.mask_init(reduced(raw, ysz, xsz), header, bpm, settings.gain[TEL], settings.satlevel[TEL], ysz, xsz)
    return mask, int(hm['NOBJ-SAT'])


def prefill_mask(planted, bpm=None):
    """the mask before fill_sat_holes made directly from the planted plane: saturated = 4, its 3x3 ring = 8 (no
    crosstalk flags)"""
    mask = np.zeros(planted.shape, np.uint8) if bpm is None else bpm.copy()
    mask[planted] |= 4
    mask[ndimage.binary_dilation(planted, structure=STRUCT8) & ~planted] |= 8
    return mask


# ---- the tile decomposition, restated -----------------------------------------------------------------------------
def _tiles_any(plane):
    ny, nx = plane.shape
    th, w = -(-ny // TILE), -(-nx // TILE)
    pad = np.zeros((th * TILE, w * TILE), bool)
    pad[:ny, :nx] = plane
    return pad.reshape(th, TILE, w, TILE).any(axis=(1, 3))


class Decomposition:
    """[mask]: the oracle's final mask.  The plane before the fill, M = (mask & 4) | (mask & 8), is the saturated
    pixels and their 3x3 ring, i.e. the dilation of (mask & 4): the fill only adds 8s, the ring is where mask_init put
    the others.  From it: the closed plane, the tile occupancy at 64 x 64, the empty tiles 4-connected to the frame
    border through empty tiles (resolved wholesale by the coarse stage; every other tile is left to the pixel flood)."""

    def __init__(self, mask, bpm=None):
        self.shape = mask.shape
        self.M = ndimage.binary_dilation((mask & 4) != 0, structure=STRUCT8)
        self.closed = ndimage.binary_closing(self.M, structure=STRUCT8)
        self.holes = ndimage.binary_fill_holes(self.closed, structure=STRUCT8) & ~self.closed
        self.occ = _tiles_any(self.closed)
        self.TH, self.W = self.occ.shape
        lab, _ = ndimage.label(~self.occ, structure=CROSS)
        edge = np.zeros(self.occ.shape, bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        self.outside = np.isin(lab, np.unique(lab[edge & ~self.occ])) & ~self.occ
        self.added = self.closed & ~self.M
        self.bad_holes = self.holes & (bpm == 1) if bpm is not None else np.zeros(mask.shape, bool)

    def stats(self, box=None):
        """box = (y0, y1, x0, x1) restricts the pixel counts to a structure, and the tile counts and the free-tile
        span to the tiles that lie wholly inside it"""
        y0, y1, x0, x1 = box if box is not None else (0, self.shape[0], 0, self.shape[1])
        ty0, ty1, tx0, tx1 = -(-y0 // TILE), y1 // TILE, -(-x0 // TILE), x1 // TILE
        if box is None:
            ty0, ty1, tx0, tx1 = 0, self.TH, 0, self.W
        t = (slice(ty0, ty1), slice(tx0, tx1))
        span = 0
        if self.occ[t].size:
            sl, _ = ndimage.label(~self.occ[t], structure=CROSS)
            for s in ndimage.find_objects(sl):
                span = max(span, s[0].stop - s[0].start, s[1].stop - s[1].start)
        ys, xs = np.nonzero(self.added[y0:y1, x0:x1])
        return {'unresolved': int((~self.outside)[t].sum()),
                'unresolved_empty': int((~self.outside & ~self.occ)[t].sum()),
                'added_x_seam': int(np.isin((xs + x0) % TILE, (0, TILE - 1)).sum()),
                'added_y_seam': int(np.isin((ys + y0) % TILE, (0, TILE - 1)).sum()),
                'holes': int(self.holes[y0:y1, x0:x1].sum()),
                'free_span': int(span),
                'bad_in_hole': int(self.bad_holes[y0:y1, x0:x1].sum())}


# ---- canonical canvas and layout -----------------------------------------------------------------------------------
def _canon(shape):
    ny, nx = shape
    tall = ny >= 2 * nx
    return (nx, ny, True) if tall else (ny, nx, False)


def _marks(n):
    """coordinates along an axis of n px next to which seam pairs go: the first word / tile boundary, 4096 (the
    boundary between two words of a free-tile bit row), the start of a partial last word / tile row, the end"""
    m = {TILE}
    if n >= 4096 + 32:
        m.add(4096)
    if n % TILE:
        m.add(n - n % TILE)
    return sorted(m) + [n]


def layout(shape):
    """regions (v0, v1, u0, u1) in canonical coordinates for every structure of the combined frame.  Items are laid
    out along the long axis with equal spacing, so that a long frame has holes in every third of it (tile rows of all
    three waves of the run-id scan at geometry C); thin frames (short axis < 600 px) keep the columns next to the
    long-axis seam marks free for the seam pairs."""
    S, L, tall = _canon(shape)
    thin = S < 600
    vm = 8
    lay = {'thin': thin, 'S': S, 'L': L, 'tall': tall}
    serp = NLANE * (LANE + 1) + 1
    seams_w = 104 * (len(_marks(S)) - 1) + 50 + 6          # the end's patch is the narrow one
    if thin:
        full = (vm, S - vm)
        items = [('seams', seams_w, full, None), ('pin_u_open', PIN, full, 62), ('pin_u_shut', PIN, full, 62),
                 ('pin_v_open', PIN, (62, S - vm), None), ('pin_v_shut', PIN, (62, S - vm), None),
                 ('serp_open', serp, full, None), ('serp_shut', serp, full, None), ('sparse', 80, full, None),
                 ('borders', 82, (0, S), None), ('ring_nested', 2 * 160 + 1, full, None)]
    else:
        items = [('seams', seams_w, (0, S), None), ('pin_u_open', PIN, (200, 420), 62), ('pin_u_shut', PIN, (200, 420), 62),
                 ('pin_v_open', PIN, (254, 254 + PIN), None), ('pin_v_shut', PIN, (254, 254 + PIN), None),
                 ('serp_open', 6 * TILE + LANE, (vm, vm + serp), None), ('serp_shut', 6 * TILE + LANE, (vm, vm + serp), None),
                 ('sparse', 300, (200, 500), None), ('borders', 82, (0, S), None),
                 ('ring_nested', 2 * 190 + 1, (1600, 1600 + 2 * 190 + 1), None)]
    # thin frames: the columns next to the long-axis seam marks are the seam pairs'
    zones = [(m - 14, m + 16) for m in _marks(L) if m != L] if thin else []
    # a ring at the frame end (crosses the last word / tile row boundary where the seam columns leave room) ...
    if thin:
        end = min([L - 40] + [z[0] - 4 for z in zones if z[0] > L - 200])
        lay['ring_edge'] = (vm, S - vm, end - 2 * 100, end + 1)
        zones.append((lay['ring_edge'][2] - 8, L))
    else:
        end = L - 12
        lay['ring_edge'] = (2300, 2300 + 2 * 150 + 1, end - 2 * 150, end + 1)
    # ... and one across u = 8192 where the frame is long enough
    if L >= 8800:
        lay['ring_word'] = (vm, S - vm, 8192 - 150, 8192 + 151) if thin else (2300, 2601, 8192 - 150, 8192 + 151)
        zones.append((8192 - 158, 8192 + 159))
    u_start = 84 if thin else 40                              # thin: past the left-border ring and the seam columns of u = 64
    limit = lay['ring_edge'][2] - 8 if thin else L - 8
    # the widest equal spacing (at most 1200 px) with which everything fits: a structure that has to step over seam
    # columns or wait for its alignment uses up room
    for gap in range(1200, 5, -1):
        u = u_start
        for name, width, (v0, v1), align in items:
            u += gap
            moved = True
            while moved:
                moved = False
                if align is not None:
                    u += (align - u) % TILE
                for z0, z1 in zones:
                    if u < z1 and u + width > z0:
                        u = z1
                        moved = True
            lay[name] = (v0, v1, u, u + width)
            u += width
        if u <= limit:
            break
    else:
        raise ValueError('layout: the structures do not fit')
    return lay


class _Canvas:
    def __init__(self, shape):
        self.shape = tuple(shape)
        self.lay = layout(shape)
        self.S, self.L, self.tall = self.lay['S'], self.lay['L'], self.lay['tall']
        self.p = np.zeros((self.S, self.L), bool)

    def out(self):
        return np.ascontiguousarray(self.p.T) if self.tall else self.p

    def ring(self, cv, cu, rv, ru, t=3):
        """elliptical ring, t px thick, clipped by the frame"""
        v0, v1 = max(0, cv - rv - 1), min(self.S, cv + rv + 2)
        u0, u1 = max(0, cu - ru - 1), min(self.L, cu + ru + 2)
        vv, uu = np.ogrid[v0:v1, u0:u1]
        outer = ((vv - cv) / float(rv)) ** 2 + ((uu - cu) / float(ru)) ** 2 <= 1.0
        inner = ((vv - cv) / float(rv - t)) ** 2 + ((uu - cu) / float(ru - t)) ** 2 <= 1.0
        self.p[v0:v1, u0:u1] |= outer & ~inner


def real_box(shape, region):
    """canonical region -> (y0, y1, x0, x1) of the frame"""
    v0, v1, u0, u1 = region
    return (u0, u1, v0, v1) if _canon(shape)[2] else (v0, v1, u0, u1)


# ---- scene builders --------------------------------------------------------------------------------------------------
def big_rings(shape, seed=0):
    """rings 3 px thick, outer radius 100 to 200 px (ellipses in thin frames), each with at least one empty tile
    strictly inside; a ring inside a ring with a blob at the centre"""
    c = _Canvas(shape)
    rs = np.random.RandomState(seed)
    lay = c.lay
    # ring inside a ring, blob at the centre of a tile so that it occupies one tile only
    v0, v1, u0, u1 = lay['ring_nested']
    cv, cu = (v0 + v1) // 2, (u0 + u1) // 2
    ro = (u1 - u0 - 1) // 2
    rv_o = min(ro, (v1 - v0 - 1) // 2)
    c.ring(cv, cu, rv_o, ro)
    c.ring(cv, cu, rv_o - 12 if lay['thin'] else ro - 45, ro - 45)
    bv, bu = (cv // TILE) * TILE + 32, (cu // TILE) * TILE + 32
    c.p[bv - 2:bv + 3, bu - 2:bu + 3] = True
    for name in ('ring_edge', 'ring_word'):
        if name in lay:
            v0, v1, u0, u1 = lay[name]
            ru = (u1 - u0 - 1) // 2
            rv = min(ru, (v1 - v0 - 1) // 2)
            shrink = int(rs.randint(0, 3))                   # the seed moves the inner edge only: the outer extent is the layout's
            c.ring((v0 + v1) // 2, (u0 + u1) // 2, rv - shrink, ru - shrink)
    return c.out()


def _serpentine(c, region, open_, stack_u):
    """NLANE lanes LANE px wide, stacked along u (stack_u) or v, separated by 1-px walls that leave a LANE px gap at
    alternating ends; outer walls all round; the mouth (open) is the whole end of the first lane"""
    v0, v1, u0, u1 = region
    p = c.p if stack_u else c.p.T                            # p[b, a]: a = stacking axis
    (b0, b1, a0) = (v0, v1, u0) if stack_u else (u0, u1, v0)
    a1 = a0 + NLANE * (LANE + 1)
    for i in range(NLANE + 1):
        a = a0 + i * (LANE + 1)
        if i in (0, NLANE):
            p[b0:b1, a] = True
        elif i % 2:
            p[b0:b1 - 1 - LANE, a] = True
        else:
            p[b0 + 1 + LANE:b1, a] = True
    p[b0, a0:a1 + 1] = True
    p[b1 - 1, a0:a1 + 1] = True
    if open_:
        p[b0, a0 + 1:a0 + LANE + 1] = False


def serpentine(shape, open=True, seed=0):
    c = _Canvas(shape)
    _serpentine(c, c.lay['serp_open' if open else 'serp_shut'], open, c.lay['thin'])
    return c.out()


def pinhole(shape, axis='x', gap=5, seed=0):
    """a closed box of 1-px walls round two whole empty tiles with one gap.  axis 'x': the gap is in a wall whose
    ring ends at X % 64 == 63 (seed even; the interior begins at X % 64 == 0, so the flood has to cross from bit 63
    of one word to bit 0 of the next) or begins at X % 64 == 0 (seed odd: the other direction); axis 'y': the same
    across a tile row seam.  gap = 5 planted pixels survives the closing (interior not a hole), gap = 4 is sealed by
    it (interior a hole)."""
    c = _Canvas(shape)
    along_u = (axis == 'x') != c.tall                        # the wall with the gap is perpendicular to u
    name = ('pin_u_' if along_u else 'pin_v_') + ('open' if gap >= 5 else 'shut')
    v0, v1, u0, u1 = c.lay[name]
    p = c.p
    p[v0, u0:u1] = True
    p[v1 - 1, u0:u1] = True
    p[v0:v1, u0] = True
    p[v0:v1, u1 - 1] = True
    rs = np.random.RandomState(seed)
    far = seed % 2 == 1
    if along_u:
        assert u0 % TILE == TILE - 2 and (u1 - 1) % TILE == 1
        g = (v0 + v1) // 2 + int(rs.randint(-8, 9))
        p[g:g + gap, u1 - 1 if far else u0] = False
    else:
        assert v0 % TILE == TILE - 2
        g = (u0 + u1) // 2 + int(rs.randint(-8, 9))
        p[v0, g:g + gap] = False
    return c.out()


def _pairs(p, fixed0, mark, n, along_axis1, blobs=True):
    """pairs of single pixels and of 2x2 blobs, 2 to 6 px apart along one axis (with their rings the closing joins
    those up to 5 px apart and must leave those 6 px apart alone), first member at every offset 60 to 67 modulo 64
    next to [mark]; stacked along the other axis from fixed0, 6 px apart so that the pairs do not join each other.
    mark == n: pairs that touch the last two pixels of the axis instead."""
    q = p if along_axis1 else p.T                            # q[fixed, moving]
    f = fixed0
    if mark == n:
        for blob, last, seps in ((0, n - 1, (2, 3, 4, 5, 6)), (0, n - 2, (5,)), (1, n - 2, (3, 6))):
            for s in seps:
                first = last - s - blob                      # s = distance between the facing edges
                q[f:f + 1 + blob, first:first + 1 + blob] = True
                q[f:f + 1 + blob, last:last + 1 + blob] = True
                f += 6 + blob
        return f
    for blob in ((0, 1) if blobs else (0,)):
        for k, off in enumerate(range(60, 68)):
            s = 2 + (k + 2 * blob) % 5
            first = mark - TILE + off
            second = first + blob + s                        # s = distance between the facing edges
            if second + blob >= n:
                continue
            q[f:f + 1 + blob, first:first + 1 + blob] = True
            q[f:f + 1 + blob, second:second + 1 + blob] = True
            f += 6 + blob
    return f


def seams(shape, seed=0):
    """pairs the closing joins, at every offset 60..67 mod 64 across word and tile seams, in both directions"""
    c = _Canvas(shape)
    lay = c.lay
    S, L = c.S, c.L
    # pairs separated along u, stacked along v, in the columns next to each u mark (the end's above the others')
    # (a partial last word narrower than 24 px leaves no room for the blob pairs next to the border's own structures)
    for m in _marks(L):
        _pairs(c.p, 8 if m == L else 62, m, L, True, blobs=L - m >= 24 or not lay['thin'])
    # pairs separated along v, stacked along u inside the seams slot, next to each v mark
    for k, m in enumerate(_marks(S)):
        _pairs(c.p, lay['seams'][2] + 3 + 104 * k, m, S, False)
    return c.out()


def borders(shape, seed=0):
    """blobs touching the four borders and corners; rings cut by each border (open to the outside: no holes)"""
    c = _Canvas(shape)
    S, L, p = c.S, c.L, c.p
    u0 = c.lay['borders'][2]
    for v in (0, S - 4):
        for u in (0, L - 4):
            p[v:v + 4, u:u + 4] = True
    c.ring(0, u0 + 20, 16, 16)
    p[0:4, u0 + 42:u0 + 47] = True
    c.ring(S - 1, u0 + 62, 16, 16)
    p[S - 4:S, u0 + 14:u0 + 19] = True
    # the two short borders: blob at a third, cut ring further down (thin frames: both below the seam pairs)
    va, vb, r = (122, 144, 10) if c.lay['thin'] else (S // 3, 2 * S // 3, 20)
    for u_blob, u_ring in ((0, 0), (L - 4, L - 1)):
        p[va:va + 5, u_blob:u_blob + 4] = True
        c.ring(vb, u_ring, r, r)
    return c.out()


def sparse(shape, seed=0):
    """-> (plane, bpm): 0.5 % random saturated pixels, three 5x5 blobs and two small rings in the scene's slot; a
    bad-pixel mask over the whole frame with 1 % of the pixels 1, one of them forced at the centre of each small ring
    (inside a hole: such a pixel keeps its 1 and must not become 8)"""
    c = _Canvas(shape)
    rs = np.random.RandomState(seed)
    v0, v1, u0, u1 = c.lay['sparse']
    c.p[v0:v1, u0:u1] = rs.random_sample((v1 - v0, u1 - u0)) < 0.005
    w = u1 - u0
    for k in range(3):
        bv, bu = v0 + 20 + 30 * k, u0 + 10 + (w - 30) * k // 2
        c.p[bv:bv + 5, bu:bu + 5] = True
    bpm_c = (rs.random_sample(c.p.shape) < 0.01).astype(np.uint8)
    for cv, cu in ((v0 + 40, u0 + w // 2 + 20), (v1 - 30, u0 + w // 2 - 20)):
        c.p[cv - 10:cv + 11, cu - 10:cu + 11] = False
        c.ring(cv, cu, 8, 8, t=2)
        bpm_c[cv, cu] = 1
    bpm = np.ascontiguousarray(bpm_c.T) if c.tall else bpm_c
    return c.out(), bpm


def empty(shape, seed=0):
    return np.zeros(shape, bool)


def single(shape, seed=0):
    """one saturated pixel in the middle of a tile away from the border: with its ring it occupies that tile only"""
    p = np.zeros(shape, bool)
    rs = np.random.RandomState(seed)
    ty, tx = int(rs.randint(1, shape[0] // TILE - 1)), int(rs.randint(1, shape[1] // TILE - 1))
    p[ty * TILE + int(rs.randint(8, 56)), tx * TILE + int(rs.randint(8, 56))] = True
    return p


SCENES = ('big_rings', 'serp_open', 'serp_shut', 'pinhole_x', 'pinhole_y', 'pinhole_x_shut', 'pinhole_y_shut', 'seams',
          'borders', 'sparse')


def build(shape, seed=0):
    """every scene on its own plane (same builder calls as compose): name -> plane, plus 'bpm'"""
    sp, bpm = sparse(shape, seed)
    return {'big_rings': big_rings(shape, seed), 'serp_open': serpentine(shape, True, seed),
            'serp_shut': serpentine(shape, False, seed), 'pinhole_x': pinhole(shape, 'x', 5, seed),
            'pinhole_y': pinhole(shape, 'y', 5, seed), 'pinhole_x_shut': pinhole(shape, 'x', 4, seed),
            'pinhole_y_shut': pinhole(shape, 'y', 4, seed), 'seams': seams(shape, seed), 'borders': borders(shape, seed),
            'sparse': sp, 'bpm': bpm}


def boxes(shape):
    """name -> (y0, y1, x0, x1) of the structures whose conditions are counted inside their own box"""
    lay = layout(shape)
    tall = lay['tall']
    b = {'serp_open': lay['serp_open'], 'serp_shut': lay['serp_shut'], 'ring_nested': lay['ring_nested'],
         'ring_edge': lay['ring_edge'], 'sparse': lay['sparse'],
         'pinhole_x': lay['pin_v_open' if tall else 'pin_u_open'], 'pinhole_y': lay['pin_u_open' if tall else 'pin_v_open'],
         'pinhole_x_shut': lay['pin_v_shut' if tall else 'pin_u_shut'],
         'pinhole_y_shut': lay['pin_u_shut' if tall else 'pin_v_shut']}
    if 'ring_word' in lay:
        b['ring_word'] = lay['ring_word']
    return {k: real_box(shape, r) for k, r in b.items()}


def compose(shape, seed=0):
    """-> (planted plane with every scene, bpm, dict of the single planes)"""
    parts = build(shape, seed)
    bpm = parts.pop('bpm')
    plane = np.zeros(shape, bool)
    for p in parts.values():
        plane |= p
    return plane, bpm, parts


# ---- the cases of the tests, built once per process ----------------------------------------------------------------
SEEDS = {'A': 1, 'B': 2, 'C': 3, 'D': 4, 'E': 5, 'F': 6}     # (odd and even: the pinhole's gap on either side of its box)
_CASES = {}


def case(name, scene='all'):
    """geometry name, scene 'all' | 'empty' | 'single' -> dict(ysz, xsz, shape, planted, bpm, parts, mask, nobj): the
    planted plane, and the oracle's mask and NOBJ-SAT for it.  Cached: the host and the GPU tests share one reference."""
    key = (name, scene)
    if key not in _CASES:
        ysz, xsz = GEOMS[name]
        shape = shape_of(name)
        if scene == 'all':
            planted, bpm, parts = compose(shape, SEEDS[name])
        else:
            planted, bpm, parts = {'empty': empty, 'single': single}[scene](shape, SEEDS[name]), None, {}
        mask, nobj = oracle_mask(planted, bpm, ysz, xsz)
        mask.setflags(write=False)
        _CASES[key] = dict(ysz=ysz, xsz=xsz, shape=shape, planted=planted, bpm=bpm, parts=parts, mask=mask, nobj=nobj)
    return _CASES[key]
