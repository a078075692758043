"""Astrometric solution of the new frame from a star catalogue (bbx_wcs.hip + the chain of bbx_align.hip): the
catalogue on the device, the pointing of a frame, the solve, the FITS WCS that states its result and the A-* header keys.

[EXT] zogy solves with astrometry.net, which is not in the reference tree: only the key names follow the reference
(blackbox.py:3067-3084, 3144-3145); the method and its rules are this project's own, stated in include/bbx.h and in float64 numpy by
tests/astrometry_ref.py.  The catalogue, projected about the telescope's pointing onto a virtual pixel grid of the frame's shape at
the nominal geometry, is a star list like the reference's: the chain that registers the reference (align.align_chain) finds T, frame
pixels -> virtual-grid pixels, and sky = inverse gnomonic(CD0 (T(x, y) - centre)).  Because the tangent point stays the pointing,
that composition IS a TAN[-SIP] header in closed form (wcs_header)."""
import os

import numpy as np
import torch

from . import fitsio, settings
from ._lib import lib, check, fetch, ptr as _p, expect as _expect
from .align import ALIGN_FEW_PAIRS, _expect_list, align_chain

D2R, R2D = 0.017453292519943295, 57.29577951308232
AST_MARGIN = 16.0                                                      # [pix] rows this far beyond ast_max_shift outside the frame still enter list B
# the keys of a frame with the switch on, in the order they are written; a solve that failed: A-P False, 'None' for the rest
WCS_KEYS = ('CTYPE1', 'CTYPE2', 'CRVAL1', 'CRVAL2', 'CRPIX1', 'CRPIX2', 'CD1_1', 'CD1_2', 'CD2_1', 'CD2_2', 'RADESYS')
SIP_KEYS = ('A_ORDER', 'B_ORDER', 'A_2_0', 'A_1_1', 'A_0_2', 'B_2_0', 'B_1_1', 'B_0_2')
AST_KEYS = (('A-PSCALE', '[arcsec/pix] pixel scale WCS solution'), ('A-PSCALX', '[arcsec/pix] X-axis pixel scale WCS solution'),
            ('A-PSCALY', '[arcsec/pix] Y-axis pixel scale WCS solution'), ('A-ROT', '[deg] rotation WCS solution (E of N for "up")'),
            ('A-ROTX', '[deg] X-axis rotation WCS (E of N for "up")'), ('A-ROTY', '[deg] Y-axis rotation WCS (E of N for "up")'),
            ('A-CAT-F', 'astrometric catalog'), ('A-NAST', 'sources used in the astrometric solution'),
            ('A-TNAST', 'catalogue rows in the field'), ('A-DRA', '[arcsec] dRA cos(DEC) mean offset to astrom. catalog'),
            ('A-DRASTD', '[arcsec] dRA sigma (STD) offset'), ('A-DDEC', '[arcsec] dDEC mean offset to astrom. catalog'),
            ('A-DDESTD', '[arcsec] dDEC sigma (STD) offset'), ('RA-CNTR', '[deg] RA (ICRS) at image center'),
            ('DEC-CNTR', '[deg] DEC (ICRS) at image center'), ('A-PLDG', 'degree of the astrometric polynomial'),
            ('A-NVOTE', 'votes of the winning offset block'), ('A-MSHFT', '[pix] offset of the catalogue grid at the frame centre'),
            ('A-FLAGS', 'flags: 1 vote 2 pairs 4 singular 8 det'))


# ---- inputs --------------------------------------------------------------------------------------------------------
class AstCatalog:
    """the catalogue on the device: sky float64 [n, 2] = (RA, DEC) in degrees (ICRS), mag float32 [n]; name: what A-CAT-F states"""

    def __init__(self, ctx, ra, dec, mag, name='None', max_rows=None):
        ra, dec, mag = (np.asarray(t).reshape(-1) for t in (ra, dec, mag))
        if not (ra.size == dec.size == mag.size):
            raise ValueError('astrometric catalogue: columns of {} / {} / {} rows'.format(ra.size, dec.size, mag.size))
        max_rows = settings.ast_cat_max if max_rows is None else int(max_rows)
        if ra.size > max_rows:
            raise ValueError('astrometric catalogue: {} rows, more than ast_cat_max = {}'.format(ra.size, max_rows))
        self.n, self.name = int(ra.size), str(name)
        sky = np.ascontiguousarray(np.stack([ra.astype(np.float64), dec.astype(np.float64)], axis=1))
        self.sky = torch.from_numpy(sky).to(ctx.device)
        self.mag = torch.from_numpy(np.ascontiguousarray(mag.astype(np.float32))).to(ctx.device)


def load_catalog(ctx, path, cols=None, max_rows=None):
    """--ast_cat: the FITS binary table [path] with the columns cols = (RA, DEC, MAG) (settings.ast_cat_cols) -> AstCatalog.  A
    missing column or more than ast_cat_max rows: ValueError, before any frame runs"""
    cols = tuple(settings.ast_cat_cols if cols is None else cols)
    if len(cols) != 3:
        raise ValueError('ast_cat_cols: three column names (RA, DEC, MAG) expected, got {!r}'.format(cols))
    table, _ = fitsio.read_table(path)
    missing = [c for c in cols if c not in table]
    if missing:
        raise ValueError('astrometric catalogue {}: no column {} (it has {})'.format(path, ', '.join(missing), ', '.join(table)))
    return AstCatalog(ctx, table[cols[0]], table[cols[1]], table[cols[2]], name=os.path.basename(str(path)), max_rows=max_rows)


def _angle(value, hours):
    """a header coordinate: degrees as a number, or sexagesimal with ':' (hours when [hours]) -> degrees"""
    if isinstance(value, tuple):
        value = value[0]
    if isinstance(value, str):
        s = value.strip()
        if ':' in s:
            sign = -1.0 if s.startswith('-') else 1.0
            parts = [float(p) for p in s.lstrip('+-').split(':')]
            parts += [0.0] * (3 - len(parts))
            v = sign * (parts[0] + parts[1] / 60.0 + parts[2] / 3600.0)
            return v * 15.0 if hours else v
        return float(s)
    return float(value)


def frame_pointing(header, ra=None, dec=None):
    """the pointing (RA, DEC) in degrees of a frame: --ast_ra / --ast_dec where given, else the header's RA, DEC as the reduced
    header carries them (degrees, or sexagesimal with ':' and RA in hours).  They are taken to be ICRS coordinates of the date
    of the catalogue, near the frame's centre: no precession, no epoch.  None: the header has no usable pair"""
    try:
        a = float(ra) if ra is not None else _angle(header['RA'], True)
        d = float(dec) if dec is not None else _angle(header['DEC'], False)
    except (KeyError, TypeError, ValueError, IndexError):
        return None
    if not (np.isfinite(a) and np.isfinite(d) and abs(d) <= 90.0):
        return None
    return float(a % 360.0), float(d)


def cd0(pixscale=None, rot=None, parity=None):
    """CD0 [deg / pix] float64 [2, 2] of the nominal geometry: (s / 3600) [[-p cos r, -sin r], [-p sin r, cos r]], the FITS CROTA2
    convention (parity +1: north up, east left at rotation 0)"""
    s = float(settings.pixscale if pixscale is None else pixscale) / 3600.0
    r = float(settings.ast_rot if rot is None else rot) * D2R
    p = float(settings.ast_parity if parity is None else parity)
    if p not in (1.0, -1.0) or not s > 0:
        raise ValueError('astrometry: parity +1 or -1 and a positive pixel scale expected')
    return s * np.array([[-p * np.cos(r), -np.sin(r)], [-p * np.sin(r), np.cos(r)]], np.float64)


def _cd_arg(cd):
    cd = np.ascontiguousarray(np.asarray(cd, np.float64).reshape(4))
    return cd, cd.ctypes.data_as(lib.bbx_wcs_pix2sky.argtypes[9])


# ---- device entries ------------------------------------------------------------------------------------------------
def cat_list(ctx, cat, pointing, shape, cd, margin, mag_zp=None):
    """bbx_wcs_cat_list: the catalogue as list B on the virtual grid of a frame of [shape] -> device ((ys, xs, off, flux, err),
    count int32 [1] of the eligible rows).  No host wait"""
    mag_zp = settings.ast_mag_zp if mag_zp is None else mag_zp
    n, dev = cat.n, ctx.device
    _expect(cat.sky, torch.float64, (n, 2), 'catalogue positions')
    _expect(cat.mag, torch.float32, (n,), 'catalogue magnitudes')
    ys, xs = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty((n, 2), dtype=torch.float32, device=dev)
    flux, err = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    cd, pcd = _cd_arg(cd)
    check(lib.bbx_wcs_cat_list(ctx.h, n, _p(cat.sky), _p(cat.mag), float(pointing[0]), float(pointing[1]), int(shape[0]), int(shape[1]), pcd,
                               float(margin), float(mag_zp), _p(ys), _p(xs), _p(off), _p(flux), _p(err), _p(count), ctx.stream()),
          'bbx_wcs_cat_list', ctx.h)
    return (ys, xs, off, flux, err), count


def pix2sky(ctx, coef, shape, cd, pointing, pos=None, ys=None, xs=None, off=None):
    """bbx_wcs_pix2sky: 0-based frame positions -> device float64 [n, 2] = (RA, DEC).  pos: device float64 [n, 2] = (x, y); or the
    int32 peaks (ys, xs) with float32 offsets off [n, 2] = (dy, dx) (None: the integers).  coef: device float64 [12].  No host wait"""
    _expect(coef, torch.float64, (12,), 'coef')
    if pos is not None:
        n = int(pos.shape[0])
        _expect(pos, torch.float64, (n, 2), 'positions')
    else:
        n = int(ys.numel())
        _expect(ys, torch.int32, (n,), 'ys')
        _expect(xs, torch.int32, (n,), 'xs')
        if off is not None:
            _expect(off, torch.float32, (n, 2), 'offsets')
    sky = torch.empty((n, 2), dtype=torch.float64, device=ctx.device)
    cd, pcd = _cd_arg(cd)
    check(lib.bbx_wcs_pix2sky(ctx.h, n, _p(pos), _p(ys), _p(xs), _p(off), _p(coef), int(shape[0]), int(shape[1]), pcd, float(pointing[0]),
                              float(pointing[1]), _p(sky), ctx.stream()), 'bbx_wcs_pix2sky', ctx.h)
    return sky


def pair_stats(ctx, items, kept, a, cat, coef, shape, cd, pointing):
    """bbx_wcs_pair_stats: the residuals against the catalogue of the pairs items int32 [N, 2] that the last fit kept (uint8 [N])
    -> device float64 [8] = (count, mean dRA cos DEC, its std, mean dDEC, its std [arcsec], 0, 0, 0).  No host wait"""
    N = int(items.shape[0])
    _expect(items, torch.int32, (N, 2), 'items')
    _expect(kept, torch.uint8, (N,), 'kept')
    _expect(coef, torch.float64, (12,), 'coef')
    n_a = _expect_list(a, 'list a', 3)
    _expect(cat.sky, torch.float64, (cat.n, 2), 'catalogue positions')
    out = torch.tensor([0.0] + [float('nan')] * 4 + [0.0] * 3, dtype=torch.float64).to(ctx.device) if N == 0 else \
        torch.empty(8, dtype=torch.float64, device=ctx.device)
    cd, pcd = _cd_arg(cd)
    check(lib.bbx_wcs_pair_stats(ctx.h, N, _p(items), _p(kept), n_a, _p(a[0]), _p(a[1]), _p(a[2]), cat.n, _p(cat.sky), _p(coef), int(shape[0]),
                                 int(shape[1]), pcd, float(pointing[0]), float(pointing[1]), _p(out), ctx.stream()), 'bbx_wcs_pair_stats', ctx.h)
    return out


# ---- host: rule 5 and the header -----------------------------------------------------------------------------------
def _transform(coef, shape, x, y):
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    u, v = (np.asarray(x, np.float64) - hx) / hx, (np.asarray(y, np.float64) - hy) / hy
    b = (np.ones_like(u), u, v, u * u, u * v, v * v)
    X, Y = np.zeros_like(u), np.zeros_like(u)
    for t in range(6):
        X, Y = X + b[t] * coef[t], Y + b[t] * coef[6 + t]
    return X, Y


def sky_of_std(xi, eta, ra0, dec0):
    """the inverse gnomonic projection, (xi, eta) in degrees about (ra0, dec0) -> (RA in [0, 360), DEC) in degrees; numpy"""
    with np.errstate(all='ignore'):
        x, e, d0 = np.asarray(xi, np.float64) * D2R, np.asarray(eta, np.float64) * D2R, float(dec0) * D2R
        sd0, cd0_ = np.sin(d0), np.cos(d0)
        den = cd0_ - e * sd0
        a = float(ra0) + np.arctan2(x, den) * R2D
        a = a - 360.0 * np.floor(a / 360.0)
        a = np.where(a >= 360.0, 0.0, a)
        return a, np.arctan2(sd0 + e * cd0_, np.hypot(x, den)) * R2D


def pix2sky_host(coef, shape, cd, pointing, x, y):
    """rule 5 in float64 numpy: 0-based frame positions -> (RA, DEC) in degrees"""
    cd = np.asarray(cd, np.float64).reshape(4)
    X, Y = _transform(np.asarray(coef, np.float64), shape, x, y)
    dx, dy = X - 0.5 * (shape[1] - 1), Y - 0.5 * (shape[0] - 1)
    return sky_of_std(cd[0] * dx + cd[1] * dy, cd[2] * dx + cd[3] * dy, pointing[0], pointing[1])


def _jacobian(coef, shape, x, y):
    """dT / d(x, y) in pixels at (x, y) -> [[dX/dx, dX/dy], [dY/dx, dY/dy]]"""
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    u, v = (x - hx) / hx, (y - hy) / hy
    c, d = coef[:6], coef[6:12]
    return np.array([[(c[1] + 2.0 * c[3] * u + c[4] * v) / hx, (c[2] + c[4] * u + 2.0 * c[5] * v) / hy],
                     [(d[1] + 2.0 * d[3] * u + d[4] * v) / hx, (d[2] + d[4] * u + 2.0 * d[5] * v) / hy]], np.float64)


def wcs_header(coef, shape, poldeg, cd, pointing):
    """The FITS WCS of T, in closed form (host, float64): CRVAL = the pointing (the tangent point of the virtual grid, which is
    what makes the header exact), CRPIX = 1 + x0 with T(x0) = the grid's centre (Newton from the frame centre), CD = CD0 J(x0);
    degree 2: the SIP terms A, B of order 2 = J(x0)^-1 (second-order part of T), which re-expanded about x0 is T's own -> {key:
    (value, comment)}, also A-PSCALE, A-PSCALX, A-PSCALY, A-ROT, A-ROTX, A-ROTY.  ValueError where Newton does not converge"""
    coef, cd = np.asarray(coef, np.float64), np.asarray(cd, np.float64).reshape(2, 2)
    ny, nx = int(shape[0]), int(shape[1])
    xc, yc = 0.5 * (nx - 1), 0.5 * (ny - 1)
    p = np.array([xc, yc])
    for _ in range(50):
        X, Y = _transform(coef, shape, p[0], p[1])
        step = np.linalg.solve(_jacobian(coef, shape, p[0], p[1]), np.array([float(X) - xc, float(Y) - yc]))
        p = p - step
        if not np.isfinite(p).all():
            break
        if np.abs(step).max() < 1e-13 * max(nx, ny):
            break
    else:
        raise ValueError('wcs_header: no root of T(x) = centre')
    if not np.isfinite(p).all():
        raise ValueError('wcs_header: no root of T(x) = centre')
    J = _jacobian(coef, shape, p[0], p[1])
    CD = cd @ J
    sip = poldeg == 2
    hdr = {'CTYPE1': ('RA---TAN-SIP' if sip else 'RA---TAN', 'gnomonic projection' + (' + SIP distortion' if sip else '')),
           'CTYPE2': ('DEC--TAN-SIP' if sip else 'DEC--TAN', ''),
           'CRVAL1': (float(pointing[0]), '[deg] RA of the tangent point'), 'CRVAL2': (float(pointing[1]), '[deg] DEC of the tangent point'),
           'CRPIX1': (float(p[0] + 1.0), '[pix] tangent point'), 'CRPIX2': (float(p[1] + 1.0), '[pix] tangent point'),
           'CD1_1': (float(CD[0, 0]), '[deg/pix]'), 'CD1_2': (float(CD[0, 1]), '[deg/pix]'), 'CD2_1': (float(CD[1, 0]), '[deg/pix]'),
           'CD2_2': (float(CD[1, 1]), '[deg/pix]'), 'RADESYS': ('ICRS', 'reference system of the catalogue')}
    if sip:
        hy, hx = 0.5 * ny, 0.5 * nx
        Q = np.array([[coef[3] / (hx * hx), coef[4] / (hx * hy), coef[5] / (hy * hy)],
                      [coef[9] / (hx * hx), coef[10] / (hx * hy), coef[11] / (hy * hy)]])
        AB = np.linalg.solve(J, Q)
        hdr['A_ORDER'], hdr['B_ORDER'] = (2, 'SIP polynomial order, axis 1'), (2, 'SIP polynomial order, axis 2')
        for row, name in enumerate('AB'):
            for col, pq in enumerate(('2_0', '1_1', '0_2')):
                hdr['{}_{}'.format(name, pq)] = (float(AB[row, col]), 'SIP distortion coefficient')
    # derived: the scales along the two pixel axes [arcsec], and the position angle (E of N) of each axis' "up"
    sx, sy = float(np.hypot(CD[0, 0], CD[1, 0]) * 3600.0), float(np.hypot(CD[0, 1], CD[1, 1]) * 3600.0)
    par = -1.0 if np.linalg.det(CD) < 0 else 1.0                          # (det < 0: east left of north, the sky's usual)
    rot_y = float(np.degrees(np.arctan2(-CD[0, 1], CD[1, 1])))
    rot_x = float(np.degrees(np.arctan2(par * CD[1, 0], par * CD[0, 0])))
    d = (rot_x - rot_y + 180.0) % 360.0 - 180.0
    hdr.update({'A-PSCALE': (float(np.sqrt(abs(np.linalg.det(CD))) * 3600.0), AST_KEYS[0][1]), 'A-PSCALX': (sx, AST_KEYS[1][1]),
                'A-PSCALY': (sy, AST_KEYS[2][1]), 'A-ROT': (float(rot_y + 0.5 * d), AST_KEYS[3][1]), 'A-ROTX': (rot_x, AST_KEYS[4][1]),
                'A-ROTY': (rot_y, AST_KEYS[5][1])})
    return hdr


def _hv(header, key, default=None):
    v = header.get(key, default)
    return v[0] if isinstance(v, tuple) else v


def wcs_pix2sky(header, x, y):
    """a TAN or TAN-SIP header evaluated in float64 numpy: FITS pixel coordinates (1-based) -> (RA, DEC) in degrees.  Used by
    nothing on the hot path: it is what a reader of the products does"""
    ct = str(_hv(header, 'CTYPE1')).strip()
    if not ct.startswith('RA---TAN'):
        raise ValueError('wcs_pix2sky: CTYPE1 {!r} is not a TAN projection'.format(ct))
    u = np.asarray(x, np.float64) - float(_hv(header, 'CRPIX1'))
    v = np.asarray(y, np.float64) - float(_hv(header, 'CRPIX2'))
    U, V = u, v
    if ct.endswith('-SIP'):
        for name, order_key in (('A', 'A_ORDER'), ('B', 'B_ORDER')):
            order = int(_hv(header, order_key))
            f = np.zeros_like(u)
            for p in range(order + 1):
                for q in range(order + 1 - p):
                    k = '{}_{}_{}'.format(name, p, q)
                    if k in header:
                        f = f + float(_hv(header, k)) * u ** p * v ** q
            if name == 'A':
                U = u + f
            else:
                V = v + f
    xi = float(_hv(header, 'CD1_1')) * U + float(_hv(header, 'CD1_2')) * V
    eta = float(_hv(header, 'CD2_1')) * U + float(_hv(header, 'CD2_2')) * V
    return sky_of_std(xi, eta, float(_hv(header, 'CRVAL1')), float(_hv(header, 'CRVAL2')))


def ast_header(sol=None):
    """the keys of a frame with the switch on.  sol: a solution that succeeded (solve_finish's dict); else: A-P False and the string
    'None' (set_qc's default) for every other key (the flag word of a solve that failed stays in its dict and in the log).  No WCS
    key without a solution"""
    if sol is None or not sol.get('ok'):
        hdr = {'A-P': (False, 'successfully processed by astrometric solve?')}
        for k, c in AST_KEYS:
            hdr[k] = ('None', c)
        return hdr
    return dict(sol['header'])


# ---- the solve -----------------------------------------------------------------------------------------------------
def solve_enqueue(ctx, new_list, cat, pointing, shape, pixscale=None, rot=None, parity=None, max_shift=None, bin=None, poldeg=None,
                  rounds=None, dist=None, snr_min=None, mag_zp=None, nbright=None):
    """The solve, queued on ctx's stream without a host wait: the catalogue as list B (bbx_wcs_cat_list), align_chain with A =
    new_list = the frame's (ys, xs, off, flux, err) sorted by (y, x), the residuals of the last fit's pairs (bbx_wcs_pair_stats)
    -> dict(coef: device float64 [12] for pix2sky, back: the six small device tensors solve_finish wants on the host, ...)"""
    poldeg = int(settings.ast_poldeg if poldeg is None else poldeg)
    if poldeg not in (1, 2):
        raise ValueError('astrometry: degree 1 or 2, got {}'.format(poldeg))
    rounds = int(settings.ast_rounds if rounds is None else rounds)
    max_shift = float(settings.ast_max_shift if max_shift is None else max_shift)
    bin = float(settings.ast_bin if bin is None else bin)
    dist = settings.ast_dist if dist is None else dist
    dist = float(settings.match_dist_pix if dist is None else dist)
    if pointing is None:
        raise ValueError('astrometry: the frame has no usable pointing (header RA, DEC or --ast_ra --ast_dec)')
    cd = cd0(pixscale, rot, parity)
    a = tuple(new_list)
    b, count = cat_list(ctx, cat, pointing, shape, cd, max_shift + AST_MARGIN, mag_zp)
    info, coarse, coef, stats, items, kept = align_chain(ctx, a, b, shape, poldeg, rounds, dist, snr_min, nbright, max_shift, bin)
    pst = pair_stats(ctx, items, kept, a, cat, coef, shape, cd, pointing)
    return dict(coef=coef, back=[coef, stats, info, coarse, count, pst], cd=cd, pointing=(float(pointing[0]), float(pointing[1])),
                shape=(int(shape[0]), int(shape[1])), poldeg=poldeg, cat=cat, items=items, kept=kept, b=b)


def solve_finish(pending, got):
    """got: the host copies of pending['back'] -> dict(ok, flags, coef, header, fit, n_eligible, resid, ...).  ok False: the
    chain's flag word is not 0, a coefficient is not finite, or the header cannot be formed; header is then ast_header(None)"""
    h_coef, h_stats, h_info, h_coarse, h_count, h_pst = (np.asarray(t) for t in got)
    flags = int(h_stats[3]) | int(h_info[5])
    if not np.isfinite(h_coef).all():
        flags |= int(h_stats[3]) or ALIGN_FEW_PAIRS
    shape, cd, pointing, poldeg = pending['shape'], pending['cd'], pending['pointing'], pending['poldeg']
    fit = dict(coef=h_coef, n_used=int(h_stats[0]), rms_x=float(h_stats[1]), rms_y=float(h_stats[2]), flags=flags, info=h_info, coarse=h_coarse)
    sol = dict(ok=False, flags=flags, coef=h_coef, d_coef=pending['coef'], fit=fit, n_eligible=int(h_count[0]), resid=h_pst[:5].copy(),
               cd=cd, pointing=pointing, shape=shape, poldeg=poldeg)
    if flags == 0:
        try:
            hdr = wcs_header(h_coef, shape, poldeg, cd, pointing)
            xc, yc = 0.5 * (shape[1] - 1), 0.5 * (shape[0] - 1)
            X, Y = _transform(h_coef, shape, xc, yc)
            ra_c, dec_c = pix2sky_host(h_coef, shape, cd, pointing, xc, yc)
            vals = {'A-CAT-F': pending['cat'].name, 'A-NAST': int(h_pst[0]), 'A-TNAST': int(h_count[0]), 'A-DRA': float(h_pst[1]),
                    'A-DRASTD': float(h_pst[2]), 'A-DDEC': float(h_pst[3]), 'A-DDESTD': float(h_pst[4]), 'RA-CNTR': float(ra_c),
                    'DEC-CNTR': float(dec_c), 'A-PLDG': poldeg, 'A-NVOTE': int(h_info[0]),
                    'A-MSHFT': float(np.hypot(float(X) - xc, float(Y) - yc)), 'A-FLAGS': 0}
            if not all(np.isfinite(v) for v in vals.values() if isinstance(v, float)) or \
                    not all(np.isfinite(v[0]) for v in hdr.values() if isinstance(v[0], float)):
                raise ValueError('a key of the solution is not finite')
            out = {k: hdr[k] for k in WCS_KEYS + (SIP_KEYS if poldeg == 2 else ())}
            out['A-P'] = (True, 'successfully processed by astrometric solve?')
            for k, c in AST_KEYS:
                out[k] = hdr[k] if k in hdr else (vals[k], c)
            sol.update(ok=True, header=out)
        except (ValueError, np.linalg.LinAlgError):
            sol['ok'] = False
    if not sol['ok']:
        sol['header'] = ast_header(None)
    return sol


def solve(ctx, new_list, cat, pointing, shape, **kw):
    """solve_enqueue + ONE host wait + solve_finish"""
    pending = solve_enqueue(ctx, new_list, cat, pointing, shape, **kw)
    sol = solve_finish(pending, fetch(ctx, *pending['back']))
    sol['pending'] = pending
    return sol
