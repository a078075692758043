"""A mini (per-box) image brought to frame pixels: scipy.ndimage.zoom(mini, box, order=3, mode='nearest') restated as a
B-spline prefilter and per-row / per-column tap tables (bbx_spline_prefilter, bbx_spline_zoom), zogy.mini2back on top of it,
and MiniImage: the form in which the kernels read a mini image at frame pixels without a frame being made."""
import ctypes as C
import functools
import math

import numpy as np
import torch
from scipy import ndimage

from . import settings
from ._lib import lib, check, push, ptr as _p, SplineImage as _SplineImage

NPAD = 12          # scipy.ndimage.zoom pads 'nearest' inputs by 12 samples before prefiltering


def _bspline_weights(t):
    return np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6,
                     t ** 3 / 6], -1)


def _axis_map(nin, nout, offset):
    o = np.arange(nout)
    cc = o * ((nin - 1) / (nout - 1)) + NPAD if nout > 1 else np.zeros(1) + NPAD
    fl = np.floor(cc).astype(np.int64)
    return (fl + offset).astype(np.int32), _bspline_weights(cc - fl)


@functools.lru_cache(maxsize=16)
def _tap_tables(nby, nbx, box, cy, cx):
    """per-row / per-column tap tables of the zoom (shape-only: cached)"""
    py, px = cy + 2 * NPAD, cx + 2 * NPAD
    fy = np.empty(nby * box, np.int32); wy = np.empty((nby * box, 4))
    fx = np.empty(nbx * box, np.int32); wx = np.empty((nbx * box, 4))
    for iy in range(nby // cy):
        f, w = _axis_map(cy, cy * box, iy * py)
        fy[iy * cy * box:(iy + 1) * cy * box], wy[iy * cy * box:(iy + 1) * cy * box] = f, w
    for ix in range(nbx // cx):
        f, w = _axis_map(cx, cx * box, ix * px)
        fx[ix * cx * box:(ix + 1) * cx * box], wx[ix * cx * box:(ix + 1) * cx * box] = f, w
    for a in (fy, wy, fx, wx):
        a.setflags(write=False)
    return fy, wy, fx, wx


def zoom_coefficients(mini, channels=None):
    """B-spline coefficients of the (edge-padded) mini image; channels=(cy, cx) boxes -> every
    channel block gets its own padded coefficient patch (interp_Xchan=False)"""
    mini = np.asarray(mini, np.float64)
    nby, nbx = mini.shape
    cy, cx = (nby, nbx) if channels is None else channels
    py, px = cy + 2 * NPAD, cx + 2 * NPAD
    coef = np.empty(((nby // cy) * py, (nbx // cx) * px))
    for iy in range(nby // cy):
        for ix in range(nbx // cx):
            blk = np.pad(mini[iy * cy:(iy + 1) * cy, ix * cx:(ix + 1) * cx], NPAD, mode='edge')
            coef[iy * py:(iy + 1) * py, ix * px:(ix + 1) * px] = ndimage.spline_filter(blk, order=3, mode='nearest',
                                                                                      output=np.float64)
    return coef


def zoom_plan(mini, box, channels=None):
    """host part of mini2back: B-spline coefficients of the (edge-padded) mini image and the
    per-row / per-column tap tables for scipy.ndimage.zoom(mini, box, order=3, mode='nearest');
    channels=(cy, cx) boxes -> every channel block gets its own padded coefficient patch
    (interp_Xchan=False)."""
    nby, nbx = np.shape(mini)
    cy, cx = (nby, nbx) if channels is None else channels
    return (zoom_coefficients(mini, channels),) + _tap_tables(nby, nbx, box, cy, cx)


def _device_taps(ctx, nby, nbx, box, cy, cx):
    """the tap tables on the context's device (kept with the context)"""
    cache = ctx.__dict__.setdefault('_zoom_taps', {})
    key = (nby, nbx, box, cy, cx)
    if key not in cache:
        cache[key] = tuple(torch.from_numpy(np.array(a)).to(ctx.device) for a in _tap_tables(*key))      # (writable copies)
    return cache[key]


SPLINE_POLE = -0.2679491924311227          # sqrt(3) - 2 correctly rounded: the constant gcc folds into scipy's ni_splines.c


def device_zoom_coefficients(ctx, mini, channels=None):
    """zoom_coefficients on the device (bbx_spline_prefilter: scipy's prefilter operation by operation, same bits):
    mini = float32 device tensor [nby, nbx] -> float64 device tensor of the padded coefficient patches"""
    nby, nbx = mini.shape
    cy, cx = (nby, nbx) if channels is None else channels
    py, px = cy + 2 * NPAD, cx + 2 * NPAD
    coef = torch.empty(((nby // cy) * py, (nbx // cx) * px), dtype=torch.float64, device=mini.device)
    check(lib.bbx_spline_prefilter(ctx.h, nby, nbx, cy, cx, NPAD, math.pow(SPLINE_POLE, py), math.pow(SPLINE_POLE, px), _p(mini), _p(coef),
                                   ctx.stream()), 'bbx_spline_prefilter', ctx.h)
    return coef


def mini2back(ctx, mini, shape, bkg_boxsize=None, interp_Xchan=True, subtract_from=None, want_bkg=True, subtract_into=None):
    """zogy.mini2back(data_mini, data_shape, order_interp=3, bkg_boxsize, interp_Xchan): full-
    frame background from the mini image; with subtract_from the same pass does `data -= bkg`
    (in place, or into the tensor subtract_into with subtract_from left as it is).  A float32 mini image (device tensor
    or numpy) never leaves the device: the B-spline prefilter runs there too (no host round trip in the frame's path);
    a float64 numpy mini image takes scipy's prefilter on the host."""
    box = bkg_boxsize or settings.bkg_boxsize
    dev = ctx.device
    nby, nbx = mini.shape
    channels = None
    if not interp_Xchan:
        if nby % settings.ny or nbx % settings.nx:
            raise ValueError('interp_Xchan=False needs a whole number of boxes per channel: mini image {}x{} over {}x{} channels'
                             .format(nby, nbx, settings.ny, settings.nx))
        channels = (nby // settings.ny, nbx // settings.nx)
    cy, cx = (nby, nbx) if channels is None else channels
    if not torch.is_tensor(mini) and np.asarray(mini).dtype != np.float32:
        d_coef = torch.from_numpy(zoom_coefficients(np.asarray(mini), channels)).to(dev)
    else:
        d_mini = mini if torch.is_tensor(mini) else push(ctx, np.ascontiguousarray(mini))
        if d_mini.dtype != torch.float32 or not d_mini.is_contiguous():
            d_mini = d_mini.to(torch.float32).contiguous()
        d_coef = device_zoom_coefficients(ctx, d_mini, channels)
    cshape = tuple(d_coef.shape)
    d_fy, d_wy, d_fx, d_wx = _device_taps(ctx, nby, nbx, box, cy, cx)
    ny, nx = shape
    if subtract_into is not None:
        check(lib.bbx_spline_zoom_sub(ctx.h, ny, nx, _p(d_coef), cshape[0], cshape[1], _p(d_fy), _p(d_wy), _p(d_fx),
                                      _p(d_wx), _p(subtract_from), _p(subtract_into), ctx.stream()), 'bbx_spline_zoom_sub', ctx.h)
        return None
    bkg = torch.empty((ny, nx), dtype=torch.float32, device=dev) if want_bkg else None
    check(lib.bbx_spline_zoom(ctx.h, ny, nx, _p(d_coef), cshape[0], cshape[1], _p(d_fy), _p(d_wy), _p(d_fx),
                              _p(d_wx), _p(subtract_from), _p(bkg), ctx.stream()), 'bbx_spline_zoom', ctx.h)
    return bkg


class MiniImage:
    """A mini (per-box) image in the form the kernels read it at frame pixels (bbx_zogy_frame_mini, bbx_psf_optflux_mini):
    the B-spline coefficients of its edge-padded patches on the device + the geometry of zogy.mini2back(mini, shape,
    bkg_boxsize, interp_Xchan).  The full-frame image is never made; frame() makes it for callers that need one."""

    def __init__(self, ctx, mini, box, interp_Xchan=True):
        nby, nbx = mini.shape
        self.channels = None
        if not interp_Xchan:
            if nby % settings.ny or nbx % settings.nx:
                raise ValueError('interp_Xchan=False needs a whole number of boxes per channel: mini image {}x{} over {}x{} channels'
                                 .format(nby, nbx, settings.ny, settings.nx))
            self.channels = (nby // settings.ny, nbx // settings.nx)
        cy, cx = (nby, nbx) if self.channels is None else self.channels
        if torch.is_tensor(mini) or np.asarray(mini).dtype == np.float32:
            d_mini = mini if torch.is_tensor(mini) else push(ctx, np.ascontiguousarray(mini))
            if d_mini.dtype != torch.float32 or not d_mini.is_contiguous():
                d_mini = d_mini.to(torch.float32).contiguous()
            self.coef = device_zoom_coefficients(ctx, d_mini, self.channels)
        else:
            self.coef = torch.from_numpy(zoom_coefficients(np.asarray(mini), self.channels)).to(ctx.device)
        self.box, self.shape = int(box), (nby * int(box), nbx * int(box))
        self.c = _SplineImage(self.coef.data_ptr(), nby, nbx, cy, cx, int(box), NPAD)

    def ref(self):
        return C.byref(self.c)

    def frame(self, ctx):
        """the full-frame image (bbx_spline_zoom of the same coefficients)"""
        nby, nbx = self.c.nby, self.c.nbx
        d_fy, d_wy, d_fx, d_wx = _device_taps(ctx, nby, nbx, self.box, self.c.cy, self.c.cx)
        out = torch.empty(self.shape, dtype=torch.float32, device=ctx.device)
        check(lib.bbx_spline_zoom(ctx.h, self.shape[0], self.shape[1], _p(self.coef), self.coef.shape[0], self.coef.shape[1], _p(d_fy), _p(d_wy),
                                  _p(d_fx), _p(d_wx), None, _p(out), ctx.stream()), 'bbx_spline_zoom', ctx.h)
        return out


def remap_mini(mini, grid, shape_in, box, step, shape_out=None):
    """a mini (per-box) image of the reference frame sampled on the new frame's box centres:
    bilinear interpolation of [mini] at the reference-frame positions that the projection
    lattice [grid] (coadd.projection_grid: [gny][gnx][2] = x, y input position of the output
    pixels (j*step, i*step)) assigns to the centres of the new frame's boxes.  Host, float64:
    176 x 176 values.  shape_out: the new frame's shape: the result has the new frame's boxes (None: as many as the reference's
    mini image has, which is the same thing only for two frames of one shape)."""
    mini = np.asarray(mini, np.float64)
    nby, nbx = mini.shape if shape_out is None else (shape_out[0] // box, shape_out[1] // box)
    cy = (np.arange(nby) + 0.5) * box - 0.5
    cx = (np.arange(nbx) + 0.5) * box - 0.5
    gy, gx = cy / step, cx / step
    j0 = np.clip(np.floor(gy).astype(int), 0, grid.shape[0] - 2); fy = (gy - j0)[:, None]
    i0 = np.clip(np.floor(gx).astype(int), 0, grid.shape[1] - 2); fx = (gx - i0)[None, :]
    g00, g01 = grid[j0][:, i0], grid[j0][:, i0 + 1]
    g10, g11 = grid[j0 + 1][:, i0], grid[j0 + 1][:, i0 + 1]
    pos = ((1 - fy) * (1 - fx))[..., None] * g00 + ((1 - fy) * fx)[..., None] * g01 + \
          (fy * (1 - fx))[..., None] * g10 + (fy * fx)[..., None] * g11
    # position in box units of the reference frame's mini image (box centres at k + 0.5)
    by = np.clip((pos[..., 1] + 0.5) / box - 0.5, 0, shape_in[0] // box - 1)
    bx = np.clip((pos[..., 0] + 0.5) / box - 0.5, 0, shape_in[1] // box - 1)
    y0 = np.clip(np.floor(by).astype(int), 0, mini.shape[0] - 2); wy = by - y0
    x0 = np.clip(np.floor(bx).astype(int), 0, mini.shape[1] - 2); wx = bx - x0
    out = (1 - wy) * (1 - wx) * mini[y0, x0] + (1 - wy) * wx * mini[y0, x0 + 1] + \
          wy * (1 - wx) * mini[y0 + 1, x0] + wy * wx * mini[y0 + 1, x0 + 1]
    return out.astype(np.float32)
