"""Numerical core of zogy.optimal_subtraction on the GPU: background mesh, sub-image ZOGY
(rocFFT), PSF photometry.  Call sites in the reference: blackbox.py:2350-2354 / 2460-2465;
helper signatures seen in buildref.py:2398-2405, 2480-2495, 3357-3366.

[EXT] zogy itself is not part of /root/reference: the conventions are those of
oracle/zogy_core.py (parity unpinned).  Astrometry, PSFEx,
SExtractor and the real-bogus CNN stay out of scope: PSF images and a WCS-aligned
reference frame are inputs.
"""
import ctypes as C

import numpy as np
import torch
from scipy import ndimage

from . import settings
from ._lib import lib, check, fetch, push, BBXError as _lib_BBXError, SplineImage as _SplineImage
from ._lib import BBX_OPT_ZOGY_KSMALL_OFF          # noqa: F401  (k_n, k_r through the full grid: tests and timings compare the paths)
from .catalogs import format_cat, transient_table         # noqa: F401  (zogy.format_cat)

BBX_ERR_OVERFLOW, BBX_ERR_PSFWIN = -4, -6          # include/bbx.h
BBX_OPT_ZOGY_KWIN_OFF = 4
NPAD = 12          # scipy.ndimage.zoom pads 'nearest' inputs by 12 samples before prefiltering


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---- background mesh --------------------------------------------------------------------
def get_back(ctx, data, data_mask, objmask=None, bkg_boxsize=None, limfrac=0.5):
    """-> (mini_median, mini_std) float32 device tensors (ny/box, nx/box), NaN boxes filled
    and 3x3-median filtered (zogy.get_back)"""
    box = bkg_boxsize or settings.bkg_boxsize
    ny, nx = data.shape
    nby, nbx = ny // box, nx // box
    med = torch.empty((nby, nbx), dtype=torch.float32, device=ctx.device)
    std = torch.empty((nby, nbx), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_bkg_boxstats(ctx.h, ny, nx, box, _p(data), _p(data_mask), _p(objmask), float(limfrac), _p(med), _p(std),
                               ctx.stream()), 'bbx_bkg_boxstats', ctx.h)
    for m in (med, std):
        check(lib.bbx_mini_fill_filter(ctx.h, nby, nbx, _p(m), ctx.stream()), 'bbx_mini_fill_filter', ctx.h)
    return med, std


def object_mask_enqueue(ctx, img, sig_mini, box, nsigma=None, minarea=None, grow=None, filter=None, max_pixels=None):
    """queue bbx_object_mask -> (objmask, d_counts): device uint8 [ny, nx] and device int32 [3] (pixels listed, components
    kept, pixels set); no host wait.  The defaults are the settings'"""
    nsigma = settings.objmask_nsigma if nsigma is None else nsigma
    minarea = settings.objmask_minarea if minarea is None else minarea
    grow = settings.objmask_grow if grow is None else grow
    filter = settings.objmask_filter if filter is None else filter
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    ny, nx = img.shape
    box = int(box)
    if box < 1 or ny % box or nx % box or tuple(sig_mini.shape) != (ny // box, nx // box):
        raise ValueError('sigma mini image of {} x {} boxes of {} px expected'.format(ny // max(box, 1), nx // max(box, 1), box))
    if not (float(nsigma) > 0) or int(minarea) < 1 or not 0 <= int(grow) <= 8:
        raise ValueError('object mask: nsigma > 0, minarea >= 1 and 0 <= grow <= 8 expected')
    sig = sig_mini if torch.is_tensor(sig_mini) else push(ctx, np.ascontiguousarray(sig_mini, np.float32))
    if sig.dtype != torch.float32 or not sig.is_contiguous():
        sig = sig.to(torch.float32).contiguous()
    objmask = torch.empty((ny, nx), dtype=torch.uint8, device=ctx.device)
    d_counts = torch.empty(3, dtype=torch.int32, device=ctx.device)
    check(lib.bbx_object_mask(ctx.h, ny, nx, _p(img), _p(sig), box, float(nsigma), int(minarea), int(grow), int(bool(filter)),
                              int(max_pixels or 0), _p(objmask), _p(d_counts), ctx.stream()), 'bbx_object_mask', ctx.h)
    return objmask, d_counts


def _objmask_counts(c, npix):
    return dict(n_listed=int(c[0]), n_objects=int(c[1]), n_masked=int(c[2]), frac=int(c[2]) / float(npix))


def object_mask(ctx, img, sig_mini, box, nsigma=None, minarea=None, grow=None, filter=None, max_pixels=None):
    """Object mask of a background-subtracted frame: the pixels of the 3x3-smoothed frame [img] at or above
    nsigma x the sigma of their box ([sig_mini]: the filled and filtered sigma mini image of get_back), their 8-connected
    components of at least [minarea] pixels, each pixel of those grown by a disk of radius [grow]
    -> (objmask: device uint8 [ny, nx], 1 = object; counts: dict(n_listed, n_objects, n_masked, frac)).
    One host wait, which also reads the context's device error word: more listed pixels than [max_pixels] (default:
    max(npix / 8, min(npix, 65536))) raise BBXError (BBX_ERR_OVERFLOW) here"""
    objmask, d_counts = object_mask_enqueue(ctx, img, sig_mini, box, nsigma, minarea, grow, filter, max_pixels)
    return objmask, _objmask_counts(fetch(ctx, d_counts, check_device_errors=True), img.numel())


def _objmask_stage(ctx, new, new_mask, work, mini, mini_std, box, nsigma=None, minarea=None, grow=None, max_frac=None):
    """the object-mask stage of optimal_subtraction: [work] holds the first pass's background-subtracted frame, (mini, mini_std)
    that pass's mesh.  -> dict(header, objmask, mini, mini_std, bkg_mini_pass1, bkg_std_mini_pass1); objmask None: the frame
    keeps its first pass (list overflow, an exception, a mask over more than max_frac of the frame; one log line says which).
    One host wait: the counters, the device error word and the first pass's mini images come back together.  [work] is not written"""
    import logging
    log = logging.getLogger(__name__)
    nsigma = float(settings.objmask_nsigma if nsigma is None else nsigma)
    minarea = int(settings.objmask_minarea if minarea is None else minarea)
    grow = int(settings.objmask_grow if grow is None else grow)
    max_frac = float(settings.objmask_max_frac if max_frac is None else max_frac)
    hdr = {'OBJM-P': (False, 'object mask made and used for the background?'),
           'OBJM-THR': (nsigma, '[sigma] object mask detection threshold'),
           'OBJM-MIN': (minarea, '[pix] object mask minimum area'),
           'OBJM-GRW': (grow, '[pix] object mask growth radius'),
           'OBJM-NPX': ('None', 'number of pixels above the threshold'),
           'OBJM-NOB': ('None', 'number of objects in the object mask'),
           'OBJM-FRC': ('None', 'fraction of the frame in the object mask'),
           'S-BKG1': ('None', '[e-] median background, first pass'),
           'S-BKGSD1': ('None', '[e-] sigma (STD) background, first pass')}
    out = dict(header=hdr, objmask=None)
    try:
        om, d_counts = object_mask_enqueue(ctx, work, mini_std, box, nsigma, minarea, grow)
        c, m1, s1 = fetch(ctx, d_counts, mini, mini_std, check_device_errors=True)
        counts = _objmask_counts(c, work.numel())
        hdr['OBJM-NPX'] = (counts['n_listed'],) + hdr['OBJM-NPX'][1:]
        hdr['OBJM-NOB'] = (counts['n_objects'],) + hdr['OBJM-NOB'][1:]
        hdr['OBJM-FRC'] = (counts['frac'],) + hdr['OBJM-FRC'][1:]
        hdr['S-BKG1'] = (float(np.median(m1)),) + hdr['S-BKG1'][1:]
        hdr['S-BKGSD1'] = (float(np.median(s1)),) + hdr['S-BKGSD1'][1:]
        if counts['frac'] > max_frac:
            log.warning('object mask covers %.3f of the frame, more than %.3f: the frame keeps its first background pass', counts['frac'], max_frac)
            return out
        mini2, std2 = get_back(ctx, new, new_mask, om, bkg_boxsize=box)
        out.update(objmask=om, mini=mini2, mini_std=std2, bkg_mini_pass1=m1, bkg_std_mini_pass1=s1)
        hdr['OBJM-P'] = (True,) + hdr['OBJM-P'][1:]
    except Exception as e:
        log.warning('object mask failed (%s): the frame keeps its first background pass', e)
    return out


def _bspline_weights(t):
    return np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6,
                     t ** 3 / 6], -1)


def _axis_map(nin, nout, offset):
    o = np.arange(nout)
    cc = o * ((nin - 1) / (nout - 1)) + NPAD if nout > 1 else np.zeros(1) + NPAD
    fl = np.floor(cc).astype(np.int64)
    return (fl + offset).astype(np.int32), _bspline_weights(cc - fl)


import functools


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
    import math
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


def mini_path_supported(shape, size, border, box, *minis):
    """can bbx_zogy_frame_mini read these mini images for a frame of this geometry (aligned groups of four pixels)?"""
    ny, nx = shape
    if size % 4 or border % 4 or nx % 4 or (size + 2 * border) % 4:
        return False
    for m in minis:
        if m.shape != (ny, nx) or (m.c.cx * m.box) % 4:
            return False
    return True


# ---- ZOGY ---------------------------------------------------------------------------------
def cut_subimages(ctx, img, size=None, border=None):
    size = size or settings.subimage_size
    border = settings.subimage_border if border is None else border
    ny, nx = img.shape
    L = size + 2 * border
    nsub = (ny // size) * (nx // size)
    subs = torch.empty((nsub, L, L), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_cut_subimages(ctx.h, ny, nx, size, border, _p(img), _p(subs), ctx.stream()), 'bbx_cut_subimages', ctx.h)
    return subs


def stitch_subimages(ctx, subs, shape, size=None, border=None):
    size = size or settings.subimage_size
    border = settings.subimage_border if border is None else border
    ny, nx = shape
    img = torch.empty((ny, nx), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_stitch_subimages(ctx.h, ny, nx, size, border, _p(subs), _p(img), ctx.stream()), 'bbx_stitch_subimages', ctx.h)
    return img


def run_zogy(ctx, N, R, Pn, Pr, Vn, Vr, scal):
    """batched run_ZOGY: all inputs [nsub, L, L] float32 device tensors; scal [nsub, 6] =
    (sigma_n, sigma_r, f_n, f_r, dx, dy) -> D, S, Scorr, Fpsf, Fpsferr"""
    nsub, L, _ = N.shape
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    assert scal.shape == (nsub, 6)
    outs = [torch.empty_like(N) for _ in range(5)]
    check(lib.bbx_zogy_subimages(ctx.h, L, nsub, _p(N), _p(R), _p(Pn), _p(Pr), _p(Vn), _p(Vr),
                                 scal.ctypes.data_as(C.POINTER(C.c_float)), *[_p(o) for o in outs], ctx.stream()),
          'bbx_zogy_subimages', ctx.h)
    return outs


def frame_path_supported(L):
    """sub-image sides the hand-written FFT path (bbx_zogy_frame) is built for; BBX_ZOGY_ROCFFT=1
    forces the rocFFT path (bbx_zogy_subimages) everywhere"""
    import os
    return bool(lib.bbx_zogy_frame_supported(int(L))) and not os.environ.get('BBX_ZOGY_ROCFFT')


def zogy_frame_outputs(new, want_S=False):
    """the frames bbx_zogy_frame fills: D, S (or None), Scorr, Fpsf, Fpsferr"""
    return [torch.empty_like(new) if (k != 1 or want_S) else None for k in range(5)]


class RefRows:
    """The reference's half of bbx_zogy_frame's forward transforms (include/bbx.h, bbx_zogy_refrows): the 2-D half spectra
    of the reference frame and of its variance image (row pass, then column pass; the name dates from when the buffer held
    the row transforms only), made once for a reference that stays the same over many frames.  Holds the
    buffer and what it was made of (the reference and its sigma map: a frame or a MiniImage); run_zogy_frame uses it for
    calls with that very reference, sigma map and geometry.  Made on ctx's current stream: a caller that hands the object to
    other streams or contexts waits for that stream first."""
    fills = 0                                    # row passes of a reference made so far (tests: once per run, not per frame)

    def __init__(self, ctx, ref, sig_ref, size, border):
        ny, nx = ref.shape
        nbytes = int(lib.bbx_zogy_refrows_bytes(ny, nx, int(size), int(border)))
        if not nbytes or not ref.is_contiguous() or ref.dtype != torch.float32:
            raise ValueError('no prepared reference rows for this geometry')
        self.ref, self.sig_ref, self.geom = ref, sig_ref, (ny, nx, int(size), int(border))
        self.buf = torch.empty(nbytes // 4, dtype=torch.float32, device=ctx.device)
        if isinstance(sig_ref, MiniImage):
            check(lib.bbx_zogy_refrows_fill_mini(ctx.h, ny, nx, int(size), int(border), _p(ref), sig_ref.ref(), _p(self.buf), ctx.stream()),
                  'bbx_zogy_refrows_fill_mini', ctx.h)
        else:
            check(lib.bbx_zogy_refrows_fill(ctx.h, ny, nx, int(size), int(border), _p(ref), _p(sig_ref), _p(self.buf), ctx.stream()),
                  'bbx_zogy_refrows_fill', ctx.h)
        RefRows.fills += 1

    @staticmethod
    def supported(shape, size, border):
        return bool(lib.bbx_zogy_refrows_bytes(int(shape[0]), int(shape[1]), int(size), int(border)))

    def sigma_id(self):
        return self.sig_ref.coef.data_ptr() if isinstance(self.sig_ref, MiniImage) else self.sig_ref.data_ptr()

    def matches(self, ref, sig_ref, size, border):
        """made of these very tensors, for this geometry?"""
        return (ref is self.ref or (ref.data_ptr() == self.ref.data_ptr() and ref.shape == self.ref.shape)) and sig_ref is self.sig_ref \
            and (ref.shape[0], ref.shape[1], int(size), int(border)) == self.geom


class RefPsf:
    """The reference PSF's half of bbx_zogy_frame's PSF spectra (include/bbx.h, bbx_zogy_refpsf): Pr^ of every sub-image,
    made once for a reference PSF that stays the same over many frames (--psf_ref is loaded once per run; the new frame's
    PSF is per-frame work and stays it).  Holds the buffer and the contiguous stamp tensor [nsub, S, S] it was made of:
    the library knows the stamps by their pointer, so frame calls pass this very tensor (stamps) as the reference's PSFs.
    psf_ref is the caller's object (a stamp tensor or a PSFEx model dict) that matches() recognises.  Made on ctx's
    current stream: a caller that hands the object to other streams or contexts waits for that stream first."""
    fills = 0                                    # reference PSF spectra made so far (tests: once per run, not per frame)

    def __init__(self, ctx, psf_ref, shape, size, border):
        ny, nx = int(shape[0]), int(shape[1])
        nbytes = int(lib.bbx_zogy_refpsf_bytes(ny, nx, int(size), int(border)))
        if not nbytes:
            raise ValueError('no prepared reference PSF spectra for this geometry')
        self.psf_ref, self.geom = psf_ref, (ny, nx, int(size), int(border))
        self.stamps = subimage_psfs(ctx, psf_ref, ny // int(size), nx // int(size), int(size)).contiguous()
        if self.stamps.dtype != torch.float32:
            raise ValueError('float32 PSF stamps expected')
        self.S = int(self.stamps.shape[1])
        self.buf = torch.empty(nbytes // 4, dtype=torch.float32, device=ctx.device)
        check(lib.bbx_zogy_refpsf_fill(ctx.h, ny, nx, int(size), int(border), _p(self.stamps), self.S, _p(self.buf), ctx.stream()),
              'bbx_zogy_refpsf_fill', ctx.h)
        RefPsf.fills += 1

    @staticmethod
    def supported(shape, size, border):
        return bool(lib.bbx_zogy_refpsf_bytes(int(shape[0]), int(shape[1]), int(size), int(border)))

    def matches(self, psf_ref, shape, size, border):
        """made of this very psf_ref object, for this geometry?"""
        return psf_ref is self.psf_ref and (int(shape[0]), int(shape[1]), int(size), int(border)) == self.geom


# ---- flux ratio and dx, dy from matched stars ---------------------------------------------
# buildref.py:2782-3014 (get_fratio, "simplified version of zogy.get_fratio_dxdy") shows the computation; [EXT]
# get_fratio_dxdy, get_matches, get_mean_fratio are not in the reference tree (conventions: include/bbx.h).
MATCH_COLS = ('n_qualifying', 'n_fr', 'med_fr', 'mean_fr', 'std_fr', 'wmean_fr', 'werr_fr', 'n_dx', 'med_dx', 'mean_dx', 'std_dx',
              'n_dy', 'med_dy', 'mean_dy', 'std_dy', 'stride')
_MC = {k: i for i, k in enumerate(MATCH_COLS)}


def window_sigma(stamps):
    """window sigma of the centroid from unit-sum PSF stamps [..., S, S] (device tensor or numpy): sigma_w =
    sqrt(1 / (4 pi sum P^2)), the sigma of the Gaussian with the stamp's effective area.  Stays where the stamps are"""
    if torch.is_tensor(stamps):
        return (1.0 / (4.0 * np.pi * (stamps * stamps).sum(dim=(-2, -1)))).sqrt().to(torch.float32).contiguous()
    stamps = np.asarray(stamps, np.float64)
    return np.sqrt(1.0 / (4.0 * np.pi * (stamps * stamps).sum(axis=(-2, -1))))


def win_centroid(ctx, img, d_ys, d_xs, d_sigw, size, nsy, nsx, radius=None, niter=None):
    """bbx_win_centroid: windowed centroids of the sources at the int32 device peaks (d_ys, d_xs) of the frame [img] ->
    device float32 [n, 2] = (dy, dx) relative to the integer peak, NaN where there is none.  No host wait"""
    radius = settings.centroid_radius if radius is None else radius
    niter = settings.centroid_niter if niter is None else niter
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    n = int(d_ys.numel())
    off = torch.empty((n, 2), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_win_centroid(ctx.h, img.shape[0], img.shape[1], _p(img), n, _p(d_ys), _p(d_xs), _p(d_sigw), int(size), int(nsy), int(nsx),
                               int(radius), int(niter), _p(off), ctx.stream()), 'bbx_win_centroid', ctx.h)
    return off


def match_mutual(ctx, a, b, dist_max):
    """bbx_match_mutual of two lists (d_ys, d_xs, d_off), each sorted by (y, x) -> device int32 [n_a]: index into b, or -1"""
    n_a, n_b = int(a[0].numel()), int(b[0].numel())
    d_match = torch.empty(n_a, dtype=torch.int32, device=ctx.device)
    d_best = torch.empty(n_b, dtype=torch.int32, device=ctx.device)
    check(lib.bbx_match_mutual(ctx.h, n_a, _p(a[0]), _p(a[1]), _p(a[2]), n_b, _p(b[0]), _p(b[1]), _p(b[2]), float(dist_max),
                               _p(d_best), _p(d_match), ctx.stream()), 'bbx_match_mutual', ctx.h)
    return d_match


def empty_match_table(nsub):
    """the table of a frame without a pair: counts 0, stride 1, NaN elsewhere (what bbx_match_stats writes for empty segments)"""
    t = np.full((nsub + 1, 16), np.nan)
    t[:, [_MC['n_qualifying'], _MC['n_fr'], _MC['n_dx'], _MC['n_dy']]] = 0.0
    t[:, _MC['stride']] = 1.0
    return t


def match_stats(ctx, a, b, d_match, size, nsy, nsx, snr_min):
    """bbx_match_stats of the lists a, b = (d_ys, d_xs, d_off, d_flux, d_err) matched by d_match -> device float64
    [nsy * nsx + 1, 16] (MATCH_COLS; last row: the whole frame)"""
    n_a, n_b = int(a[0].numel()), int(b[0].numel())
    if not n_a:
        return torch.from_numpy(empty_match_table(nsy * nsx)).to(ctx.device)
    out = torch.empty((nsy * nsx + 1, 16), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_match_stats(ctx.h, n_a, *[_p(t) for t in a], n_b, *[_p(t) for t in b], _p(d_match), int(size), int(nsy), int(nsx),
                              float(snr_min), _p(out), ctx.stream()), 'bbx_match_stats', ctx.h)
    return out


_MATCH_HDR = (('Z-DX', 'med_dx', '[pix] dx median offset full image'), ('Z-DY', 'med_dy', '[pix] dy median offset full image'),
              ('Z-DXSTD', 'std_dx', '[pix] dx sigma (STD) offset full image'), ('Z-DYSTD', 'std_dy', '[pix] dy sigma (STD) offset full image'),
              ('Z-FNR', 'med_fr', 'median flux ratio (Fnew/Fref) full image'), ('Z-FNRSTD', 'std_fr', 'sigma (STD) flux ratio (Fnew/Fref) full image'),
              ('Z-FNRERR', 'werr_fr', 'weighted error flux ratio (Fnew/Fref) full image'))


def match_scalars(table, fratio, dx, dy, nmin):
    """the table of bbx_match_stats [nsub + 1, 16] (host) -> dict(success, fratio_sub, dx_sub, dy_sub [nsub], header).
    A tile with n_fr >= nmin takes its clipped median ratio; with n_dx >= nmin sqrt(mean_dx^2 + std_dx^2) (the scatter about
    zero that enters V(S)), likewise dy; a tile below nmin takes the full-frame row's value.  A full-frame row with any of the
    three counts below nmin: success False, every tile takes the caller's fratio, dx, dy (one number or one per tile).
    header: Z-DX, Z-DY, Z-DXSTD, Z-DYSTD, Z-FNR, Z-FNRSTD, Z-FNRERR from the full-frame row (set_qc.py:370-375, 425); without
    success the caller's medians for Z-DX, Z-DY, Z-FNR and the string 'None', set_qc's default, for the other four.  Pure numpy"""
    table = np.asarray(table, np.float64)
    nsub = table.shape[0] - 1
    full = table[nsub]
    caller = [np.broadcast_to(np.asarray(v, np.float64), (nsub,)).copy() for v in (fratio, dx, dy)]
    success = bool(full[_MC['n_fr']] >= nmin and full[_MC['n_dx']] >= nmin and full[_MC['n_dy']] >= nmin)
    if not success:
        fall = {'Z-DX': float(np.median(dx)), 'Z-DY': float(np.median(dy)), 'Z-FNR': float(np.median(fratio))}
        hdr = {key: (fall.get(key, 'None'), comment) for key, _, comment in _MATCH_HDR}
        return dict(success=False, fratio_sub=caller[0], dx_sub=caller[1], dy_sub=caller[2], header=hdr)
    hdr = {}

    def scatter(rows, q):
        return np.sqrt(rows[..., _MC['mean_' + q]] ** 2 + rows[..., _MC['std_' + q]] ** 2)
    t = table[:nsub]
    out = [np.where(t[:, _MC['n_fr']] >= nmin, t[:, _MC['med_fr']], full[_MC['med_fr']])]
    for q in ('dx', 'dy'):
        out.append(np.where(t[:, _MC['n_' + q]] >= nmin, scatter(t, q), scatter(full, q)))
    for key, col, comment in _MATCH_HDR:
        hdr[key] = (float(full[_MC[col]]), comment)
    return dict(success=True, fratio_sub=out[0], dx_sub=out[1], dy_sub=out[2], header=hdr)


class RefCatalog:
    """The reference's half of the star match, made once for a reference that stays the same over many frames: the peaks of
    the reference as the subtraction sees it (background-subtracted, on the new frame's grid) above cat_nsigma x the median
    of its sigma mini image, those on masked pixels dropped, with their PSF-weighted fluxes (psf_optflux) and windowed
    centroids (bbx_win_centroid), all on the device in (y, x) order.  Holds what it was made of (the reference and its sigma
    map: a frame or a MiniImage); optimal_subtraction uses it for calls with that very reference, sigma map and geometry.
    Made on ctx's current stream with host waits (once per run): a caller that hands the object to other streams waits for
    that stream first."""
    builds = 0                                   # catalogues made so far (tests: once per run, not per frame)

    def __init__(self, ctx, ref, sig_ref, ref_mask, psf_ref, size, border, cat_nsigma=5.0, sigma_median=None, sub_psfs=None,
                 max_sources=200000, phot_centroid=False):
        if ref.dim() != 2 or ref.dtype != torch.float32 or not ref.is_contiguous():
            raise ValueError('contiguous 2-D float32 reference expected')
        self.phot_centroid = bool(phot_centroid)
        ny, nx = ref.shape
        size, border = int(size), int(border)
        nsy, nsx = ny // size, nx // size
        if sigma_median is None:
            if isinstance(sig_ref, MiniImage):
                raise ValueError('sigma_median (median of the sigma mini image) is needed with a MiniImage')
            sigma_median = float(np.median(fetch(ctx, sig_ref)))
        self.ref, self.sig_ref, self.geom = ref, sig_ref, (ny, nx, size, border)
        sub_pr = sub_psfs if sub_psfs is not None else subimage_psfs(ctx, psf_ref, nsy, nsx, size)
        thr = float(cat_nsigma) * float(sigma_median)
        if np.isfinite(thr) and thr > 0:
            ys, xs, pk = find_peaks_arrays(ctx, ref, thr, max_out=max_sources)
        else:
            ys = xs = np.zeros(0, np.int32); pk = np.zeros(0, np.float32)
        keep = pk > 0
        if ref_mask is not None and ys.size:
            d_ys, d_xs = push(ctx, ys.astype(np.int64), xs.astype(np.int64))
            keep &= fetch(ctx, ref_mask[d_ys, d_xs]) == 0
        ys, xs = ys[keep], xs[keep]
        self.n = int(ys.size)
        dev = ctx.device
        if self.n and self.phot_centroid:
            # the centroids first: the photometry places the PSF on them, as the new frame's does (both sides of a pair alike)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_pr), size, nsy, nsx)
            self.flux, self.err, _ = psf_optflux_centroid(ctx, ref, sig_ref, psf_ref, sub_pr, ys, xs, self.off, ref_mask, nsx, size,
                                                             d_peaks=(self.ys, self.xs))
        elif self.n:
            stamps = source_psfs(ctx, psf_ref, sub_pr, ys, xs, nsx, size)
            self.flux, self.err = psf_optflux(ctx, ref, sig_ref, stamps, ys, xs, v_is_sigma=True)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_pr), size, nsy, nsx)
        else:
            self.ys = self.xs = torch.empty(0, dtype=torch.int32, device=dev)
            self.flux = self.err = torch.empty(0, dtype=torch.float32, device=dev)
            self.off = torch.empty((0, 2), dtype=torch.float32, device=dev)
        RefCatalog.builds += 1

    def lists(self):
        return self.ys, self.xs, self.off, self.flux, self.err

    def matches(self, ref, sig_ref, size, border, phot_centroid=False):
        """made of these very tensors, for this geometry, with its PSFs placed the same way (phot_centroid)?"""
        return (ref is self.ref or (ref.data_ptr() == self.ref.data_ptr() and ref.shape == self.ref.shape)) and sig_ref is self.sig_ref \
            and (ref.shape[0], ref.shape[1], int(size), int(border)) == self.geom and bool(phot_centroid) == self.phot_centroid


def match_enqueue(ctx, work, ys, xs, d_mk, f, e, sub_pn, rc, size, nsy, nsx, dist_max=None, snr_min=None, peaks_off=None):
    """queue the new frame's half of the star match behind its photometry: centroids of the peaks (ys, xs: host, sorted by
    (y, x)) of the background-subtracted frame [work], the mutual match against the RefCatalog [rc] and the table.  Peaks
    on masked pixels (d_mk != 0) are taken out on the device: NaN offset (matches nothing) and flux 0.
    peaks_off: (d_y32, d_x32, off) where the caller has the peaks on the device as int32 and their centroids already (the
    source shapes start from the same ones); they are not changed.
    -> device (table float64 [nsub + 1, 16], number of pairs int64 [1]); no host wait"""
    dist_max = settings.match_dist_pix if dist_max is None else dist_max
    snr_min = settings.match_snr_min if snr_min is None else snr_min
    if peaks_off is not None:
        d_y32, d_x32, off = peaks_off
    else:
        d_y32, d_x32 = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
        off = win_centroid(ctx, work, d_y32, d_x32, window_sigma(sub_pn), size, nsy, nsx)
    bad = d_mk != 0
    off = torch.where(bad[:, None], torch.full_like(off, float('nan')), off).contiguous()
    f_m = torch.where(bad, torch.zeros_like(f), f).contiguous()
    a = (d_y32, d_x32, off, f_m, e)
    d_match = match_mutual(ctx, a[:3], rc.lists()[:3], dist_max)
    d_tab = match_stats(ctx, a, rc.lists(), d_match, size, nsy, nsx, snr_min)
    return d_tab, (d_match >= 0).sum().reshape(1)


# ---- registration of the reference on the new frame from the two star lists (bbx_align.hip) ---------
# [EXT] zogy registers with SWarp and two astrometric solutions; the method and its rules are this project's own, stated in
# float64 numpy by tests/test_align_host.py.  A list is (ys int32, xs int32, off float32 [n, 2], flux float32, err float32) on
# the device; T maps new-frame to reference pixels, coef float64 [12].
ALIGN_PAIR_CAP, ALIGN_NMIN, ALIGN_FAR, ALIGN_CLIP = 8192, 15, 8, 3.0
ALIGN_VOTE_FAILED, ALIGN_FEW_PAIRS, ALIGN_NOT_PD, ALIGN_DET = 1, 2, 4, 8          # the flag word


def _expect_list(lst, name, n_cols=5):
    """a star list crosses the C ABI as bare pointers: every column is checked against the list's length here"""
    from .reduce import _expect
    n = int(lst[0].numel())
    for t, dt, shape, col in zip(lst[:n_cols], (torch.int32, torch.int32, torch.float32, torch.float32, torch.float32),
                                 ((n,), (n,), (n, 2), (n,), (n,)), ('ys', 'xs', 'off', 'flux', 'err')):
        _expect(t, dt, shape, '{} {}'.format(name, col))
    return n


def align_vote(ctx, a, b, nbright=None, max_shift=None, bin=None, nmin=ALIGN_NMIN, far=ALIGN_FAR, cap=ALIGN_PAIR_CAP):
    """bbx_align_vote of the lists a, b = (ys, xs, off, flux[, ...]) -> device (info int32 [8], coarse float64 [2] = (dy, dx),
    pairs int32 [cap, 2]; (-1, -1) past info[4] pairs).  No host wait"""
    nbright = settings.align_nbright if nbright is None else nbright
    max_shift = settings.align_max_shift if max_shift is None else max_shift
    bin = settings.align_bin if bin is None else bin
    n_a, n_b = _expect_list(a, 'list a', 4), _expect_list(b, 'list b', 4)
    nbytes = int(lib.bbx_align_vote_bytes(int(nbright), float(max_shift), float(bin), int(cap)))
    if nbytes == 0:
        raise ValueError('align_vote: nbright {} (1 .. 2048), cap {} (1 .. 8192), max_shift {} or bin {} out of range'.format(nbright, cap, max_shift, bin))
    dev = ctx.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    coarse = torch.empty(2, dtype=torch.float64, device=dev)
    pairs = torch.empty((int(cap), 2), dtype=torch.int32, device=dev)
    check(lib.bbx_align_vote(ctx.h, n_a, *[_p(t) for t in a[:4]], n_b, *[_p(t) for t in b[:4]], int(nbright), float(max_shift), float(bin),
                             int(nmin), int(far), int(cap), _p(work), nbytes, _p(info), _p(coarse), _p(pairs), ctx.stream()),
          'bbx_align_vote', ctx.h)
    return info, coarse, pairs


def align_fit(ctx, a, b, items, shape, poldeg, snr_min=None, clip=ALIGN_CLIP, nmin=ALIGN_NMIN):
    """bbx_align_fit of the pairs items int32 [N, 2] (index into a, into b; -1: none) of the lists a, b (five columns each);
    shape: the new frame's -> device (coef float64 [12], stats float64 [4] = n_used, rms_x, rms_y, flags; kept uint8 [N])"""
    from .reduce import _expect
    snr_min = settings.match_snr_min if snr_min is None else snr_min
    if poldeg not in (1, 2):
        raise ValueError('align_fit: degree 1 or 2, got {}'.format(poldeg))
    n_a, n_b = _expect_list(a, 'list a'), _expect_list(b, 'list b')
    N = int(items.shape[0])
    _expect(items, torch.int32, (N, 2), 'items')
    dev = ctx.device
    coef = torch.empty(12, dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    kept = torch.empty(N, dtype=torch.uint8, device=dev)
    check(lib.bbx_align_fit(ctx.h, n_a, *[_p(t) for t in a[:5]], n_b, *[_p(t) for t in b[:5]], N, _p(items), int(shape[0]), int(shape[1]),
                            int(poldeg), float(snr_min), float(clip), int(nmin), _p(coef), _p(stats), _p(kept), ctx.stream()),
          'bbx_align_fit', ctx.h)
    return coef, stats, kept


def align_apply(ctx, b, coef, shape, poldeg):
    """bbx_align_apply: the list b = (ys, xs, off) through the inverse of T (coef: device float64 [12]; shape: the new frame's)
    -> device (ys int32, xs int32, off float32 [n, 2]), not sorted; a source T^-1 sends beyond 1e9 keeps its integers and gets
    a NaN offset (it matches nothing)"""
    from .reduce import _expect
    if poldeg not in (1, 2):
        raise ValueError('align_apply: degree 1 or 2, got {}'.format(poldeg))
    n = _expect_list(b, 'list b', 3)
    _expect(coef, torch.float64, (12,), 'coef')
    dev = ctx.device
    oys, oxs = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ooff = torch.empty((n, 2), dtype=torch.float32, device=dev)
    check(lib.bbx_align_apply(ctx.h, n, _p(b[0]), _p(b[1]), _p(b[2]), _p(coef), int(shape[0]), int(shape[1]), int(poldeg), _p(oys), _p(oxs),
                              _p(ooff), ctx.stream()), 'bbx_align_apply', ctx.h)
    return oys, oxs, ooff


def align_sort(ys, xs, off):
    """(ys, xs, off) in (y, x) order of the integer peak, as bbx_match_mutual wants it, and the permutation that made it
    (stable: equal peaks keep their list order).  Plumbing: a torch sort of the key y W + x and gathers"""
    if not ys.numel():
        return ys, xs, off, torch.empty(0, dtype=torch.int64, device=ys.device)
    x64, y64 = xs.to(torch.int64), ys.to(torch.int64)
    x0 = x64.min()
    W = x64.max() - x0 + 1
    perm = torch.sort(y64 * W + (x64 - x0), stable=True).indices
    return ys[perm].contiguous(), xs[perm].contiguous(), off[perm].contiguous(), perm


def align_grid_shape(shape, step):
    """nodes of the lattice of a frame: one past the last pixel in both directions (coadd.projection_grid's count)"""
    return -(-(int(shape[0]) + int(step)) // int(step)), -(-(int(shape[1]) + int(step)) // int(step))


def align_grid(ctx, coef, shape, step=32):
    """bbx_align_grid: T at the lattice nodes of the new frame -> device float64 [gny, gnx, 2] = (x, y), what coadd.resample
    and remap_mask take as grid.  No host wait"""
    from .reduce import _expect
    _expect(coef, torch.float64, (12,), 'coef')
    gny, gnx = align_grid_shape(shape, step)
    grid = torch.empty((gny, gnx, 2), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_align_grid(ctx.h, _p(coef), int(shape[0]), int(shape[1]), int(step), gny, gnx, _p(grid), ctx.stream()), 'bbx_align_grid', ctx.h)
    return grid


def align_grid_host(coef, shape, step=32):
    """the same lattice on the host, float64 numpy [gny, gnx, 2]: for remap_mini, which works there"""
    c = np.asarray(coef, np.float64)
    gny, gnx = align_grid_shape(shape, step)
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    v, u = np.meshgrid((np.arange(gny) * float(step) - hy) / hy, (np.arange(gnx) * float(step) - hx) / hx, indexing='ij')
    b = np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], axis=-1)
    return np.ascontiguousarray(np.stack([b @ c[:6], b @ c[6:12]], axis=-1))


def remap_mask(ctx, mask, in_shape, grid, out_shape, step=32, edge=None):
    """bbx_remap_mask: the mask (uint8 [in_shape] or None) of the reference on the new frame's grid through the lattice [grid]
    (device float64 [gny, gnx, 2]) -> device (mask uint8 [out_shape] with the edge bit where the resampler has no footprint,
    number of such pixels int64 [1]).  No host wait"""
    from .reduce import _expect
    edge = settings.mask_value['edge'] if edge is None else edge
    in_ny, in_nx = int(in_shape[0]), int(in_shape[1])
    out_ny, out_nx = int(out_shape[0]), int(out_shape[1])
    if mask is not None:
        _expect(mask, torch.uint8, (in_ny, in_nx), 'mask')
    if not torch.is_tensor(grid) or grid.dim() != 3:
        raise ValueError('remap_mask: the lattice as a device tensor [gny, gnx, 2] expected')
    gny, gnx = int(grid.shape[0]), int(grid.shape[1])
    _expect(grid, torch.float64, (gny, gnx, 2), 'grid')
    out = torch.empty((out_ny, out_nx), dtype=torch.uint8, device=ctx.device)
    nedge = torch.empty(1, dtype=torch.int64, device=ctx.device)
    check(lib.bbx_remap_mask(ctx.h, in_ny, in_nx, _p(mask), out_ny, out_nx, _p(grid), gny, gnx, int(step), int(edge), _p(out), _p(nedge),
                             ctx.stream()), 'bbx_remap_mask', ctx.h)
    return out, nedge


class RefStars:
    """The reference's star list ON ITS OWN GRID, for the registration: the peaks of the background-subtracted reference above
    cat_nsigma x the median of its sigma mini image, those on masked pixels dropped, with windowed centroids and PSF-weighted
    fluxes, in (y, x) order on the device.  The PSF plane of a source is the one of its clamped tile (tile_index) among
    sub_psfs [nsy * nsx, S, S]: only the S/N cut and the brightness ranking rest on it.  sigma: the reference's sigma frame
    on its own grid.  Made once per run (host waits) and used while the reference tensor stays the same"""
    builds = 0

    def __init__(self, ctx, ref, sigma, ref_mask, sub_psfs, nsy, nsx, size, cat_nsigma=5.0, sigma_median=None, max_sources=200000,
                 made_of=None):
        from .reduce import _expect
        rny, rnx = ref.shape
        _expect(ref, torch.float32, (rny, rnx), 'reference')
        _expect(sigma, torch.float32, (rny, rnx), 'reference sigma')
        if ref_mask is not None:
            _expect(ref_mask, torch.uint8, (rny, rnx), 'reference mask')
        nsy, nsx = int(nsy), int(nsx)
        _expect(sub_psfs, torch.float32, (nsy * nsx, sub_psfs.shape[1], sub_psfs.shape[1]), 'PSF stamps')
        # made_of: the tensor the list is kept for, where [ref] is a background-subtracted copy of it made for this call
        self.ref, self.shape = (ref if made_of is None else made_of), (rny, rnx)
        thr = float(cat_nsigma) * float(sigma_median)
        if np.isfinite(thr) and thr > 0:
            ys, xs, pk = find_peaks_arrays(ctx, ref, thr, max_out=max_sources)
        else:
            ys = xs = np.zeros(0, np.int32); pk = np.zeros(0, np.float32)
        keep = pk > 0
        if ref_mask is not None and ys.size:
            d_ys, d_xs = push(ctx, ys.astype(np.int64), xs.astype(np.int64))
            keep &= fetch(ctx, ref_mask[d_ys, d_xs]) == 0
        ys, xs = ys[keep], xs[keep]
        self.n = int(ys.size)
        dev = ctx.device
        if self.n:
            stamps = source_psfs(ctx, None, sub_psfs, ys, xs, nsx, size)
            self.flux, self.err = psf_optflux(ctx, ref, sigma, stamps, ys, xs, v_is_sigma=True)
            self.ys, self.xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
            self.off = win_centroid(ctx, ref, self.ys, self.xs, window_sigma(sub_psfs), size, nsy, nsx)
        else:
            self.ys = self.xs = torch.empty(0, dtype=torch.int32, device=dev)
            self.flux = self.err = torch.empty(0, dtype=torch.float32, device=dev)
            self.off = torch.empty((0, 2), dtype=torch.float32, device=dev)
        RefStars.builds += 1

    def lists(self):
        return self.ys, self.xs, self.off, self.flux, self.err

    def matches(self, ref):
        return ref is self.ref or (ref.data_ptr() == self.ref.data_ptr() and tuple(ref.shape) == self.shape)


def align_header(fit=None, shape=None, poldeg=None, n_edge=None):
    """the A-* keys of _trans_hdr.fits from the host copy of a registration: fit = dict(coef [12], n_used, rms_x, rms_y, flags,
    info [8]); shape: the new frame's.  A-DX, A-DY: new - ref at the frame centre; A-ROT [deg] and A-SCALE from the linear part
    in pixels.  No fit, or a flag word that is not 0: A-P False and the string 'None', set_qc's default, for the rest"""
    keys = (('A-PLDG', 'degree of the registration polynomial'), ('A-NVOTE', 'votes of the winning offset block'),
            ('A-NRUN', 'votes of the runner-up block'), ('A-NFAR', 'votes of the largest far block'),
            ('A-NPAIR', 'star pairs in the last fit'), ('A-RMSX', '[pix] rms of the fit in x'), ('A-RMSY', '[pix] rms of the fit in y'),
            ('A-DX', '[pix] x offset new - ref at the frame centre'), ('A-DY', '[pix] y offset new - ref at the frame centre'),
            ('A-ROT', '[deg] rotation of ref against new'), ('A-SCALE', 'pixel scale new / ref'),
            ('A-FLAGS', 'flags: 1 vote 2 pairs 4 singular 8 det'), ('A-NEDGE', 'pixels without reference coverage'))
    ok = fit is not None and int(fit['flags']) == 0
    hdr = {'A-P': (bool(ok), 'reference registered from its stars?')}
    if not ok:
        for k, c in keys:
            hdr[k] = ('None', c)
        if fit is not None:
            hdr['A-FLAGS'] = (int(fit['flags']), keys[11][1])
        return hdr
    c = np.asarray(fit['coef'], np.float64)
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    # the linear part in pixels: d(x_ref) / d(x_new) ... ; T(centre) = (c[0], c[6])
    a11, a12, a21, a22 = c[1] / hx, c[2] / hy, c[7] / hx, c[8] / hy
    info = np.asarray(fit['info'])
    vals = (int(poldeg), int(info[0]), int(info[1]), int(info[7]), int(fit['n_used']), float(fit['rms_x']), float(fit['rms_y']),
            float(hx - c[0]), float(hy - c[6]), float(np.degrees(np.arctan2(a21 - a12, a11 + a22))),
            float(np.sqrt(abs(a11 * a22 - a12 * a21))), 0, int(n_edge) if n_edge is not None else 'None')
    for (k, cm), v in zip(keys, vals):
        hdr[k] = (v, cm)
    return hdr


def align_reference(ctx, new_lists, ref_stars, shape_new, shape_ref, ref_mask=None, poldeg=None, max_shift=None, bin=None, dist=None,
                    snr_min=None, step=32, rounds=None, nbright=None):
    """The registration of the reference on the new frame: new_lists = the new frame's (ys, xs, off, flux, err), sorted by
    (y, x); ref_stars: a RefStars (or its five columns).  Queued on ctx's stream: the vote, the affine fit of its pairs, [rounds]
    times (the reference's list through the inverse of T, sort, bbx_match_mutual, fit of degree poldeg), the lattice, the
    reference's mask on the new frame's grid; then ONE host wait for coef, stats and info.
    -> dict(grid, mask, coef, header, flags, n_edge, fit); flags != 0: grid and mask are None"""
    poldeg = settings.align_poldeg if poldeg is None else int(poldeg)
    rounds = settings.align_rounds if rounds is None else int(rounds)
    dist = settings.match_dist_pix if dist is None else dist
    if poldeg not in (1, 2):
        raise ValueError('align_reference: degree 1 or 2, got {}'.format(poldeg))
    a = tuple(new_lists)
    b = tuple(ref_stars.lists()) if hasattr(ref_stars, 'lists') else tuple(ref_stars)
    n_a = _expect_list(a, 'new list')
    _expect_list(b, 'reference list')
    info, coarse, pairs = align_vote(ctx, a, b, nbright, max_shift, bin)
    coef, stats, _ = align_fit(ctx, a, b, pairs, shape_new, 1, snr_min)
    ar = torch.arange(n_a, dtype=torch.int32, device=ctx.device)
    for _ in range(rounds):
        sy, sx, so, perm = align_sort(*align_apply(ctx, b[:3], coef, shape_new, poldeg))
        m = match_mutual(ctx, a[:3], (sy, sx, so), dist)
        if perm.numel():
            ib = torch.where(m >= 0, perm[m.clamp(min=0).to(torch.int64)].to(torch.int32), torch.full_like(m, -1))
        else:
            ib = torch.full_like(m, -1)
        items = torch.stack([torch.where(m >= 0, ar, torch.full_like(ar, -1)), ib], dim=1).contiguous()
        coef, stats, _ = align_fit(ctx, a, b, items, shape_new, poldeg, snr_min)
    grid = align_grid(ctx, coef, shape_new, step)
    mask, nedge = remap_mask(ctx, ref_mask, shape_ref, grid, shape_new, step)
    h_coef, h_stats, h_info, h_coarse, h_nedge = fetch(ctx, coef, stats, info, coarse, nedge)
    flags = int(h_stats[3]) | int(h_info[5])
    if not np.isfinite(h_coef).all():
        flags |= int(h_stats[3]) or ALIGN_FEW_PAIRS
    fit = dict(coef=h_coef, n_used=int(h_stats[0]), rms_x=float(h_stats[1]), rms_y=float(h_stats[2]), flags=flags, info=h_info, coarse=h_coarse)
    ok = flags == 0
    n_edge = int(h_nedge[0]) if ok else None
    return dict(grid=grid if ok else None, mask=mask if ok else None, coef=h_coef, flags=flags, n_edge=n_edge, fit=fit,
                header=align_header(fit, shape_new, poldeg, n_edge))


# ---- source shapes of the catalogue and the frame's seeing / elongation statistics ---------
# header keys S-NOBJ S-FWHM S-FWSTD S-SEEING S-SEESTD S-ELONG S-ELOSTD (blackbox.py:3051-3057; ranges set_qc.py:256-266).
# [EXT] zogy takes them from SExtractor; here: adaptive second moments (include/bbx.h), parity unpinned.
SHAPE_COLS = ('c_y', 'c_x', 'Tyy', 'Txx', 'Txy', 'FWHM', 'ELONGATION', 'THETA')
SHAPE_STAT_COLS = ('n_qualifying', 'stride', 'n_fwhm', 'med_fwhm', 'std_fwhm', 'n_elong', 'med_elong', 'std_elong')
_SC = {k: i for i, k in enumerate(SHAPE_STAT_COLS)}


def src_shapes(ctx, img, mask, d_ys, d_xs, d_off, d_sigw, size, nsy, nsx, radius=None, niter=None):
    """bbx_src_shapes: adaptive second moments of the sources at the int32 device peaks (d_ys, d_xs) of the frame [img],
    starting at the centroid offsets d_off [n, 2] (win_centroid) -> device (float32 [n, 8] (SHAPE_COLS), NaN rows where a source
    fails; uint8 [n]: OR of [mask] (or None) over each window).  No host wait"""
    radius = settings.centroid_radius if radius is None else radius
    niter = settings.centroid_niter if niter is None else niter
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(img.shape) or not mask.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')
    n = int(d_ys.numel())
    if d_off.dtype != torch.float32 or tuple(d_off.shape) != (n, 2) or not d_off.is_contiguous():
        raise ValueError('contiguous float32 offsets [n, 2] expected')
    out = torch.empty((n, 8), dtype=torch.float32, device=ctx.device)
    flags = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    check(lib.bbx_src_shapes(ctx.h, img.shape[0], img.shape[1], _p(img), _p(mask) if mask is not None else None, n, _p(d_ys), _p(d_xs),
                             _p(d_off), _p(d_sigw), int(size), int(nsy), int(nsx), int(radius), int(niter), _p(out), _p(flags),
                             ctx.stream()), 'bbx_src_shapes', ctx.h)
    return out, flags


def empty_shape_table(nsub):
    """the table of a frame without a qualifying source: counts 0, stride 1, NaN elsewhere (bbx_shape_stats's empty segments)"""
    t = np.full((nsub + 1, 8), np.nan)
    t[:, [_SC['n_qualifying'], _SC['n_fwhm'], _SC['n_elong']]] = 0.0
    t[:, _SC['stride']] = 1.0
    return t


def shape_stats(ctx, d_ys, d_xs, d_shapes, d_flags, d_flux, d_err, size, nsy, nsx, snr_min=None):
    """bbx_shape_stats of the (y, x)-sorted list -> device float64 [nsy * nsx + 1, 8] (SHAPE_STAT_COLS; last row: the whole
    frame).  No host wait"""
    snr_min = settings.shape_snr_min if snr_min is None else snr_min
    n = int(d_ys.numel())
    if not n:
        return torch.from_numpy(empty_shape_table(nsy * nsx)).to(ctx.device)
    out = torch.empty((nsy * nsx + 1, 8), dtype=torch.float64, device=ctx.device)
    check(lib.bbx_shape_stats(ctx.h, n, _p(d_ys), _p(d_xs), _p(d_shapes), _p(d_flags), _p(d_flux), _p(d_err), int(size), int(nsy), int(nsx),
                              float(snr_min), _p(out), ctx.stream()), 'bbx_shape_stats', ctx.h)
    return out


def shape_columns(ys, xs, shp, flags):
    """the catalogue columns made of the rows of bbx_src_shapes (host, float32 [n, 8]) and its flags: X_POS / Y_POS = peak + 1 +
    offset (the integer peak where the source has no shape), FWHM, ELONGATION, A, B = sqrt of the eigenvalues of T, THETA,
    X2 = Txx, Y2 = Tyy, XY = Txy, FLAGS_MASK"""
    shp = np.asarray(shp, np.float32).reshape(-1, 8)
    F = np.float32
    cy, cx, Tyy, Txx, Txy = (shp[:, k] for k in range(5))
    with np.errstate(invalid='ignore'):
        tr, df = Tyy + Txx, Txx - Tyy
        rad = np.sqrt(df * df + F(4) * (Txy * Txy))
        A, B = np.sqrt((tr + rad) / F(2)), np.sqrt((tr - rad) / F(2))
    return dict(Y_POS=(np.asarray(ys).astype(F) + F(1)) + np.where(np.isnan(cy), F(0), cy),
                X_POS=(np.asarray(xs).astype(F) + F(1)) + np.where(np.isnan(cx), F(0), cx),
                FWHM=shp[:, 5].copy(), ELONGATION=shp[:, 6].copy(), A=A.astype(F), B=B.astype(F), THETA=shp[:, 7].copy(),
                X2=Txx.copy(), Y2=Tyy.copy(), XY=Txy.copy(), FLAGS_MASK=np.asarray(flags, np.uint8).copy())


_SHAPE_HDR = (('S-FWHM', 'med_fwhm', 1, '[pix] median FWHM of the unflagged stars'), ('S-FWSTD', 'std_fwhm', 1, '[pix] sigma (STD) FWHM'),
              ('S-SEEING', 'med_fwhm', 0, '[arcsec] median seeing of the unflagged stars'), ('S-SEESTD', 'std_fwhm', 0, '[arcsec] sigma (STD) seeing'),
              ('S-ELONG', 'med_elong', 1, 'median elongation of the unflagged stars'), ('S-ELOSTD', 'std_elong', 1, 'sigma (STD) elongation'))


def shape_header(table, nobj, nmin, pixscale):
    """the table of bbx_shape_stats [nsub + 1, 8] (host) -> {S-NOBJ, S-FWHM, S-FWSTD, S-SEEING, S-SEESTD, S-ELONG, S-ELOSTD:
    (value, comment)} from the full-frame row; S-SEEING, S-SEESTD = the FWHM values x pixscale.  With fewer than nmin clipped
    values of either quantity in that row the six statistics are the string 'None' (set_qc's default).  Pure numpy"""
    full = np.asarray(table, np.float64)[-1]
    hdr = {'S-NOBJ': (int(nobj), 'number of objects in the catalogue')}
    good = bool(full[_SC['n_fwhm']] >= nmin and full[_SC['n_elong']] >= nmin)
    for key, col, plain, comment in _SHAPE_HDR:
        hdr[key] = ((float(full[_SC[col]]) if plain else float(full[_SC[col]]) * float(pixscale)) if good else 'None', comment)
    return hdr


# ---- PSF model from the frame's own stars ---------------------------------------------------
# `_psf.fits` and the header keys PSF-P PSF-NOBJ PSF-CHI2 PSF-FWHM PSF-SEE PSF-SIZE PSF-CFGS PSF-SAMP PSF-PLDG PSF-FIX
# (blackbox.py:3085-3110, set_qc.py:293-296, 408-409).  [EXT] zogy runs PSFEx; here: the rules of include/bbx.h
# (bbx_psfbuild.hip), parity unpinned.
BBX_ERR_NOTCONV = -5
PSF_REASONS = ('star', 'no shape or flagged', 'peak S/N', 'FWHM or elongation', 'frame edge', 'neighbour')
_PSF_HDR = (('PSF-P', 'successfully processed by the PSF build?'), ('PSF-NOBJ', 'number of stars in the final PSF fit'),
            ('PSF-CHI2', 'mean reduced chi2 of the stars in the final PSF fit'), ('PSF-FWHM', '[pix] median FWHM of the PSF stars'),
            ('PSF-SEE', '[arcsec] PSF-FWHM x pixel scale'), ('PSF-SIZE', '[pix] size of the PSF model image'),
            ('PSF-CFGS', '[pix] size of the PSF vignettes'), ('PSF-SAMP', '[pix] sampling step of the PSF model'),
            ('PSF-PLDG', 'degree of the polynomial in the frame position'), ('PSF-FIX', 'single fixed PSF used for the entire image?'))


def psf_ncoef(poldeg):
    return (poldeg + 1) * (poldeg + 2) // 2


def psf_select(ctx, d_ys, d_xs, d_pk, d_shapes, d_flags, sigma_bkg, fwhm_med, V, ny, nx, cap=None, snr_min=None, fwhm_tol=None,
               elong_max=None, iso_frac=None):
    """bbx_psf_select of the (y, x)-sorted list; fwhm_med: a number, or a one-element float64 device tensor (the frame row of
    bbx_shape_stats, no host wait) -> device (reason uint8 [n], star int32 [cap] (zeros past the kept ones), nstar int32 [2])"""
    S = settings
    cap = int(S.psf_stars_nmax if cap is None else cap)
    n = int(d_ys.numel())
    reason = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    star = torch.zeros(cap, dtype=torch.int32, device=ctx.device)
    nstar = torch.empty(2, dtype=torch.int32, device=ctx.device)
    dev_med = torch.is_tensor(fwhm_med)
    if dev_med and (fwhm_med.dtype != torch.float64 or fwhm_med.numel() != 1):
        raise ValueError('fwhm_med: a number or a one-element float64 device tensor expected')
    check(lib.bbx_psf_select(ctx.h, n, _p(d_ys), _p(d_xs), _p(d_pk), _p(d_shapes), _p(d_flags), float(sigma_bkg),
                             float(S.psf_snr_min if snr_min is None else snr_min), 0.0 if dev_med else float(fwhm_med),
                             _p(fwhm_med) if dev_med else None, float(S.psf_fwhm_tol if fwhm_tol is None else fwhm_tol),
                             float(S.psf_elong_max if elong_max is None else elong_max), float(S.psf_iso_frac if iso_frac is None else iso_frac),
                             int(V), int(ny), int(nx), cap, _p(reason), _p(star), _p(nstar), ctx.stream()), 'bbx_psf_select', ctx.h)
    return reason, star, nstar


def psf_stamps(ctx, img, mask, d_ys, d_xs, d_shapes, d_sig, V, nstar, d_star=None, d_nstar=None, acc=None):
    """bbx_psf_stamps: [nstar] vignettes V x V about the centroids of the sources d_star (None: the first nstar of the list)
    -> device (I float32 [nstar, V, V], w float32 [nstar, V, V], norm float64 [nstar], ok uint8 [nstar])"""
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(img.shape) or not mask.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')
    nstar, V = int(nstar), int(V)
    dev = ctx.device
    I = torch.empty((nstar, V, V), dtype=torch.float32, device=dev)
    w = torch.empty((nstar, V, V), dtype=torch.float32, device=dev)
    norm = torch.empty(nstar, dtype=torch.float64, device=dev)
    ok = torch.empty(nstar, dtype=torch.uint8, device=dev)
    check(lib.bbx_psf_stamps(ctx.h, img.shape[0], img.shape[1], _p(img), _p(mask), int(d_ys.numel()), _p(d_ys), _p(d_xs), _p(d_shapes),
                             _p(d_sig), nstar, _p(d_star), _p(d_nstar), V, float(settings.psf_accuracy if acc is None else acc), _p(I), _p(w),
                             _p(norm), _p(ok), ctx.stream()), 'bbx_psf_stamps', ctx.h)
    return I, w, norm, ok


def psf_fit(ctx, I, w, terms, ok, chi2=None, chi2_med=None, clip=None):
    """bbx_psf_fit over the stars with ok set and, where chi2 [nstar] and chi2_med [1] (device float32) are given, chi2 <=
    clip * chi2_med -> device basis float32 [ncoef, V, V]"""
    nstar, V = int(I.shape[0]), int(I.shape[1])
    ncoef = int(terms.shape[1])
    basis = torch.empty((ncoef, V, V), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_fit(ctx.h, nstar, V, ncoef, _p(I), _p(w), _p(terms), _p(ok), _p(chi2), _p(chi2_med),
                          float(settings.psf_chi2_clip if clip is None else clip), _p(basis), ctx.stream()), 'bbx_psf_fit', ctx.h)
    return basis


def psf_chi2(ctx, I, w, terms, basis, ok):
    """bbx_psf_chi2 -> device float32 [nstar], NaN where ok is 0"""
    nstar, V = int(I.shape[0]), int(I.shape[1])
    chi2 = torch.empty(nstar, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_chi2(ctx.h, nstar, V, int(terms.shape[1]), _p(I), _p(w), _p(terms), _p(basis), _p(ok), _p(chi2), ctx.stream()),
          'bbx_psf_chi2', ctx.h)
    return chi2


def psf_chi2_median(ctx, chi2, ok):
    """np.median of chi2 over the stars with ok set, on the device without knowing their number there: bbx_mini_median of the
    values taken twice, the others replaced once by the lowest and once by the highest float32 -- the middle pair of that
    sample is the middle (pair) of the ok values.  No ok star: 0.  -> device float32 [1]"""
    good = ok != 0
    big = torch.finfo(torch.float32).max
    both = torch.cat([torch.where(good, chi2, torch.full_like(chi2, -big)), torch.where(good, chi2, torch.full_like(chi2, big))]).contiguous()
    med = torch.empty(1, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_mini_median(ctx.h, both.numel(), _p(both), _p(med), ctx.stream()), 'bbx_mini_median', ctx.h)
    return med


def psf_header(ok, nobj=None, chi2=None, fwhm=None, V=None, poldeg=None, pixscale=None):
    """{PSF-P, PSF-NOBJ, PSF-CHI2, PSF-FWHM, PSF-SEE, PSF-SIZE, PSF-CFGS, PSF-SAMP, PSF-PLDG, PSF-FIX: (value, comment)}; a build that
    failed: PSF-P False and the string 'None', set_qc's default, for the rest.  Pure Python"""
    pixscale = settings.pixscale if pixscale is None else pixscale
    if ok:
        vals = (True, int(nobj), float(chi2), float(fwhm), float(fwhm) * float(pixscale), int(V), int(V), 1.0, int(poldeg), False)
    else:
        vals = (False,) + ('None',) * 9
    return {k: (v, c) for (k, c), v in zip(_PSF_HDR, vals)}


def _source_sigma(ctx, sigma, shape, ys, xs):
    """the background sigma at the integer peaks (host arrays): a number, a frame, a mini image (a small 2-D tensor or array: the
    value of the box the peak falls in) or a MiniImage (its frame is made) -> device float32 [n]"""
    ny, nx = shape
    n = len(ys)
    if isinstance(sigma, MiniImage):
        sigma = sigma.frame(ctx)
    if np.isscalar(sigma):
        return torch.full((n,), float(sigma), dtype=torch.float32, device=ctx.device)
    if not torch.is_tensor(sigma):
        sigma = push(ctx, np.ascontiguousarray(sigma, np.float32))
    if sigma.dim() != 2:
        raise ValueError('sigma: a number, a frame, a mini image or a MiniImage expected')
    if tuple(sigma.shape) == (ny, nx):
        iy, ix = ys, xs
    else:
        by, bx = -(-ny // sigma.shape[0]), -(-nx // sigma.shape[1])
        iy, ix = np.minimum(np.asarray(ys) // by, sigma.shape[0] - 1), np.minimum(np.asarray(xs) // bx, sigma.shape[1] - 1)
    d_iy, d_ix = push(ctx, np.asarray(iy, np.int64), np.asarray(ix, np.int64)) if n else (torch.empty(0, dtype=torch.int64, device=ctx.device),) * 2
    return sigma[d_iy, d_ix].to(torch.float32).contiguous()


def build_psf(ctx, data_bkgsub, sigma, mask, size, nsy, nsx, cat_nsigma=5.0, sigma_median=None, peaks=None, psf_size=None,
              poldeg=None, max_sources=200000):
    """A PSFEx-style model of the frame's PSF from its own stars (include/bbx.h, bbx_psfbuild.hip):
      peaks of the background-subtracted frame above cat_nsigma x sigma_median (peaks = (ys, xs, pk), host arrays sorted by
      (y, x), where the caller has searched already) -> windowed centroids and adaptive moments from the seed window
      settings.psf_seed_fwhm / 2.3548 -> the frame's median FWHM (bbx_shape_stats, flux = peak, err = sigma) -> bbx_psf_select
      -> bbx_psf_stamps -> bbx_psf_fit over all stars, then settings.psf_nclip rounds of {bbx_psf_chi2, median, fit of the stars
      within settings.psf_chi2_clip x the median} and a last bbx_psf_chi2.
    sigma: the background sigma: a number, a frame, a mini image or a MiniImage (_source_sigma); sigma_median: its median
    (S-BKGSTD; needed unless sigma is a number).  The polynomial terms are those of the integer peak in FITS pixels, where
    source_psfs evaluates the model.  Every degree up to poldeg (settings.psf_poldeg) that the list could support is fitted, and
    the degree taken is the largest with 5 coefficients' worth of stars with a vignette; fewer than settings.psf_nstars_min
    stars in its final fit: no model.  ONE host wait (two when a fit raised the device's soft-fault word), besides the search.
    -> dict(model: dict(basis device float32 [ncoef, V, V], polzero, polscal, poldeg, psf_samp, psf_fwhm) as fitsio.read_psfex
            gives it, or None; header: psf_header; stars: dict(n_sources, n_qualifying, stride, reason [n_sources], index, ys,
            xs [m], ok, used [m], chi2 [m], norm [m]))"""
    S = settings
    V = int(psf_size or S.psf_size)
    poldeg = int(S.psf_poldeg if poldeg is None else poldeg)
    if V < 1 or V > 49 or not V % 2 or not 0 <= poldeg <= 3:
        raise ValueError('psf_size odd and at most 49, psf_poldeg 0..3 expected')
    if data_bkgsub.dim() != 2 or data_bkgsub.dtype != torch.float32 or not data_bkgsub.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    ny, nx = data_bkgsub.shape
    if sigma_median is None:
        if not np.isscalar(sigma):
            raise ValueError('sigma_median (median of the sigma image) is needed unless sigma is a number')
        sigma_median = float(sigma)
    sigma_median = float(sigma_median)
    fail = dict(model=None, header=psf_header(False), stars=dict(n_sources=0, n_qualifying=0, stride=1))
    if peaks is None:
        thr = float(cat_nsigma) * sigma_median
        if not (np.isfinite(thr) and thr > 0):
            return fail
        peaks = find_peaks_arrays(ctx, data_bkgsub, thr, max_out=max_sources)
    ys, xs, pk = (np.asarray(a) for a in peaks)
    keep = pk > 0
    ys, xs, pk = ys[keep].astype(np.int32), xs[keep].astype(np.int32), pk[keep].astype(np.float32)
    n = int(ys.size)
    fail['stars']['n_sources'] = n
    if not n or not (np.isfinite(sigma_median) and sigma_median > 0):
        return fail
    nsub = nsy * nsx
    dev = ctx.device
    d_y32, d_x32, d_pk = push(ctx, ys, xs, pk)
    d_sig = _source_sigma(ctx, sigma, (ny, nx), ys, xs)
    sigw = torch.full((nsub,), float(S.psf_seed_fwhm) / 2.3548, dtype=torch.float32, device=dev)
    off = win_centroid(ctx, data_bkgsub, d_y32, d_x32, sigw, size, nsy, nsx)
    d_shp, d_sfl = src_shapes(ctx, data_bkgsub, mask, d_y32, d_x32, off, sigw, size, nsy, nsx)
    d_stab = shape_stats(ctx, d_y32, d_x32, d_shp, d_sfl, d_pk, d_sig, size, nsy, nsx, S.psf_snr_min)
    d_fmed = d_stab[nsub, _SC['med_fwhm']:_SC['med_fwhm'] + 1]         # (a view: one float64 of the frame row)
    cap = max(1, min(int(S.psf_stars_nmax), n))
    d_reason, d_star, d_nstar = psf_select(ctx, d_y32, d_x32, d_pk, d_shp, d_sfl, sigma_median, d_fmed, V, ny, nx, cap=cap)
    I, w, d_norm, d_ok = psf_stamps(ctx, data_bkgsub, mask, d_y32, d_x32, d_shp, d_sig, V, cap, d_star=d_star, d_nstar=d_nstar)
    polzero, polscal = ((nx + 1) / 2.0, (ny + 1) / 2.0), (nx / 2.0, ny / 2.0)
    degs = [d for d in range(poldeg + 1) if 5 * psf_ncoef(d) <= cap] or [0]
    idx = d_star.to(torch.int64)
    fits, back = [], [d_nstar, d_star, d_ok, d_norm, d_reason, d_fmed]
    for d in degs:
        terms = push(ctx, psf_poly_terms(xs + 1.0, ys + 1.0, polzero, polscal, d)).index_select(0, idx).contiguous()
        basis = psf_fit(ctx, I, w, terms, d_ok)
        used = d_ok != 0
        for _ in range(int(S.psf_nclip)):
            chi2 = psf_chi2(ctx, I, w, terms, basis, d_ok)
            med = psf_chi2_median(ctx, chi2, d_ok)
            basis = psf_fit(ctx, I, w, terms, d_ok, chi2, med, S.psf_chi2_clip)
            used = (d_ok != 0) & (chi2 <= float(S.psf_chi2_clip) * med)
        chi2 = psf_chi2(ctx, I, w, terms, basis, d_ok)
        nfit = used.sum().reshape(1)
        csum = torch.where(used, chi2, torch.zeros_like(chi2)).to(torch.float64).sum().reshape(1)
        fits.append(basis)
        back += [used.to(torch.uint8), chi2, nfit, csum]
    try:
        got = fetch(ctx, *back, check_device_errors=True)
    except _lib_BBXError as e:
        if e.code != BBX_ERR_NOTCONV:
            raise
        # a fit met a pixel without a positive definite matrix (a degree with too few stars): the numbers decide below
        got = fetch(ctx, *back)
    (nq, stride), star, ok, norm, reason, fmed = got[:6]
    m = min(-(-int(nq) // max(int(stride), 1)), cap)
    star, ok, norm = star[:m], ok[:m], norm[:m]
    n_ok = int((ok != 0).sum())
    k = max([j for j, d in enumerate(degs) if n_ok >= 5 * psf_ncoef(d)] or [0])
    used, chi2, nfit, csum = got[6 + 4 * k:10 + 4 * k]
    nfit, fwhm = int(nfit[0]), float(fmed[0])
    stars = dict(n_sources=n, n_qualifying=int(nq), stride=int(stride), reason=reason, index=star, ys=ys[star], xs=xs[star], ok=ok,
                 used=used[:m] != 0, chi2=chi2[:m], norm=norm)
    chi2_mean = float(csum[0]) / nfit if nfit else float('nan')
    if nfit < int(S.psf_nstars_min) or not np.isfinite(fwhm) or not np.isfinite(chi2_mean):
        import logging
        logging.getLogger(__name__).warning('PSF build: %d stars in the final fit (%d sources, %d selected), fewer than the minimum or no '
                                            'finite statistics: no model', nfit, n, int(nq))
        return dict(model=None, header=psf_header(False), stars=stars)
    model = dict(basis=fits[k], polzero=polzero, polscal=polscal, poldeg=degs[k], psf_samp=1.0, psf_fwhm=fwhm)
    return dict(model=model, header=psf_header(True, nfit, chi2_mean, fwhm, V, degs[k]), stars=stars)


def run_zogy_frame(ctx, new, ref, sig_new, sig_ref, psf_n, psf_r, scal, size, border, want_S=False, outs=None, ref_rows=None, ref_psf=None):
    """ZOGY of whole frames (bbx_zogy_frame): background-subtracted frames + sigma images + PSF
    stamps [nsub, S, S] -> D, S (or None), Scorr, Fpsf, Fpsferr full frames.  sig_new, sig_ref: frames, or both
    MiniImage (bbx_zogy_frame_mini: the sigma maps are read off their mini images, no frames exist).
    ref_rows: a RefRows made of (ref, sig_ref): the call skips the reference's row and column pass (the library refuses rows of
    another reference, sigma map or geometry)
    ref_psf: a RefPsf whose stamps tensor is psf_r: the call transforms the new stamps only (needs ref_rows; the library refuses
    spectra of another stamp tensor, stamp size or geometry)"""
    if ref_psf is not None:
        ny, nx = new.shape
        check(lib.bbx_zogy_refpsf(ctx.h, _p(ref_psf.buf), ny, nx, int(size), int(border), _p(ref_psf.stamps), ref_psf.S), 'bbx_zogy_refpsf', ctx.h)
        try:
            return run_zogy_frame(ctx, new, ref, sig_new, sig_ref, psf_n, psf_r, scal, size, border, want_S=want_S, outs=outs, ref_rows=ref_rows)
        finally:
            lib.bbx_zogy_refpsf(ctx.h, None, 0, 0, 0, 0, None, 0)         # the setting never outlives the call it was made for
    if ref_rows is not None:
        ny, nx = new.shape
        check(lib.bbx_zogy_refrows(ctx.h, _p(ref_rows.buf), ny, nx, int(size), int(border), _p(ref), C.c_void_p(ref_rows.sigma_id())),
              'bbx_zogy_refrows', ctx.h)
        try:
            return run_zogy_frame(ctx, new, ref, sig_new, sig_ref, psf_n, psf_r, scal, size, border, want_S=want_S, outs=outs)
        finally:
            lib.bbx_zogy_refrows(ctx.h, None, 0, 0, 0, 0, None, None)     # the setting never outlives the call it was made for
    ny, nx = new.shape
    nsub = (ny // size) * (nx // size)
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    assert scal.shape == (nsub, 6) and psf_n.shape[0] == nsub and psf_r.shape[0] == nsub
    S = int(psf_n.shape[1])
    outs = outs or zogy_frame_outputs(new, want_S)
    if isinstance(sig_new, MiniImage):
        check(lib.bbx_zogy_frame_mini(ctx.h, ny, nx, int(size), int(border), _p(new), _p(ref), sig_new.ref(), sig_ref.ref(),
                                      _p(psf_n.contiguous()), _p(psf_r.contiguous()), S, scal.ctypes.data_as(C.POINTER(C.c_float)),
                                      *[_p(o) for o in outs], ctx.stream()), 'bbx_zogy_frame_mini', ctx.h)
        return outs
    check(lib.bbx_zogy_frame(ctx.h, ny, nx, int(size), int(border), _p(new), _p(ref), _p(sig_new), _p(sig_ref),
                             _p(psf_n.contiguous()), _p(psf_r.contiguous()), S, scal.ctypes.data_as(C.POINTER(C.c_float)),
                             *[_p(o) for o in outs], ctx.stream()), 'bbx_zogy_frame', ctx.h)
    return outs


def psf_optflux(ctx, D, V, psfs, ys, xs, v_is_sigma=False):
    """zogy.get_psfoptflux at integer positions -> (flux, fluxerr) float32 device tensors; with v_is_sigma
    V is the sigma image of the background-subtracted frame D -- a frame, or a MiniImage read at the stamp pixels --
    and the variance max(D, 0) + sigma^2 is formed at the stamp pixels only"""
    nsrc, S, _ = psfs.shape
    dev = ctx.device
    d_ys, d_xs = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
    flux = torch.empty(nsrc, dtype=torch.float32, device=dev)
    err = torch.empty(nsrc, dtype=torch.float32, device=dev)
    ny, nx = D.shape
    if isinstance(V, MiniImage):
        check(lib.bbx_psf_optflux_mini(ctx.h, ny, nx, _p(D), V.ref(), _p(psfs), S, nsrc, _p(d_ys), _p(d_xs), _p(flux), _p(err), ctx.stream()),
              'bbx_psf_optflux_mini', ctx.h)
        return flux, err
    fn = lib.bbx_psf_optflux_sigma if v_is_sigma else lib.bbx_psf_optflux
    check(fn(ctx.h, ny, nx, _p(D), _p(V), _p(psfs), S, nsrc, _p(d_ys), _p(d_xs), _p(flux), _p(err), ctx.stream()), 'bbx_psf_optflux', ctx.h)
    return flux, err


PD_FOLD_WARN = 0.01             # a T-PDFOLD above this is logged: P_D does not fit its stamp (Moffat pairs fold 1e-4 at most, a point / box pair 0.15)
TRANS_AT_BOUND, TRANS_MASKED, TRANS_NO_FIT, TRANS_NOT_CONVERGED = 1, 2, 4, 8       # FLAGS_PSF_D bits (include/bbx.h, bbx_trans_psffit)


def pd_stamps(ctx, sub_pn, sub_pr, scal, M=None):
    """bbx_zogy_pd_stamps: the PSF of the difference image of every sub-image from its two PSF stamps [nsub, S, S] (device float32,
    unit sum) and scal [nsub, 6] = (sn, sr, fn, fr, dx, dy) (host), on a grid of M x M (settings.trans_pd_grid)
    -> device (pd float32 [nsub, S, S], fold float32 [nsub]: the share of sum |p| on the grid that the stamp leaves out).  No host wait"""
    M = int(settings.trans_pd_grid if M is None else M)
    if sub_pn.dim() != 3 or sub_pn.dtype != torch.float32 or sub_pr.dtype != torch.float32 or tuple(sub_pn.shape) != tuple(sub_pr.shape) or \
            sub_pn.shape[1] != sub_pn.shape[2]:
        raise ValueError('two float32 stamp tensors [nsub, S, S] of one shape expected')
    nsub, S = int(sub_pn.shape[0]), int(sub_pn.shape[1])
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    if scal.shape != (nsub, 6):
        raise ValueError('scal [nsub, 6] expected')
    sub_pn, sub_pr = sub_pn.contiguous(), sub_pr.contiguous()
    pd = torch.empty((nsub, S, S), dtype=torch.float32, device=ctx.device)
    fold = torch.empty(nsub, dtype=torch.float32, device=ctx.device)
    check(lib.bbx_zogy_pd_stamps(ctx.h, nsub, S, M, _p(sub_pn), _p(sub_pr), scal.ctypes.data_as(C.POINTER(C.c_float)), _p(pd), _p(fold),
                                 ctx.stream()), 'bbx_zogy_pd_stamps', ctx.h)
    return pd, fold


def trans_psffit(ctx, D, N, R, sig_n, sig_r, mask, pd, ys, xs, scal, size, nsx, fit_size=None, niter=None, maxshift=None, d_peaks=None):
    """bbx_trans_psffit: the PSF of D (pd [nsub, S, S], pd_stamps) fitted to D with free position in a window of fit_size x fit_size
    pixels around every candidate's integer peak (ys, xs: host arrays; d_peaks: the same as int32 device tensors where the caller
    has them).  N, R: the background-subtracted new and reference frames; sig_n, sig_r: their sigma maps, two frames or two
    MiniImage; mask: uint8 frame or None, its pixels are left out; scal [nsub, 6] (host); fit_size, niter, maxshift: settings.trans_fit_*
    -> device (flux, err, dy, dx, chi2 float32 [n], flags uint8 [n]: TRANS_AT_BOUND | TRANS_MASKED | TRANS_NO_FIT |
    TRANS_NOT_CONVERGED).  No host wait"""
    ny, nx = D.shape
    for f in (D, N, R):
        if f.dim() != 2 or f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (ny, nx):
            raise ValueError('contiguous 2-D float32 frames of one shape expected')
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (ny, nx) or not mask.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')
    mini = isinstance(sig_n, MiniImage)
    if mini != isinstance(sig_r, MiniImage):
        raise ValueError('the two sigma maps must be of one form: two frames or two MiniImage')
    if not mini:
        for f in (sig_n, sig_r):
            if f.dtype != torch.float32 or tuple(f.shape) != (ny, nx) or not f.is_contiguous():
                raise ValueError('sigma: contiguous float32 frames of the image shape or MiniImage expected')
    if pd.dim() != 3 or pd.dtype != torch.float32 or pd.shape[1] != pd.shape[2] or not pd.is_contiguous():
        raise ValueError('contiguous float32 stamps [nsub, S, S] expected')
    nsub, S = int(pd.shape[0]), int(pd.shape[1])
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    if scal.shape != (nsub, 6):
        raise ValueError('scal [nsub, 6] expected')
    ys, xs = np.asarray(ys), np.asarray(xs)
    n = int(ys.size)
    if d_peaks is not None:
        d_ys, d_xs = d_peaks
        if d_ys.dtype != torch.int32 or d_xs.dtype != torch.int32 or d_ys.numel() != n or d_xs.numel() != n:
            raise ValueError('d_peaks: the int32 device copies of ys, xs expected')
    else:
        d_ys, d_xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
    dev = ctx.device
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(5)] + [torch.empty(n, dtype=torch.uint8, device=dev)]
    W = int(settings.trans_fit_size if fit_size is None else fit_size)
    check(lib.bbx_trans_psffit(ctx.h, ny, nx, _p(D), _p(N), _p(R), None if mini else _p(sig_n), None if mini else _p(sig_r),
                               sig_n.ref() if mini else None, sig_r.ref() if mini else None, _p(mask) if mask is not None else None, S, nsub,
                               _p(pd), int(size), int(nsx), scal.ctypes.data_as(C.POINTER(C.c_float)), n, _p(d_ys), _p(d_xs), W,
                               int(settings.trans_fit_niter if niter is None else niter),
                               float(settings.trans_fit_maxshift if maxshift is None else maxshift), *[_p(o) for o in outs], ctx.stream()),
          'bbx_trans_psffit', ctx.h)
    return tuple(outs)


_trans_psffit = trans_psffit                                         # (_optimal_subtraction's switch bears the name)


def trans_fit_header(on, fit_size=None, rows=None, fold=None):
    """the keys of `_trans_hdr.fits` for the fit of P_D to D: T-PSFD, and with it T-FITSZ, T-NFIT (rows with flags & 12 == 0),
    T-PDFOLD (the largest fold over the sub-images), T-CHI2MD (the median chi2 of those rows; 'None' without any)"""
    h = {'T-PSFD': (bool(on), 'PSF of D fitted to the transient candidates?')}
    if on:
        good = [r['chi2_psf_d'] for r in rows if not r['flags_psf_d'] & (TRANS_NO_FIT | TRANS_NOT_CONVERGED)]
        h['T-FITSZ'] = (int(fit_size), '[pix] side of the window of the fit of P_D to D')
        h['T-NFIT'] = (len(good), 'number of candidates with a converged fit')
        h['T-PDFOLD'] = (float(np.max(fold)) if len(fold) else 'None', 'largest share of |P_D| outside its stamp')
        h['T-CHI2MD'] = (float(np.median(good)) if good else 'None', 'median CHI2_PSF_D of the converged fits')
    return h


TRANS_SHAPE_REFUSED = 16                                             # FLAGS_GAUSS_D / FLAGS_MOFFAT_D: bits 1 2 4 8 as above, and this (bbx_trans_shapefit)
SHAPE_GAUSS, SHAPE_MOFFAT = 1, 2                                     # `models` of bbx_trans_shapefit
SHAPE_OUT = ('y', 'x', 'yerr', 'xerr', 'fwhm', 'elong', 'chi2')      # the planes of its output


def trans_shapefit(ctx, D, N, R, sig_n, sig_r, mask, fwhm0, ys, xs, scal, size, nsx, fit_size=None, niter=None, maxshift=None, models=3,
                   beta=None, fwhm_lo=None, fwhm_hi=None, d_peaks=None):
    """bbx_trans_shapefit: an elliptical Gaussian and an elliptical Moffat (beta fixed) fitted to D in the window of trans_psffit
    (fit_size x fit_size pixels around every candidate's integer peak, the same used pixels and V_D) by Levenberg-Marquardt.  The
    arguments are trans_psffit's, but for fwhm0 (device float32 [nsub]: the FWHM the fits start with in every sub-image) in the
    place of the P_D stamps; fit_size, niter, maxshift, beta, fwhm_lo, fwhm_hi: settings.trans_shape_* / trans_moffat_beta (fwhm_hi
    None: twice the window's side); models: SHAPE_GAUSS | SHAPE_MOFFAT
    -> device (out float32 [2, 7, n]: per model (Gauss, Moffat) the planes SHAPE_OUT, y and x relative to the integer peak;
    flags uint8 [2, n]: TRANS_AT_BOUND | TRANS_MASKED | TRANS_NO_FIT | TRANS_NOT_CONVERGED | TRANS_SHAPE_REFUSED).  No host wait"""
    ny, nx = D.shape
    for f in (D, N, R):
        if f.dim() != 2 or f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (ny, nx):
            raise ValueError('contiguous 2-D float32 frames of one shape expected')
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (ny, nx) or not mask.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')
    mini = isinstance(sig_n, MiniImage)
    if mini != isinstance(sig_r, MiniImage):
        raise ValueError('the two sigma maps must be of one form: two frames or two MiniImage')
    if not mini:
        for f in (sig_n, sig_r):
            if f.dtype != torch.float32 or tuple(f.shape) != (ny, nx) or not f.is_contiguous():
                raise ValueError('sigma: contiguous float32 frames of the image shape or MiniImage expected')
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    if scal.ndim != 2 or scal.shape[1] != 6:
        raise ValueError('scal [nsub, 6] expected')
    nsub = int(scal.shape[0])
    if not torch.is_tensor(fwhm0) or fwhm0.dtype != torch.float32 or tuple(fwhm0.shape) != (nsub,) or not fwhm0.is_contiguous():
        raise ValueError('fwhm0: a contiguous float32 device tensor [nsub] expected')
    ys, xs = np.asarray(ys), np.asarray(xs)
    n = int(ys.size)
    if d_peaks is not None:
        d_ys, d_xs = d_peaks
        if d_ys.dtype != torch.int32 or d_xs.dtype != torch.int32 or d_ys.numel() != n or d_xs.numel() != n:
            raise ValueError('d_peaks: the int32 device copies of ys, xs expected')
    else:
        d_ys, d_xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
    dev = ctx.device
    out = torch.zeros((2, len(SHAPE_OUT), n), dtype=torch.float32, device=dev)
    flags = torch.full((2, n), TRANS_NO_FIT, dtype=torch.uint8, device=dev)        # (what a call with models == 0 leaves)
    W = int(settings.trans_shape_size if fit_size is None else fit_size)
    hi = settings.trans_shape_fwhm_hi if fwhm_hi is None else fwhm_hi
    check(lib.bbx_trans_shapefit(ctx.h, ny, nx, _p(D), _p(N), _p(R), None if mini else _p(sig_n), None if mini else _p(sig_r),
                                 sig_n.ref() if mini else None, sig_r.ref() if mini else None, _p(mask) if mask is not None else None, nsub,
                                 int(size), int(nsx), scal.ctypes.data_as(C.POINTER(C.c_float)), _p(fwhm0), n, _p(d_ys), _p(d_xs), W,
                                 int(settings.trans_shape_niter if niter is None else niter),
                                 float(settings.trans_shape_maxshift if maxshift is None else maxshift), int(models),
                                 float(settings.trans_moffat_beta if beta is None else beta),
                                 float(settings.trans_shape_fwhm_lo if fwhm_lo is None else fwhm_lo), float(2 * W if hi is None else hi),
                                 _p(out), _p(flags), ctx.stream()), 'bbx_trans_shapefit', ctx.h)
    return out, flags


_trans_shapefit = trans_shapefit                                     # (_optimal_subtraction's switch bears the name)


def shape_start_fwhm(sub_pn, sub_pr):
    """the FWHM the shape fits start with, per sub-image: 2.3548 x the larger window_sigma of the two PSF stamps; device float32
    [nsub], no fetch"""
    return (2.3548 * torch.maximum(window_sigma(sub_pn), window_sigma(sub_pr))).to(torch.float32).contiguous()


def trans_shape_header(on, fit_size=None, beta=None, rows=None):
    """the keys of `_trans_hdr.fits` for the Gauss and Moffat fits to D: T-SHAPE, and with it T-SHPSZ, T-MBETA, T-NGAUS, T-NMOFF (rows
    with flags & 12 == 0), T-FWGMD, T-ELGMD (the medians over the converged Gauss rows; 'None' without any)"""
    h = {'T-SHAPE': (bool(on), 'Gauss and Moffat fitted to the transient candidates?')}
    if on:
        bad = TRANS_NO_FIT | TRANS_NOT_CONVERGED
        good = [r for r in rows if not r['flags_gauss_d'] & bad]
        h['T-SHPSZ'] = (int(fit_size), '[pix] side of the window of the Gauss and Moffat fits')
        h['T-MBETA'] = (float(beta), 'beta of the Moffat fit (fixed)')
        h['T-NGAUS'] = (len(good), 'number of candidates with a converged Gauss fit')
        h['T-NMOFF'] = (sum(1 for r in rows if not r['flags_moffat_d'] & bad), 'number of candidates with a converged Moffat fit')
        h['T-FWGMD'] = (float(np.median([r['fwhm_gauss_d'] for r in good])) if good else 'None', '[pix] median FWHM_GAUSS_D of the converged fits')
        h['T-ELGMD'] = (float(np.median([r['elong_gauss_d'] for r in good])) if good else 'None', 'median ELONG_GAUSS_D of the converged fits')
    return h


def vet_transients(rows, chi2_max=None, fwhm_gauss_min=None, fwhm_gauss_max=None, elong_gauss_max=None):
    """the rows that pass the vetting -> (kept rows, their indices).  chi2_max (--trans_chi2_max): those with a fit of P_D (no
    TRANS_NO_FIT) and chi2_psf_d <= chi2_max.  With any of the Gauss bounds (--trans_fwhm_gauss_min / _max, --trans_elong_gauss_max):
    those with a Gauss fit (no TRANS_NO_FIT) inside every bound given"""
    keep = list(range(len(rows)))
    if chi2_max is not None:
        keep = [i for i in keep if not rows[i]['flags_psf_d'] & TRANS_NO_FIT and rows[i]['chi2_psf_d'] <= chi2_max]
    if fwhm_gauss_min is not None or fwhm_gauss_max is not None or elong_gauss_max is not None:
        keep = [i for i in keep if not rows[i]['flags_gauss_d'] & TRANS_NO_FIT
                and (fwhm_gauss_min is None or rows[i]['fwhm_gauss_d'] >= fwhm_gauss_min)
                and (fwhm_gauss_max is None or rows[i]['fwhm_gauss_d'] <= fwhm_gauss_max)
                and (elong_gauss_max is None or rows[i]['elong_gauss_d'] <= elong_gauss_max)]
    return [rows[i] for i in keep], keep


PHOT_NO_CENTROID, PHOT_MASKED, PHOT_NO_SUM = 1, 2, 4                # FLAGS_OPT bits (include/bbx.h, bbx_psf_optflux_shift)


def psf_optflux_centroid(ctx, D, sigma, psf, sub_psfs, ys, xs, d_off, mask, nsx, size, d_peaks=None):
    """bbx_psf_optflux_shift: the photometry of psf_optflux(source_psfs(...)) with every source's PSF shifted to its centroid
    d_off [n, 2] (win_centroid: relative to the integer peak; device float32) inside the kernel -- no stamp is written.
    psf: a PSFEx model dict (its terms at the integer peaks, as source_psfs) or anything else, and then sub_psfs [nsub, S, S],
    of which each source takes the plane of its sub-image; sigma: the sigma frame of D or a MiniImage; mask: uint8 frame or
    None, its pixels are left out of the sums; ys, xs: host arrays; d_peaks: (d_ys, d_xs), the same as int32 device tensors
    where the caller has them.
    -> device (flux float32 [n], err float32 [n], flags uint8 [n]: PHOT_NO_CENTROID | PHOT_MASKED | PHOT_NO_SUM).  No host wait"""
    if D.dim() != 2 or D.dtype != torch.float32 or not D.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    ny, nx = D.shape
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (ny, nx) or not mask.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')
    dev = ctx.device
    ys, xs = np.asarray(ys), np.asarray(xs)
    if d_peaks is not None:
        d_ys, d_xs = d_peaks
        if d_ys.dtype != torch.int32 or d_xs.dtype != torch.int32 or d_ys.numel() != ys.size or d_xs.numel() != xs.size:
            raise ValueError('d_peaks: the int32 device copies of ys, xs expected')
    else:
        d_ys, d_xs = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
    n = int(ys.size)
    if d_off.dtype != torch.float32 or tuple(d_off.shape) != (n, 2) or not d_off.is_contiguous():
        raise ValueError('contiguous float32 offsets [n, 2] expected')
    terms = idx = None
    if isinstance(psf, dict):
        cube = psf['basis'].contiguous()
        terms = torch.from_numpy(psf_poly_terms(np.asarray(xs) + 1.0, np.asarray(ys) + 1.0, psf['polzero'], psf['polscal'], psf['poldeg'])).to(dev)
        if terms.shape[1] != cube.shape[0]:
            raise ValueError('basis has %d planes, polynomial degree %d needs %d' % (cube.shape[0], psf['poldeg'], terms.shape[1]))
    else:
        cube = sub_psfs.contiguous()
        idx = tile_index(d_ys, d_xs, size, int(cube.shape[0]) // int(nsx), nsx).to(torch.int32)
    if cube.dim() != 3 or cube.dtype != torch.float32 or cube.shape[1] != cube.shape[2]:
        raise ValueError('float32 PSF planes [n, S, S] expected')
    if not isinstance(sigma, MiniImage) and (sigma.dtype != torch.float32 or tuple(sigma.shape) != (ny, nx) or not sigma.is_contiguous()):
        raise ValueError('sigma: a contiguous float32 frame of the image shape or a MiniImage expected')
    flux = torch.empty(n, dtype=torch.float32, device=dev)
    err = torch.empty(n, dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    mini = isinstance(sigma, MiniImage)
    check(lib.bbx_psf_optflux_shift(ctx.h, ny, nx, _p(D), None if mini else _p(sigma), sigma.ref() if mini else None,
                                    _p(mask) if mask is not None else None, int(cube.shape[1]), int(cube.shape[0]), _p(cube), _p(terms), _p(idx),
                                    n, _p(d_ys), _p(d_xs), _p(d_off), _p(flux), _p(err), _p(flags), ctx.stream()), 'bbx_psf_optflux_shift', ctx.h)
    return flux, err, flags


def psf_poly_terms(x, y, polzero, polscal, poldeg):
    """PSFEx polynomial terms of the source positions (pixel coordinates x, y; one
    polynomial group over (x, y)): x' = (x - polzero[0]) / polscal[0], same for y; order
    1, x', x'^2, .., y', x'y', .., y'^2, .. (y power outer, x power inner), float32.
    -> array [nsrc, (poldeg+1)(poldeg+2)/2]"""
    xn = ((np.asarray(x, np.float64) - polzero[0]) / polscal[0]).astype(np.float32)
    yn = ((np.asarray(y, np.float64) - polzero[1]) / polscal[1]).astype(np.float32)
    cols = []
    for j in range(poldeg + 1):
        for i in range(poldeg + 1 - j):
            cols.append((xn ** np.float32(i)) * (yn ** np.float32(j)) if (i or j) else np.ones_like(xn))
    return np.stack(cols, axis=1).astype(np.float32)


def resample_psf_basis(basis, psf_samp):
    """PSFEx tabulates its model every PSF_SAMP image pixels (automatic sampling: usually != 1).  zogy.get_psf_ima
    (buildref.py:3357-3366 passes psf_samp) resamples the model image to image pixels: psf_size =
    ceil(S_config * psf_samp) made odd, scipy.ndimage.zoom by psf_size / S_config [EXT: order 2, mode 'nearest';
    oracle/zogy_core.get_psf_ima].  The resampling is linear, so it is applied once to every basis plane (host,
    ncoef small images) and the per-source contraction (bbx_psf_model) then works on image pixels.
    -> float32 [ncoef, psf_size, psf_size]"""
    basis = np.asarray(basis, np.float64)
    s_cfg = basis.shape[1]
    size = int(np.ceil(s_cfg * float(psf_samp)))
    size += 1 - size % 2
    if size == s_cfg:
        return basis.astype(np.float32)
    out = np.stack([ndimage.zoom(b, size / s_cfg, order=2, mode='nearest') for b in basis])
    if out.shape[1:] != (size, size):
        raise ValueError('PSF resampling gave {} instead of {}'.format(out.shape[1:], (size, size)))
    return out.astype(np.float32)


def psf_model_stamps(ctx, basis, x, y, polzero, polscal, poldeg, normalize=True):
    """PSF stamp of every source from a PSFEx model: basis [ncoef, S, S] float32 device
    tensor (PSF_MASK), positions x, y (host arrays).  The contraction runs on the f32 MFMA
    (bbx_psf_model).  -> device tensor [nsrc, S, S]; normalize: each stamp sums to one"""
    terms = torch.from_numpy(psf_poly_terms(x, y, polzero, polscal, poldeg)).to(ctx.device)
    ncoef, S = basis.shape[0], basis.shape[1]
    if terms.shape[1] != ncoef:
        raise ValueError('basis has %d planes, polynomial degree %d needs %d' % (ncoef, poldeg, terms.shape[1]))
    nsrc = terms.shape[0]
    out = torch.empty((nsrc, S, S), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_psf_model(ctx.h, nsrc, ncoef, S * S, _p(terms), _p(basis.contiguous()), _p(out), ctx.stream()),
          'bbx_psf_model', ctx.h)
    if normalize:
        out /= out.sum(dim=(1, 2), keepdim=True)
    return out


def find_transients(ctx, Scorr, nsigma=None, max_out=100000):
    """connected regions of |Scorr| >= T-NSIGMA -> sorted list of (y, x, Scorr peak)"""
    ys, xs, val = find_peaks_arrays(ctx, Scorr, nsigma, max_out)
    return list(zip(ys.tolist(), xs.tolist(), val.tolist()))


def find_peaks_enqueue(ctx, Scorr, nsigma=None, max_out=100000):
    """queue bbx_find_peaks -> the device tensors find_peaks_collect reads (host work in between overlaps the search)"""
    nsigma = settings.transient_nsigma if nsigma is None else nsigma
    ny, nx = Scorr.shape
    dev = ctx.device
    yx = torch.empty((max_out, 2), dtype=torch.int32, device=dev)
    val = torch.empty(max_out, dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.bbx_find_peaks(ctx.h, ny, nx, _p(Scorr), float(nsigma), max_out, _p(yx), _p(val), _p(cnt), ctx.stream()),
          'bbx_find_peaks', ctx.h)
    return yx, val, cnt, max_out


def find_peaks_collect(ctx, pending):
    """-> arrays (y int32, x int32, peak float32), sorted by (y, x)"""
    yx, val, cnt, max_out = pending
    if max_out * 12 <= (2 << 20):
        # the count and the whole list (1.2 MB at the default capacity) in ONE copy back and one host wait: asking for the
        # count first costs a second round trip -- with the stream's other work in front of it each time
        c, yx, val = fetch(ctx, cnt, yx, val, check_device_errors=True)
        n = min(int(c[0]), max_out)
        yx, val = yx[:n], val[:n]
    else:
        n = min(int(fetch(ctx, cnt, check_device_errors=True)[0]), max_out)
        yx, val = fetch(ctx, yx[:n], val[:n])
    order = np.lexsort((yx[:, 1], yx[:, 0])) if n else np.zeros(0, int)
    return yx[order, 0], yx[order, 1], val[order]


def find_peaks_arrays(ctx, Scorr, nsigma=None, max_out=100000):
    """the same as arrays (y int32, x int32, peak float32), sorted by (y, x): no per-source Python work"""
    return find_peaks_collect(ctx, find_peaks_enqueue(ctx, Scorr, nsigma, max_out))


def embed_psfs(ctx, stamps, L):
    """PSF stamps [nsub, S, S] (unit sum, centre at S//2) -> [nsub, L, L] centred on pixel [0,0]"""
    nsub, S, _ = stamps.shape
    out = torch.empty((nsub, L, L), dtype=torch.float32, device=ctx.device)
    check(lib.bbx_embed_psf(ctx.h, nsub, S, L, _p(stamps), _p(out), ctx.stream()), 'bbx_embed_psf', ctx.h)
    return out


def variance(ctx, data_bkgsub, bkg_std):
    v = torch.empty_like(data_bkgsub)
    check(lib.bbx_variance(ctx.h, data_bkgsub.numel(), _p(data_bkgsub), _p(bkg_std), _p(v), ctx.stream()), 'bbx_variance', ctx.h)
    return v


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


def subimage_psfs(ctx, psf, nsy, nsx, size):
    """PSF stamps of the sub-images [nsub, S, S] (unit sum) from either such a tensor, a single
    stamp [S, S], or a PSFEx model dict(basis=[ncoef,S,S] device tensor, polzero, polscal, poldeg)
    evaluated at the sub-image centres on the f32 MFMA (zogy.get_psf_ima at the tile centre)"""
    nsub = nsy * nsx
    if isinstance(psf, dict):
        yc = (np.arange(nsy) + 0.5) * size + 0.5          # FITS pixel coordinates of the tile centres
        xc = (np.arange(nsx) + 0.5) * size + 0.5
        yy, xx = np.meshgrid(yc, xc, indexing='ij')
        return psf_model_stamps(ctx, psf['basis'], xx.ravel(), yy.ravel(), psf['polzero'], psf['polscal'], psf['poldeg'])
    if psf.dim() == 2:
        return psf.unsqueeze(0).expand(nsub, -1, -1).contiguous()
    if psf.shape[0] != nsub:
        raise ValueError('need one PSF stamp per sub-image ({}), got {}'.format(nsub, psf.shape[0]))
    return psf.contiguous()


def tile_index(ys, xs, size, nsy, nsx):
    """index of the sub-image tile (size x size pixels, nsy x nsx tiles) of the integer peaks (ys, xs): numpy arrays or
    tensors.  Clamped as the kernels clamp it (bbx_match.hip, k_win_centroid): min(max(y // size, 0), nsy - 1), likewise x -- a
    peak of a frame that is no multiple of the tile (a reference on its own grid) takes the last tile, not one past the end
    of the stamps.  For a frame of nsy size x nsx size pixels nothing changes"""
    size, nsy, nsx = int(size), int(nsy), int(nsx)
    if nsy < 1 or nsx < 1 or size < 1:
        raise ValueError('tile_index: size, nsy, nsx must be positive, got {} {} {}'.format(size, nsy, nsx))
    if torch.is_tensor(ys):
        return torch.clamp(ys // size, 0, nsy - 1) * nsx + torch.clamp(xs // size, 0, nsx - 1)
    return np.clip(np.asarray(ys) // size, 0, nsy - 1) * nsx + np.clip(np.asarray(xs) // size, 0, nsx - 1)


def source_psfs(ctx, psf, sub_psfs, ys, xs, nsx, size):
    """unit-sum PSF stamp of every source: the PSFEx model at the source position, or the stamp
    of the sub-image the source falls in"""
    if isinstance(psf, dict):
        return psf_model_stamps(ctx, psf['basis'], np.asarray(xs) + 1.0, np.asarray(ys) + 1.0, psf['polzero'],
                                psf['polscal'], psf['poldeg'])
    k = push(ctx, tile_index(np.asarray(ys), np.asarray(xs), size, int(sub_psfs.shape[0]) // int(nsx), nsx).astype(np.int64))
    return sub_psfs.index_select(0, k).contiguous()


def frame_clipped_stats_enqueue(ctx, img, mask=None, step=8):
    """queue bbx_frame_clipped_stats of a contiguous float32 frame -> device tensor [8] (n, median, mean, sigma, ...)"""
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    if mask is not None and (mask.dtype != torch.uint8 or mask.shape != img.shape or not mask.is_contiguous()):
        raise ValueError('mask: contiguous uint8 of the frame shape expected')
    ny, nx = img.shape
    out = torch.empty(8, dtype=torch.float64, device=img.device)
    check(lib.bbx_frame_clipped_stats(ctx.h, ny, nx, _p(img), _p(mask), int(step), 3.0, 5, 1,
                                      _p(out), ctx.stream()), 'bbx_frame_clipped_stats', ctx.h)
    return out


def frame_clipped_stats(ctx, img, mask=None, step=8):
    """sigma_clipped_stats (3 sigma, 5 iterations, centre = exact median, mask_value 0) of a frame -> (median,
    std) as zogy reports them in Z-SCMED / Z-SCSTD / Z-FPEMED / Z-FPESTD.  zogy takes these header
    statistics from a random subset of the pixels; here the subset is the regular lattice of
    every [step]-th pixel in both axes (deterministic; 1.7 10^6 samples of a 10560^2 frame)."""
    st = fetch(ctx, frame_clipped_stats_enqueue(ctx, img, mask, step))
    return float(st[1]), float(st[3])


class StreamGate:
    """Lets one stream at a time run a section on the GPU: a section starts when the previous one (of any
    stream) has finished.  bbx_zogy_frame's kernels each fill the whole GPU; two lanes running them side
    by side only slice each other's time.  With priority=True the sections run on ONE high-priority stream of the
    gate's own (in order: that is the gate), between a wait for the caller's stream and a wait of the caller's stream:
    the short kernels of the other lanes then take the CUs a section leaves free instead of an equal share of all of
    them.  Tensors a section is to fill must be allocated before it (they belong to the caller's stream)."""

    def __init__(self, device=None, priority=False):
        import threading
        self.lock = threading.Lock()
        self.last = None
        self.hp = torch.cuda.Stream(device=device, priority=-1) if priority else None
        self._cm = self._cur = None

    def __enter__(self):
        self.lock.acquire()
        cur = torch.cuda.current_stream()
        if self.hp is not None:
            self.hp.wait_stream(cur)
            self._cur, self._cm = cur, torch.cuda.stream(self.hp)
            self._cm.__enter__()
        elif self.last is not None:
            cur.wait_event(self.last)
        return self

    def __exit__(self, *exc):
        if self.hp is not None:
            self._cm.__exit__(*exc)
            self._cur.wait_stream(self.hp)
            self._cm = self._cur = None
        else:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.last = ev
        self.lock.release()
        return False


class _NoGate:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def optimal_subtraction(ctx, *args, **kw):
    try:
        return _optimal_subtraction(ctx, *args, **kw)
    finally:
        # the candidate-list handoffs (zoom -> catalogue search, final ZOGY kernel -> transient search) are keyed on the
        # frames' addresses inside the context: whatever way this call ends, none of that may outlive it (the caching
        # allocator hands the same address to the next frame)
        lib.bbx_zoom_candidates(ctx.h, None, 0.0)
        lib.bbx_zogy_candidates(ctx.h, 0.0)


def _optimal_subtraction(ctx, new, ref, new_mask, ref_mask, psf_new, psf_ref, fratio=1.0, dx=0.0, dy=0.0,
                         subimage_size=None, subimage_border=None, bkg_boxsize=None, nsigma=None,
                         ref_is_bkgsub=False, ref_bkg_std_mini=None, ref_grid=None, ref_grid_step=32,
                         cat_extract=False, cat_nsigma=5.0, trans_extract=True, frame_stats=True, max_sources=200000,
                         zogy_gate=None, ref_bkg_std=None, sigma_frames=False, thumbnails=False, thumbnail_size=None,
                         thumbnail_pngs=False, ref_rows=None, ref_psf=None, match=False, ref_catalog=None, match_dist=None, match_nmin=None,
                         match_snr_min=None, shapes=False, shape_snr_min=None, psf_build=False, psf_size=None, psf_poldeg=None,
                         phot_centroid=False, objmask=False, objmask_nsigma=None, objmask_minarea=None, objmask_grow=None,
                         objmask_max_frac=None, trans_psffit=False, trans_fit_size=None, trans_chi2_max=None,
                         trans_shapefit=False, trans_shape_size=None, trans_fwhm_gauss_min=None, trans_fwhm_gauss_max=None,
                         trans_elong_gauss_max=None, ref_align=False, align_poldeg=None, align_max_shift=None, align_bin=None,
                         align_nbright=None, align_rounds=None, ref_stars=None):
    """The numerical core of zogy.optimal_subtraction(new_fits, ref_fits, ...) (call sites
    blackbox.py:2350-2354 new-only, 2460-2465 new + ref) on device tensors: background mesh +
    subtraction, variance images, [remapping of the reference to the new frame's grid],
    sub-image ZOGY, stitching, transient candidates with PSF fluxes, [full-source catalogue by
    PSF-weighted optimal photometry].
      new, new_mask : reduced frame (float32, e-) and its mask
      fratio, dx, dy: flux ratio new / ref and the astrometric scatter, one number or one per sub-image
      ref, ref_mask : reference frame or None (new-only mode, trans_extract False or no ref:
                      the 2350-2354 branch): then only the background products and the catalogue
      ref_is_bkgsub : the reference is a background-subtracted co-add (buildref product);
                      ref_bkg_std_mini: its `_bkg_std_mini` image (else measured here);
                      ref_bkg_std: what an earlier call made from it (res['bkg_std_ref']: a MiniImage, or the
                      full-frame sigma image), when the caller keeps it for many frames of the same field
      ref_rows      : a RefRows made of the reference and of ref_bkg_std by the caller that keeps both for many frames: the
                      subtraction skips the reference's row transforms (used only where it was made of this call's very
                      reference, sigma map and geometry; same result bit for bit)
      ref_psf       : a RefPsf made of this call's very psf_ref object by the caller that keeps it for many frames: its stamp
                      tensor serves as the reference's PSFs and, where ref_rows is used, the subtraction skips the
                      reference PSF's transforms (same result bit for bit)
      sigma_frames  : True: the two sigma images are made as full frames (rounds 1-4; bbx_zogy_frame) instead of
                      being read off their mini images inside the kernels (bbx_zogy_frame_mini)
      ref_grid      : projection lattice (coadd.projection_grid) when the reference lives on
                      another pixel grid: it is remapped with the LANCZOS3 kernel (zogy runs SWarp)
      psf_new/ref   : PSF stamps [nsub, S, S] / [S, S] (unit sum) or a PSFEx model dict
                      (subimage_psfs) -- running PSFEx itself is out of scope
      thumbnails    : True: res['thumbnails'], device float32 [n, 4, S, S]: the cut-outs RED / REF / D / SCORR of every
                      transient candidate (qc.py:480-485), S = thumbnail_size (settings.size_thumbnails)
      thumbnail_pngs: True: res['thumbnail_png8'], device uint8 [n, 4, S, S]: their display planes (blackbox.py:2786-2826)
                      either switch adds 'flags' (FLAGS_MASK: the masks under the peak) to each transient; both off: no
                      kernel of bbx_thumb.hip is launched and the result has none of these keys
      match         : True (with a reference and both PSFs): fratio, dx, dy of every sub-image are measured from the stars matched
                      between the new frame and the reference (bbx_win_centroid, bbx_match_mutual, bbx_match_stats; match_scalars)
                      and go into the subtraction in place of the caller's, which stay the fallback where the frame has fewer
                      than match_nmin pairs; res['match'] = dict(success, n_new, n_ref, n_pairs, table, fratio_sub, dx_sub,
                      dy_sub), res['ref_catalog'], and header_trans gets Z-DXSTD, Z-DYSTD, Z-FNRSTD, Z-FNRERR.  False: no kernel
                      of bbx_match.hip is launched, no such keys.  match_dist [pix], match_nmin, match_snr_min: settings
      shapes        : True (with cat_extract and psf_new): every catalogue source gets its adaptive second moments (bbx_src_shapes,
                      started at the windowed centroids, which the star match shares when it is on too) and the frame its
                      clipped FWHM / elongation statistics (bbx_shape_stats), both riding the photometry's copy back:
                      res['catalog'] gains FWHM, ELONGATION, A, B, THETA, X2, Y2, XY, FLAGS_MASK and sub-pixel X_POS / Y_POS,
                      res['shapes'] = dict(table, n_good), header_new gets S-NOBJ, S-FWHM, S-FWSTD, S-SEEING, S-SEESTD,
                      S-ELONG, S-ELOSTD (shape_header).  False: no kernel of bbx_shapes.hip is launched, no such keys or columns.
                      shape_snr_min: settings
      psf_build     : True with psf_new None: the new frame's PSF model is built from its own stars (build_psf) between the
                      catalogue's peak search and the photometry and used as psf_new from there on (catalogue, shapes, star
                      match, sub-image PSFs, subtraction); res['psf'] = dict(model, header, stars), header_new gets PSF-P,
                      PSF-NOBJ, PSF-CHI2, PSF-FWHM, PSF-SEE, PSF-SIZE, PSF-CFGS, PSF-SAMP, PSF-PLDG, PSF-FIX.  A build that fails
                      (PSF-P False): the frame goes on as one without a PSF (background products only).  With psf_new given, or
                      False: no kernel of bbx_psfbuild.hip is launched, no such keys.  psf_size, psf_poldeg: settings
      phot_centroid : True: the catalogue photometry (cat_extract, and the star match's two lists) places every source's PSF on
                      its windowed centroid instead of its integer peak (bbx_psf_optflux_shift in place of source_psfs +
                      psf_optflux; the centroids are taken first and shared with shapes and match) and leaves the masked pixels
                      of new_mask out of the sums: res['catalog'] gains FLAGS_OPT (PHOT_NO_CENTROID | PHOT_MASKED | PHOT_NO_SUM)
                      and sub-pixel X_POS / Y_POS (peak + 1 + offset; the integer peak where there is no centroid), header_new
                      gets PHOT-CEN.  False: no kernel of bbx_psfphot.hip is launched, no such key or column
      objmask       : True: the new frame's background mesh is measured twice: the first pass's background-subtracted frame
                      gives the object mask (object_mask; objmask_nsigma, objmask_minarea, objmask_grow: settings), the second pass
                      leaves the masked pixels out, and everything from there on (S-BKG, S-BKGSTD, the sigma image, the catalogue,
                      the PSF build, the match, the subtraction) rests on the second pass.  res['objmask'] (device uint8),
                      res['bkg_mini_pass1'], res['bkg_std_mini_pass1']; header_new gets OBJM-P, OBJM-THR, OBJM-MIN, OBJM-GRW,
                      OBJM-NPX, OBJM-NOB, OBJM-FRC, S-BKG1, S-BKGSD1.  One more host wait.  A pixel list that overflows, an
                      exception in the stage or a mask over more than objmask_max_frac (settings) of the frame: the frame goes
                      on with its first pass, OBJM-P False, no res['objmask'].  False: no kernel of bbx_objmask.hip is
                      launched, no such keys
      ref_catalog   : a RefCatalog made of the reference and of ref_bkg_std by the caller that keeps both for many frames (used
                      only where it was made of this call's very reference, sigma map and geometry; same result bit for bit)
      trans_psffit  : True (with candidates and PSF stamps of one side): the PSF of D of every sub-image (pd_stamps) is fitted to D at
                      every candidate with free position (bbx_trans_psffit; trans_fit_size: settings), queued behind the peak
                      search with the Fpsf gather and read in the same copy back: every transient gains x_psf_d, y_psf_d (0-based,
                      peak + offset), flux_psf_d, fluxerr_psf_d, chi2_psf_d, flags_psf_d; header_trans gets T-PSFD, T-FITSZ, T-NFIT,
                      T-PDFOLD, T-CHI2MD (trans_fit_header).  trans_chi2_max: rows without a fit or with a chi2 above it are
                      dropped, with their thumbnails; T-NVET = the rows kept, T-NTRANS stays.  An exception in the stage:
                      today's table, T-PSFD False.  False: no kernel of bbx_transfit.hip is launched, no such keys
      trans_shapefit: True (same conditions, with or without trans_psffit): an elliptical Gaussian and an elliptical Moffat are fitted
                      to D at every candidate (bbx_trans_shapefit; trans_shape_size: settings), queued behind the fit of P_D or
                      the peak search and read in the same copy back: every transient gains x_, xerr_, y_, yerr_, fwhm_, elong_,
                      chi2_, flags_gauss_d and the same eight of _moffat_d; header_trans gets T-SHAPE, T-SHPSZ, T-MBETA, T-NGAUS,
                      T-NMOFF, T-FWGMD, T-ELGMD (trans_shape_header).  trans_fwhm_gauss_min / _max, trans_elong_gauss_max: rows
                      without a Gauss fit or outside a bound are dropped, with their thumbnails (T-NVET).  An exception in the
                      stage: today's table, T-SHAPE False.  False: bbx_trans_shapefit is not launched, no such keys
      ref_align     : True (with a reference of any shape and both PSFs; a caller's ref_grid with it is a ValueError): the reference
                      is registered on the new frame from the stars of both (align_reference): the new frame's
                      photometry and centroids first, then the reference's list on its own grid (RefStars: ref_stars where the
                      caller keeps one of this very reference, else made here and returned as res['ref_stars']), the transform, its
                      lattice -- which takes the place of ref_grid -- and the reference's mask on the new frame's grid, which
                      takes the place of ref_mask (res['ref_mask_remapped']).  One more host wait.  Transient candidates whose peak
                      has no reference under it (the mask's edge bit) are dropped with their thumbnails: T-NOFFR; T-NTRANS stays.
                      res['align'] = align_reference's dict; header_trans gets A-P, A-PLDG, A-NVOTE, A-NRUN, A-NFAR, A-NPAIR, A-RMSX,
                      A-RMSY, A-DX, A-DY, A-ROT, A-SCALE, A-FLAGS, A-NEDGE.  A registration that fails (flag word not 0, or an exception
                      in the stage): the frame goes on as one without a reference, A-P False -- it is never subtracted unregistered.
                      align_poldeg, align_max_shift, align_bin, align_nbright, align_rounds: settings.  False: no kernel of
                      bbx_align.hip is launched, no such keys
    -> dict(D, Scorr, Fpsf, Fpsferr, bkg_mini_new, bkg_std_mini_new, ..., transients, catalog,
            header (= header_new additions), header_trans)"""
    size = subimage_size or settings.subimage_size
    border = settings.subimage_border if subimage_border is None else subimage_border
    box = bkg_boxsize or settings.bkg_boxsize
    ny, nx = new.shape
    L = size + 2 * border
    res, hdr, hdr_t = {}, {}, {}
    nsy, nsx = ny // size, nx // size
    nsub = nsy * nsx
    have_ref = ref is not None and trans_extract
    build_here = bool(psf_build) and psf_new is None                 # the PSF of the new frame is made below, behind the peak search
    have_psf = psf_new is not None or build_here
    do_match = bool(match) and have_ref and have_psf and psf_ref is not None
    do_shapes = bool(shapes) and bool(cat_extract) and have_psf
    phot_centroid = bool(phot_centroid)
    do_align = bool(ref_align) and have_ref
    if do_align and ref_grid is not None:
        raise ValueError('ref_align=True makes the lattice itself: a ref_grid beside it is refused')
    ref_mask_remapped = ref_grid_host = None                        # set by a registration that succeeded

    # ---- new frame: mesh, subtraction, sigma image, variance
    mini, mini_std = get_back(ctx, new, new_mask, bkg_boxsize=box)
    work = torch.empty_like(new)
    want_phot = cat_extract or do_match or do_align
    want_cat =(want_phot or (build_here and have_ref)) and have_psf
    second_pass = False
    if objmask:
        # the first pass's frame (no candidate list: it is not the frame the catalogue is searched on), the object mask made of
        # it, and -- when the mask is usable -- the mesh once more without the masked pixels
        mini2back(ctx, mini, (ny, nx), bkg_boxsize=box, interp_Xchan=True, subtract_from=new, subtract_into=work)
        om = _objmask_stage(ctx, new, new_mask, work, mini, mini_std, box, objmask_nsigma, objmask_minarea, objmask_grow, objmask_max_frac)
        hdr.update(om['header'])
        if om['objmask'] is not None:
            second_pass = True
            mini, mini_std = om['mini'], om['mini_std']
            res['objmask'], res['bkg_mini_pass1'], res['bkg_std_mini_pass1'] = om['objmask'], om['bkg_mini_pass1'], om['bkg_std_mini_pass1']
    if want_cat and (second_pass or not objmask):
        # the kernel that writes the background-subtracted frame lists the pixels above cat_nsigma x S-BKGSTD for the
        # catalogue's peak search; S-BKGSTD = median of the sigma mini image, taken on the device for that
        # (a frame that fell back to its first pass has that frame already: bbx_find_peaks makes its own pass)
        d_sstd = torch.empty(1, dtype=torch.float32, device=ctx.device)
        check(lib.bbx_mini_median(ctx.h, mini_std.numel(), _p(mini_std), _p(d_sstd), ctx.stream()), 'bbx_mini_median', ctx.h)
        check(lib.bbx_zoom_candidates(ctx.h, _p(d_sstd), float(cat_nsigma)), 'bbx_zoom_candidates', ctx.h)
    if second_pass or not objmask:
        mini2back(ctx, mini, (ny, nx), bkg_boxsize=box, interp_Xchan=True, subtract_from=new, subtract_into=work)
    # the sigma image of the new frame: read off its mini image by the kernels that need it (catalogue photometry, the cut
    # into sub-images) where the geometry allows, a frame otherwise
    import os
    use_mini = frame_path_supported(L) and not sigma_frames and not os.environ.get('BBX_SIGMA_FRAMES')     # (the switch: A/B timing)
    bstd = None
    if use_mini:
        try:
            bstd = MiniImage(ctx, mini_std, box, interp_Xchan=False)
            use_mini = mini_path_supported((ny, nx), size, border, box, bstd)
        except ValueError:
            use_mini = False
    if not use_mini:
        bstd = mini2back(ctx, mini_std, (ny, nx), bkg_boxsize=box, interp_Xchan=False)
    Vn = None                                                        # variance image: only where a consumer needs it
    res['bkg_mini_new'], sdn = fetch(ctx, mini, mini_std)
    res['bkg_std_mini_new'] = sdn
    hdr['BKG-SIZE'] = (box, '[pix] background boxsize used')
    hdr['BKG-SUB'] = (False, 'sky background was subtracted?')          # the _red product keeps its sky
    # zogy's per-channel background correction factors (BKG-CF1..16, BKG-FDEG, BKG-FC0: blackbox.py:3061-3066, all None_OK)
    # are [EXT] without a source in the reference tree: not applied here, and the header says so
    hdr['BKG-CORR'] = (False, 'channel background correction applied?')
    hdr['S-BKGSTD'] = (float(np.median(sdn)), '[e-] sigma (STD) background full-frame image')
    res['data_bkgsub'], res['bkg_std'] = work, bstd
    bs = size // box if size % box == 0 else None

    def tile_medians(a):
        """median of the mini image over the boxes of each sub-image (or over all of it)"""
        if bs and a.shape == (nsy * bs, nsx * bs):
            return np.median(a.reshape(nsy, bs, nsx, bs).transpose(0, 2, 1, 3).reshape(nsub, bs * bs), axis=1)
        if bs:
            return np.asarray([np.median(a[(k // nsx) * bs:(k // nsx + 1) * bs, (k % nsx) * bs:(k % nsx + 1) * bs]) for k in range(nsub)])
        return np.full(nsub, np.median(a))
    scal_n = None

    def host_side_meanwhile():
        """host work that needs nothing from the device: done while a search runs there"""
        hdr['S-BKG'] = (float(np.median(res['bkg_mini_new'])), '[e-] median background full-frame image')
        return tile_medians(sdn) if have_ref else None

    sub_pn = subimage_psfs(ctx, psf_new, nsy, nsx, size) if psf_new is not None else None

    own = []

    def reference_own_grid():
        """the reference as it comes, on its own grid: background-subtracted image + sigma mini image (made once per call: the
        registration measures its stars on it before prepare_reference brings it to the new frame)"""
        if own:
            return own[0]
        rny, rnx = ref.shape
        if ref_is_bkgsub:
            rwork = ref
            if ref_bkg_std_mini is None:
                _, rstd_mini = get_back(ctx, ref, ref_mask, bkg_boxsize=box)
                sdr = fetch(ctx, rstd_mini)
            else:
                sdr = np.asarray(ref_bkg_std_mini, np.float32)
        else:
            rmini, rstd_mini = get_back(ctx, ref, ref_mask, bkg_boxsize=box)
            rwork = torch.empty_like(ref)
            mini2back(ctx, rmini, (rny, rnx), bkg_boxsize=box, interp_Xchan=True, subtract_from=ref, subtract_into=rwork)
            res['bkg_mini_ref'], sdr_meas = fetch(ctx, rmini, rstd_mini)
            sdr = sdr_meas if ref_bkg_std_mini is None else np.asarray(ref_bkg_std_mini, np.float32)
        res['bkg_std_mini_ref'] = sdr
        own.append((rwork, sdr))
        return own[0]

    def prepare_reference():
        """the reference frame on the new frame's grid: background-subtracted image + sigma image (before the star match
        where that is asked for, else where the subtraction needs it)"""
        nonlocal bstd
        rny, rnx = ref.shape
        rwork, sdr = reference_own_grid()
        if ref_grid is not None:
            from . import coadd
            ones = torch.ones_like(rwork)
            rwork, _ = coadd.resample(ctx, rwork, ones, ref_grid, (ny, nx), 1.0, ref_grid_step)
            # (a registration's lattice lives on the device: the mini image is remapped with its host twin)
            sdr = remap_mini(sdr, ref_grid_host if ref_grid_host is not None else np.asarray(ref_grid), (rny, rnx), box, ref_grid_step,
                             shape_out=(ny, nx))
        elif (rny, rnx) != (ny, nx):
            raise ValueError('reference frame of another shape needs ref_grid')
        # co-added reference: no channel structure in its noise -> interpolation across the frame
        # (a RefPsf of this psf_ref: its own stamp tensor, the one its spectra were made of -- the library knows them by pointer)
        rpsf = ref_psf if ref_psf is not None and ref_psf.matches(psf_ref, (ny, nx), size, border) else None
        sub_pr = rpsf.stamps if rpsf is not None else subimage_psfs(ctx, psf_ref, nsy, nsx, size)
        frame_path = frame_path_supported(L) and sub_pn.shape[1] == sub_pr.shape[1]
        if ref_bkg_std is not None and ref_grid is None and tuple(ref_bkg_std.shape) == (ny, nx) and isinstance(ref_bkg_std, MiniImage) == use_mini:
            rbstd = ref_bkg_std
        elif use_mini and frame_path:
            rbstd = MiniImage(ctx, np.asarray(sdr, np.float32), box, interp_Xchan=True)
            if not mini_path_supported((ny, nx), size, border, box, rbstd):
                rbstd = rbstd.frame(ctx)
        else:
            rbstd = mini2back(ctx, sdr, (ny, nx), bkg_boxsize=box, interp_Xchan=True)
        if isinstance(bstd, MiniImage) and not (frame_path and isinstance(rbstd, MiniImage)):
            bstd = res['bkg_std'] = bstd.frame(ctx)                   # the other side needs frames: both as frames
            if isinstance(rbstd, MiniImage):
                rbstd = rbstd.frame(ctx)
        res['ref_bkgsub'], res['bkg_std_ref'] = rwork, rbstd
        hdr_t['S-BKGSTDR'] = (float(np.median(sdr)), '[e-] sigma (STD) background reference image')
        return rwork, rbstd, sdr, sub_pr, frame_path

    def register_reference(new_list):
        """ref_align: the reference's star list on its own grid (the caller's RefStars of this very reference, else made
        here), the registration against the new frame's list (ys, xs, off, flux, err on the device; None: the frame has none)
        and, where it succeeds, the lattice in place of ref_grid and the remapped mask in place of ref_mask.  Where it fails the
        frame goes on as one without a reference"""
        nonlocal ref_grid, ref_grid_host, ref_mask_remapped, have_ref, do_match
        import logging
        al, why = None, None
        try:
            if new_list is None:
                raise ValueError('the new frame has no source list (no PSF, or nothing above the threshold)')
            if psf_ref is None:
                raise ValueError('no PSF of the reference')
            rs = ref_stars if ref_stars is not None and ref_stars.matches(ref) else None
            if rs is None:
                rwork_own, sdr_own = reference_own_grid()
                rny, rnx = ref.shape
                if isinstance(psf_ref, dict) or psf_ref.dim() == 2:
                    r_nsy, r_nsx = max(1, rny // size), max(1, rnx // size)
                else:                                                # stamps of the new frame's tiling: the clamped tile's plane
                    r_nsy, r_nsx = nsy, nsx
                stamps = subimage_psfs(ctx, psf_ref, r_nsy, r_nsx, size).contiguous()
                sig_med = float(np.median(sdr_own))
                try:
                    sig = mini2back(ctx, sdr_own, (rny, rnx), bkg_boxsize=box, interp_Xchan=True)
                except (ValueError, _lib_BBXError):                  # a reference that is no multiple of the box: one level
                    sig = torch.full((rny, rnx), sig_med, dtype=torch.float32, device=ctx.device)
                rs = RefStars(ctx, rwork_own, sig, ref_mask, stamps, r_nsy, r_nsx, size, cat_nsigma, sigma_median=sig_med,
                              max_sources=max_sources, made_of=ref)
            res['ref_stars'] = rs
            al = align_reference(ctx, new_list, rs, (ny, nx), tuple(ref.shape), ref_mask, poldeg=align_poldeg, max_shift=align_max_shift,
                                 bin=align_bin, dist=match_dist, snr_min=match_snr_min, step=ref_grid_step, rounds=align_rounds,
                                 nbright=align_nbright)
            if al['flags'] != 0:
                why = 'flag word %d (vote %s)' % (al['flags'], np.asarray(al['fit']['info']).tolist())
        except Exception as e:                                       # the frame goes on without its reference
            al, why = None, str(e)
        res['align'] = al
        if why is None:
            ref_grid, ref_grid_host, ref_mask_remapped = al['grid'], align_grid_host(al['coef'], (ny, nx), ref_grid_step), al['mask']
            res['ref_mask_remapped'] = al['mask']
            hdr_t.update(al['header'])
            return True
        logging.getLogger(__name__).warning('registration of the reference failed (%s): processing the new image only', why)
        hdr_t.update(al['header'] if al is not None else align_header(None))
        hdr_t['T-NOFFR'] = ('None', 'candidates dropped: no reference there')
        hdr.update({k: v for k, v in hdr_t.items() if k.startswith('A-')})         # (no _trans products will carry them: the frame's own header does)
        have_ref = do_match = False
        return False

    ref_side = None
    # ---- full-source catalogue (a17): peaks of the background-subtracted frame above
    # cat_nsigma x S-BKGSTD, PSF-weighted optimal flux at each (zogy.get_psfoptflux)
    res['catalog'] = None
    mtab = None
    if want_cat:
        thr = float(cat_nsigma) * hdr['S-BKGSTD'][0]
        if np.isfinite(thr) and thr > 0:
            pending = find_peaks_enqueue(ctx, work, thr, max_out=max_sources)
            if do_match and not build_here and not do_align:         # (a reference to be registered is prepared behind the photometry)
                ref_side = prepare_reference()                       # (behind the search: its zoom would drop the candidate list)
            scal_n = host_side_meanwhile()
            ys, xs, pk = find_peaks_collect(ctx, pending)
        else:                                                        # no usable noise level: nothing is significant
            lib.bbx_zoom_candidates(ctx.h, None, 0.0)
            if do_match and not build_here and not do_align:
                ref_side = prepare_reference()
            scal_n = host_side_meanwhile()
            ys = xs = np.zeros(0, np.int32); pk = np.zeros(0, np.float32)
        keep = pk > 0
        ys, xs, pk = ys[keep], xs[keep], pk[keep]
        if build_here:
            # the model from this very list of peaks; from here on the frame is one whose PSF was given
            res['psf'] = build_psf(ctx, work, mini_std, new_mask, size, nsy, nsx, cat_nsigma, sigma_median=hdr['S-BKGSTD'][0],
                                   peaks=(ys, xs, pk), psf_size=psf_size, poldeg=psf_poldeg, max_sources=max_sources)
            hdr.update(res['psf']['header'])
            psf_new = res['psf']['model']
            if psf_new is not None:
                sub_pn = subimage_psfs(ctx, psf_new, nsy, nsx, size)
                if do_match and not do_align:
                    ref_side = prepare_reference()
            else:                                                    # no model: the frame of today without --psf_new
                want_phot = do_match = do_shapes = have_ref = False
    if want_phot and sub_pn is not None:
        if ys.size:
            # peaks on masked pixels are dropped; their mask values come back with the fluxes (one host wait: the photometry
            # of the few masked ones is made and thrown away)
            d_ys, d_xs = push(ctx, ys.astype(np.int64), xs.astype(np.int64))
            d_mk = new_mask[d_ys, d_xs]
            peaks_off = None
            if phot_centroid or do_shapes or do_align:
                # the windowed centroids once: for the photometry (phot_centroid), the shapes, the registration and the star match
                d_y32, d_x32 = push(ctx, ys.astype(np.int32), xs.astype(np.int32))
                sigw = window_sigma(sub_pn)
            if phot_centroid:
                peaks_off = (d_y32, d_x32, win_centroid(ctx, work, d_y32, d_x32, sigw, size, nsy, nsx))
                f, e, d_pfl = psf_optflux_centroid(ctx, work, bstd, psf_new, sub_pn, ys, xs, peaks_off[2], new_mask, nsx, size, d_peaks=(d_y32, d_x32))
            else:
                stamps = source_psfs(ctx, psf_new, sub_pn, ys, xs, nsx, size)
                f, e = psf_optflux(ctx, work, bstd, stamps, ys, xs, v_is_sigma=True)        # (bstd: frame or MiniImage)
            if do_align:
                # the registration: the new frame's list as the star match sees it (a peak on a masked pixel: no offset, no flux),
                # then the reference on this frame's grid -- before anything below asks for it
                if peaks_off is None:
                    peaks_off = (d_y32, d_x32, win_centroid(ctx, work, d_y32, d_x32, sigw, size, nsy, nsx))
                bad = d_mk != 0
                a_off = torch.where(bad[:, None], torch.full_like(peaks_off[2], float('nan')), peaks_off[2]).contiguous()
                if register_reference((d_y32, d_x32, a_off, torch.where(bad, torch.zeros_like(f), f).contiguous(), e)):
                    ref_side = prepare_reference()
            back = [d_mk, f, e]
            if do_shapes:
                # the moments and their statistics are queued behind the photometry and come back with it
                if peaks_off is None:
                    peaks_off = (d_y32, d_x32, win_centroid(ctx, work, d_y32, d_x32, sigw, size, nsy, nsx))
                d_shp, d_sfl = src_shapes(ctx, work, new_mask, d_y32, d_x32, peaks_off[2], sigw, size, nsy, nsx)
                d_stab = shape_stats(ctx, d_y32, d_x32, d_shp, d_sfl, f, e, size, nsy, nsx, shape_snr_min)
            if do_match:
                # the star match rides on the same copy back: centroids, match against the reference's catalogue (the run's,
                # or made here) and the table of clipped statistics are queued behind the photometry
                rc = ref_catalog if ref_catalog is not None and ref_catalog.matches(ref_side[0], ref_side[1], size, border, phot_centroid) else \
                    RefCatalog(ctx, ref_side[0], ref_side[1], ref_mask if ref_grid is None else ref_mask_remapped, psf_ref, size, border,
                               cat_nsigma=cat_nsigma, sigma_median=hdr_t['S-BKGSTDR'][0], sub_psfs=ref_side[3], max_sources=max_sources,
                               phot_centroid=phot_centroid)
                back += match_enqueue(ctx, work, ys, xs, d_mk, f, e, sub_pn, rc, size, nsy, nsx, match_dist, match_snr_min,
                                      peaks_off=peaks_off)
            if do_shapes:
                back += [d_shp, d_sfl, d_stab]
            if phot_centroid:
                back += [peaks_off[2], d_pfl]
            got = fetch(ctx, *back)
            mk, f, e = got[:3]
            if do_match:
                mtab, npairs = got[3:5]
                res['ref_catalog'] = rc
                res['match'] = dict(n_new=int((mk == 0).sum()), n_ref=rc.n, n_pairs=int(npairs[0]))
            ok = mk == 0
            ys, xs, pk, f, e = ys[ok], xs[ok], pk[ok], f[ok], e[ok]
            if phot_centroid:
                pfl, poff = got.pop()[ok], got.pop()[ok]              # (the last two: the flags, then the offsets)
            if do_shapes:
                shp, sfl, stab = got[-3][ok], got[-2][ok], got[-1]
        else:
            if do_align:
                register_reference(None)
            f = e = np.zeros(0, np.float32)
            shp, sfl, stab = np.zeros((0, 8), np.float32), np.zeros(0, np.uint8), empty_shape_table(nsub)
            poff, pfl = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
        if cat_extract:
            peaks = ys
            res['catalog'] = dict(Y_POS=ys.astype(np.float32) + 1, X_POS=xs.astype(np.float32) + 1,
                                  E_FLUX_PEAK=pk.astype(np.float32), E_FLUX_OPT=f, E_FLUXERR_OPT=e,
                                  SNR_OPT=np.where(e > 0, f / np.where(e > 0, e, 1), 0).astype(np.float32))
            hdr['NOBJECTS'] = (len(peaks), 'number of objects detected')
            if phot_centroid:
                # positions as shape_columns forms them: peak + 1 + offset, the integer peak where there is no centroid
                cen = ((pfl & PHOT_NO_CENTROID) == 0)[:, None]
                o = np.where(cen, poff, np.float32(0)).astype(np.float32)
                res['catalog'].update(Y_POS=(ys.astype(np.float32) + np.float32(1)) + o[:, 0], X_POS=(xs.astype(np.float32) + np.float32(1)) + o[:, 1],
                                      FLAGS_OPT=pfl.astype(np.uint8))
        if phot_centroid:
            hdr['PHOT-CEN'] = (True, 'PSF placed on the centroids in the catalogue photometry?')
        if do_shapes:
            res['catalog'].update(shape_columns(ys, xs, shp, sfl))
            res['shapes'] = dict(table=stab, n_good=int(stab[nsub, _SC['n_fwhm']]))
            hdr.update(shape_header(stab, len(ys), settings.shape_nmin, settings.pixscale))
    if 'S-BKG' not in hdr:
        scal_n = host_side_meanwhile()
    if do_align and have_ref and 'align' not in res:
        register_reference(None)                                     # (no photometry ran: no PSF of the new frame)
    if not have_ref:
        hdr['Z-P'] = (False, 'successfully processed by ZOGY?')
        res['header'], res['header_new'], res['header_trans'], res['transients'] = _HeaderView(hdr, hdr_t), hdr, hdr_t, []
        return res

    # ---- reference frame on the new frame's grid: background-subtracted image + sigma image
    rwork, rbstd, sdr, sub_pr, frame_path = ref_side if ref_side is not None else prepare_reference()

    # ---- sub-images
    scal = np.zeros((nsub, 6), np.float32)
    scal[:, 0], scal[:, 1] = scal_n, tile_medians(sdr)
    # fratio, dx, dy: one number for the frame or one per sub-image (zogy measures them per sub-image from the matched stars)
    ms = None
    if do_match:
        # measured here (match=True): per sub-image where it has the pairs, the frame's values elsewhere, the caller's as fallback
        if mtab is None:
            mtab = empty_match_table(nsub)
            res['match'] = dict(n_new=0, n_ref=ref_catalog.n if ref_catalog is not None else 0, n_pairs=0)
        ms = match_scalars(mtab, fratio, dx, dy, settings.match_nmin if match_nmin is None else match_nmin)
        if not ms['success']:
            import logging
            logging.getLogger(__name__).warning('star match: %d qualifying pairs in the frame, fewer than the minimum: fratio, dx, dy as given '
                                                'by the caller', int(mtab[nsub, 0]))
        res['match'].update(success=ms['success'], table=mtab, fratio_sub=ms['fratio_sub'], dx_sub=ms['dx_sub'], dy_sub=ms['dy_sub'])
        fratio_in, dx_in, dy_in = ms['fratio_sub'], ms['dx_sub'], ms['dy_sub']
    else:
        fratio_in, dx_in, dy_in = fratio, dx, dy
    fr = np.broadcast_to(np.asarray(fratio_in, np.float64), (nsub,))
    scal[:, 2], scal[:, 3] = 1.0, np.where(fr != 0, 1.0 / np.where(fr != 0, fr, 1.0), 1.0)
    scal[:, 4], scal[:, 5] = np.broadcast_to(np.asarray(dx_in, np.float64), (nsub,)), np.broadcast_to(np.asarray(dy_in, np.float64), (nsub,))
    if frame_path:
        # hand-written FFT path: cut, variance images, ZOGY and stitching in one library call
        outs = zogy_frame_outputs(work)                           # allocated on the caller's stream, filled inside the gate
        sub_pn, sub_pr = sub_pn.contiguous(), sub_pr.contiguous()
        nsig_cand = float(settings.transient_nsigma if nsigma is None else nsigma)
        rows = ref_rows if ref_rows is not None and ref_rows.matches(rwork, rbstd, size, border) else None
        # prepared reference PSF spectra: with prepared rows only, and only where sub_pr is the tensor they were made of
        rpsf = ref_psf if rows is not None and ref_psf is not None and sub_pr is ref_psf.stamps else None

        def zogy_frame_call():
            # the kernel that writes Scorr lists the pixels above the transient threshold for the peak search below
            check(lib.bbx_zogy_candidates(ctx.h, nsig_cand), 'bbx_zogy_candidates', ctx.h)
            with (zogy_gate or _NoGate()):
                return run_zogy_frame(ctx, work, rwork, bstd, rbstd, sub_pn, sub_pr, scal, size, border, outs=outs, ref_rows=rows, ref_psf=rpsf)
        D, _, Scorr, Fpsf, Fpsferr = zogy_frame_call()
        res['D'], res['Scorr'], res['Fpsf'], res['Fpsferr'] = D, Scorr, Fpsf, Fpsferr
    else:
        Vn = Vn if Vn is not None else variance(ctx, work, bstd)
        Vr = variance(ctx, rwork, rbstd)
        subs = [cut_subimages(ctx, a, size, border) for a in (work, rwork, Vn, Vr)]
        Pn, Pr = embed_psfs(ctx, sub_pn, L), embed_psfs(ctx, sub_pr, L)
        D, S, Scorr, Fpsf, Fpsferr = run_zogy(ctx, subs[0], subs[1], Pn, Pr, subs[2], subs[3], scal)
        del subs, Pn, Pr, S, Vr
        for name, a in (('D', D), ('Scorr', Scorr), ('Fpsf', Fpsf), ('Fpsferr', Fpsferr)):
            res[name] = stitch_subimages(ctx, a, (ny, nx), size, border)
    del D, Scorr, Fpsf, Fpsferr

    # ---- transient candidates: regions of |Scorr| >= T-NSIGMA, flux = Fpsf at the peak
    nsig = settings.transient_nsigma if nsigma is None else nsigma
    for attempt in (0, 1):
        try:
            # (the first host wait behind bbx_zogy_frame: its device-side checks surface here)
            tys, txs, tsc = find_peaks_arrays(ctx, res['Scorr'], nsig)
            ntrans = int(tys.size)
        except _lib_BBXError as e:
            if e.code == BBX_ERR_PSFWIN and frame_path and attempt == 0:
                # the matched-filter kernels of these PSFs do not fit their row window (include/bbx.h, BBX_OPT_ZOGY_KWIN_OFF):
                # V(S) of this call is off by more than the tolerance.  Once more on all rows -- the frame keeps its subtraction
                check(lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 1), 'bbx_set_option', ctx.h)
                try:
                    zogy_frame_call()
                finally:
                    check(lib.bbx_set_option(ctx.h, BBX_OPT_ZOGY_KWIN_OFF, 0), 'bbx_set_option', ctx.h)
                hdr_t['Z-KWIN'] = (False, 'ZOGY matched-filter kernels on a row window?')
                continue
            if e.code != BBX_ERR_OVERFLOW:
                raise
            # more significant pixels than the candidate list holds (a failed subtraction: wrong
            # reference, gross misalignment): the images stand, the candidate table stays empty
            tys = txs = np.zeros(0, np.int32); tsc = np.zeros(0, np.float32)
            ntrans = 'None'
        break
    # the fluxes at the candidates and the frame statistics of the header: queued together, one copy back, one host wait
    d_fe = d_st = d_fl = None
    want_thumbs = bool(thumbnails or thumbnail_pngs)
    tsize = int(thumbnail_size or settings.size_thumbnails)
    if tys.size:
        d_ys, d_xs = push(ctx, tys.astype(np.int64), txs.astype(np.int64))
        d_fe = torch.stack([res['Fpsf'][d_ys, d_xs], res['Fpsferr'][d_ys, d_xs]])
    d_edge = None
    if tys.size and ref_mask_remapped is not None:
        # the registered reference's mask under every candidate: where it carries the edge bit the frame has no reference, D
        # is the new frame there and every star a candidate
        d_edge = (ref_mask_remapped[d_ys, d_xs] & settings.mask_value['edge']).to(torch.float32)
    d_tf = None
    fit_size = int(settings.trans_fit_size if trans_fit_size is None else trans_fit_size)
    if trans_psffit:
        hdr_t['T-PSFD'] = trans_fit_header(False)['T-PSFD']          # until the fit has been read back
    if trans_psffit and tys.size and sub_pn is not None and sub_pr is not None and tuple(sub_pn.shape) == tuple(sub_pr.shape):
        try:
            d_pd, d_fold = pd_stamps(ctx, sub_pn, sub_pr, scal)
            fit = _trans_psffit(ctx, res['D'], res['data_bkgsub'], res['ref_bkgsub'], bstd, rbstd, new_mask, d_pd, tys, txs, scal, size, nsx,
                                fit_size=fit_size)
            d_tf = torch.cat([torch.stack(list(fit[:5]) + [fit[5].to(torch.float32)]).reshape(-1), d_fold])
        except Exception as e:                                       # the frame keeps today's table
            import logging
            logging.getLogger(__name__).warning('fit of P_D to the transient candidates failed: %s', e)
            d_tf = None
    d_ts = None
    shape_size = int(settings.trans_shape_size if trans_shape_size is None else trans_shape_size)
    if trans_shapefit:
        hdr_t['T-SHAPE'] = trans_shape_header(False)['T-SHAPE']      # until the fits have been read back
    if trans_shapefit and tys.size and sub_pn is not None and sub_pr is not None and tuple(sub_pn.shape) == tuple(sub_pr.shape):
        try:
            sh_out, sh_fl = _trans_shapefit(ctx, res['D'], res['data_bkgsub'], res['ref_bkgsub'], bstd, rbstd, new_mask,
                                            shape_start_fwhm(sub_pn, sub_pr), tys, txs, scal, size, nsx, fit_size=shape_size)
            d_ts = torch.cat([sh_out.reshape(-1), sh_fl.to(torch.float32).reshape(-1)])
        except Exception as e:                                       # the frame keeps today's table
            import logging
            logging.getLogger(__name__).warning('Gauss and Moffat fits to the transient candidates failed: %s', e)
            d_ts = None
    if want_thumbs:
        # the cut-outs of the four frames, which are all still in HBM, and the mask flags under each peak in one pass; the
        # display planes from the cut-outs.  The reference's mask counts only where it shares the new frame's grid
        d_fl = thumbnail_stamps(ctx, res, (res['data_bkgsub'], res['ref_bkgsub'], res['D'], res['Scorr']), tys, txs, tsize, new_mask,
                                ref_mask if ref_grid is None else ref_mask_remapped, floats=thumbnails, pngs=thumbnail_pngs)
    if frame_stats:
        # statistics over the unmasked pixels (new frame's mask), clipped like zogy's header values
        d_st = torch.stack([frame_clipped_stats_enqueue(ctx, res['Scorr'], new_mask),
                            frame_clipped_stats_enqueue(ctx, res['Fpsferr'], new_mask)])
    if d_fl is not None and not d_fl.numel():
        d_fl = None
    back = [t for t in (d_fe, d_st, d_fl, d_tf, d_ts, d_edge) if t is not None]
    got = (fetch(ctx, *back) if len(back) > 1 else [fetch(ctx, back[0])]) if back else []
    fe = got.pop(0) if d_fe is not None else None
    st = got.pop(0) if d_st is not None else None
    fl = got.pop(0) if d_fl is not None else None
    tf = got.pop(0) if d_tf is not None else None
    ts = got.pop(0) if d_ts is not None else None
    edge_at = got.pop(0) if d_edge is not None else None
    if tys.size:
        res['transients'] = [dict(y=y, x=x, scorr=sc, fpsf=f, fpsferr=e)
                             for y, x, sc, f, e in zip(tys.tolist(), txs.tolist(), tsc.tolist(), fe[0].tolist(), fe[1].tolist())]
        if fl is not None:
            for d, v in zip(res['transients'], fl.tolist()):
                d['flags'] = v
        if tf is not None:
            n = int(tys.size)
            cols, fold = tf[:6 * n].reshape(6, n), tf[6 * n:]
            for i, d in enumerate(res['transients']):
                d.update(y_psf_d=float(d['y'] + cols[2, i]), x_psf_d=float(d['x'] + cols[3, i]), flux_psf_d=float(cols[0, i]),
                         fluxerr_psf_d=float(cols[1, i]), chi2_psf_d=float(cols[4, i]), flags_psf_d=int(cols[5, i]))
            hdr_t.update(trans_fit_header(True, fit_size, res['transients'], fold))
            if len(fold) and float(np.max(fold)) > PD_FOLD_WARN:
                import logging
                logging.getLogger(__name__).warning('P_D leaves %.3g of its |sum| outside its stamp (T-PDFOLD)', float(np.max(fold)))
        if ts is not None:
            n = int(tys.size)
            planes, sfl = ts[:14 * n].reshape(2, 7, n), ts[14 * n:].reshape(2, n)
            for m, name in enumerate(('gauss', 'moffat')):
                for i, d in enumerate(res['transients']):
                    d.update({'x_%s_d' % name: float(d['x'] + planes[m, 1, i]), 'xerr_%s_d' % name: float(planes[m, 3, i]),
                              'y_%s_d' % name: float(d['y'] + planes[m, 0, i]), 'yerr_%s_d' % name: float(planes[m, 2, i]),
                              'fwhm_%s_d' % name: float(planes[m, 4, i]), 'elong_%s_d' % name: float(planes[m, 5, i]),
                              'chi2_%s_d' % name: float(planes[m, 6, i]), 'flags_%s_d' % name: int(sfl[m, i])})
            hdr_t.update(trans_shape_header(True, shape_size, settings.trans_moffat_beta, res['transients']))
        if edge_at is not None:
            # candidates without a reference under their peak leave, with their thumbnails; T-NTRANS stays the count before
            keep = [i for i, v in enumerate(edge_at.tolist()) if not v]
            if len(keep) < len(res['transients']):
                res['transients'] = [res['transients'][i] for i in keep]
                for k in ('thumbnails', 'thumbnail_png8'):
                    if k in res:
                        res[k] = res[k][torch.as_tensor(keep, dtype=torch.int64, device=res[k].device)]
            hdr_t['T-NOFFR'] = (int(tys.size) - len(keep), 'candidates dropped: no reference there')
        # the vetting: the chi2 bound needs the fit of P_D, the Gauss bounds the shape fits
        bounds = dict(chi2_max=trans_chi2_max if tf is not None else None)
        if ts is not None:
            bounds.update(fwhm_gauss_min=trans_fwhm_gauss_min, fwhm_gauss_max=trans_fwhm_gauss_max, elong_gauss_max=trans_elong_gauss_max)
        if any(v is not None for v in bounds.values()):
            res['transients'], keep = vet_transients(res['transients'], **{k: None if v is None else float(v) for k, v in bounds.items()})
            for k in ('thumbnails', 'thumbnail_png8'):
                if k in res:
                    res[k] = res[k][torch.as_tensor(keep, dtype=torch.int64, device=res[k].device)]
            hdr_t['T-NVET'] = (len(keep), 'number of transient candidates that passed the vetting')
    else:
        res['transients'] = []
    if ref_mask_remapped is not None and 'T-NOFFR' not in hdr_t:
        hdr_t['T-NOFFR'] = (0, 'candidates dropped: no reference there')
    hdr['Z-P'] = (True, 'successfully processed by ZOGY?')
    for h in (hdr, hdr_t):
        h['Z-SIZE'] = (size, '[pix] size of (square) ZOGY subimages')
        h['Z-BSIZE'] = (border, '[pix] size of ZOGY subimage borders')
    if ms is not None:
        hdr_t.update(ms['header'])
    else:
        hdr_t['Z-DX'] = (float(np.median(dx)), '[pix] dx median offset full image')
        hdr_t['Z-DY'] = (float(np.median(dy)), '[pix] dy median offset full image')
        hdr_t['Z-FNR'] = (float(np.median(fratio)), 'median flux ratio (Fnew/Fref) full image')
    if frame_stats:
        hdr_t['Z-SCMED'] = (float(st[0, 1]), 'median Scorr full image')
        hdr_t['Z-SCSTD'] = (float(st[0, 3]), 'sigma (STD) Scorr full image')
        hdr_t['Z-FPEMED'] = (float(st[1, 1]), '[e-] median Fpsferr full image')
        hdr_t['Z-FPESTD'] = (float(st[1, 3]), '[e-] sigma (STD) Fpsferr full image')
    hdr_t['T-NSIGMA'] = (float(nsig), '[sigma] transient detection threshold')
    hdr_t['T-NTRANS'] = (ntrans, 'number of transient candidates')
    res['header'] = _HeaderView(hdr, hdr_t)
    res['header_new'], res['header_trans'] = hdr, hdr_t
    res['scal'] = scal
    return res


def thumbnail_stamps(ctx, res, frames, ys, xs, size, new_mask, ref_mask=None, floats=True, pngs=False, flag_win=None):
    """bbx_thumbnails (+ bbx_thumb_png8) at the integer positions (ys, xs) of the four frames (RED, REF, D, SCORR): puts
    'thumbnails' (device float32 [n, 4, size, size], when [floats]) and 'thumbnail_png8' (device uint8, same shape, when [pngs])
    into [res] and returns the device flags [n] (uint8: OR of the masks over the flag window); n = 0 gives empty tensors and
    launches nothing.  No host wait"""
    n = int(len(ys))
    dev = ctx.device
    out = torch.empty((n, 4, size, size), dtype=torch.float32, device=dev)
    d_fl = torch.empty(n, dtype=torch.uint8, device=dev)
    png = torch.empty((n, 4, size, size), dtype=torch.uint8, device=dev) if pngs else None
    if n:
        frames = [f.contiguous() for f in frames]
        ny, nx = frames[0].shape
        for f in frames:
            if f.dtype != torch.float32 or tuple(f.shape) != (ny, nx):
                raise ValueError('thumbnail frames must be float32 of one shape')
        for m in (new_mask, ref_mask):
            if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != (ny, nx) or not m.is_contiguous()):
                raise ValueError('thumbnail masks must be contiguous uint8 frames of the image shape')
        d_y32, d_x32 = push(ctx, np.asarray(ys, np.int32), np.asarray(xs, np.int32))
        planes = (C.c_void_p * 4)(*[f.data_ptr() for f in frames])
        win = int(settings.trans_flags_window if flag_win is None else flag_win)
        check(lib.bbx_thumbnails(ctx.h, ny, nx, planes, n, _p(d_y32), _p(d_x32), size, _p(new_mask),
                                 _p(ref_mask) if ref_mask is not None else None, win, _p(out), _p(d_fl), ctx.stream()),
              'bbx_thumbnails', ctx.h)
        if pngs:
            check(lib.bbx_thumb_png8(ctx.h, 4 * n, size, _p(out), _p(png), None, ctx.stream()), 'bbx_thumb_png8', ctx.h)
    if floats:
        res['thumbnails'] = out
    if pngs:
        res['thumbnail_png8'] = png
    return d_fl


class _HeaderView(dict):
    """header_new additions as {KEY: (value, comment)}; item access also finds header_trans
    keys and returns plain values (what the callers of the tensor-level function read)"""

    def __init__(self, hdr, hdr_t):
        dict.__init__(self, hdr)
        self._t = hdr_t

    def __getitem__(self, k):
        v = dict.__getitem__(self, k) if dict.__contains__(self, k) else self._t[k]
        return v[0] if isinstance(v, tuple) else v
