"""The background mesh of a frame (zogy.get_back), the object mask and the second, object-free pass, the
variance image and the clipped frame statistics of the header."""
import logging

import numpy as np
import torch

from . import _args, settings
from ._lib import lib, check, fetch, push, ptr as _p

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
    ny, nx = _args.frame(img)
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


def variance(ctx, data_bkgsub, bkg_std):
    v = torch.empty_like(data_bkgsub)
    check(lib.bbx_variance(ctx.h, data_bkgsub.numel(), _p(data_bkgsub), _p(bkg_std), _p(v), ctx.stream()), 'bbx_variance', ctx.h)
    return v


def frame_clipped_stats_enqueue(ctx, img, mask=None, step=8):
    """queue bbx_frame_clipped_stats of a contiguous float32 frame -> device tensor [8] (n, median, mean, sigma, ...)"""
    ny, nx = _args.frame(img)
    _args.mask(mask, (ny, nx))
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
