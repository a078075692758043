"""The ZOGY launch wrappers: sub-image path (rocFFT: cut, bbx_zogy_subimages, stitch) and whole-frame path (bbx_zogy_frame,
bbx_zogy_frame_mini) with the reference's prepared halves (RefRows, RefPsf), and the gate that lets one stream at a time
into the frame kernels."""
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import settings
from ._lib import lib, check, ptr as _p
from .psfphot import subimage_psfs
from .zoom import MiniImage


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


class StreamGate:
    """Lets one stream at a time run a section on the GPU: a section starts when the previous one (of any
    stream) has finished.  bbx_zogy_frame's kernels each fill the whole GPU; two lanes running them side
    by side only slice each other's time.  With priority=True the sections run on ONE high-priority stream of the
    gate's own (in order: that is the gate), between a wait for the caller's stream and a wait of the caller's stream:
    the short kernels of the other lanes then take the CUs a section leaves free instead of an equal share of all of
    them.  Tensors a section is to fill must be allocated before it (they belong to the caller's stream)."""

    def __init__(self, device=None, priority=False):
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
