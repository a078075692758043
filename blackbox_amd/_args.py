"""The argument rules of the frame-level ctypes wrappers, each stated once.  A wrapper hands bare pointers to the C ABI, which
cannot see extents: what these refuse (always a ValueError, before the wrapper's first library call or push) would be a
device fault.  Plain functions on the tensors' dtype, shape and layout; where a tensor lives is not asked (reduce._expect
asks that too)."""
import numpy as np
import torch

from ._lib import ptr, push
from .zoom import MiniImage


def frame(img, shape=None):
    """a contiguous 2-D float32 frame, of [shape] where one is given -> its shape"""
    if img.dim() != 2 or img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError('contiguous 2-D float32 frame expected')
    if shape is not None and tuple(img.shape) != tuple(shape):
        raise ValueError('contiguous 2-D float32 frames of one shape expected')
    return img.shape


def frames(first, *others):
    """several frames of one shape -> that shape"""
    shape = frame(first)
    for f in others:
        frame(f, shape)
    return shape


def mask(m, shape):
    """None, or a contiguous uint8 frame of the image shape"""
    if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != tuple(shape) or not m.is_contiguous()):
        raise ValueError('the mask must be a contiguous uint8 frame of the image shape')


def sigma_map(sigma, shape):
    """a sigma map: a contiguous float32 frame of the image shape or a MiniImage -> what the C call takes for it: (the frame's
    pointer or None, the mini image's ref() or None)"""
    if isinstance(sigma, MiniImage):
        return None, sigma.ref()
    if sigma.dtype != torch.float32 or tuple(sigma.shape) != tuple(shape) or not sigma.is_contiguous():
        raise ValueError('sigma: a contiguous float32 frame of the image shape or a MiniImage expected')
    return ptr(sigma), None


def sigma_maps(sig_n, sig_r, shape):
    """the two sigma maps of one form, two frames or two MiniImage -> the C call's quartet (pointer n, pointer r, ref n, ref r)"""
    if isinstance(sig_n, MiniImage) != isinstance(sig_r, MiniImage):
        raise ValueError('the two sigma maps must be of one form: two frames or two MiniImage')
    (p_n, r_n), (p_r, r_r) = sigma_map(sig_n, shape), sigma_map(sig_r, shape)
    return p_n, p_r, r_n, r_r


def scal6(scal, nsub=None):
    """scal [nsub, 6] = (sigma_n, sigma_r, f_n, f_r, dx, dy) per sub-image (host) -> contiguous float32; nsub None: as many rows
    as it has"""
    scal = np.ascontiguousarray(scal, dtype=np.float32)
    if scal.ndim != 2 or scal.shape[1] != 6 or (nsub is not None and scal.shape[0] != nsub):
        raise ValueError('scal [nsub, 6] expected')
    return scal


def peaks(ctx, ys, xs, d_peaks=None):
    """the candidate positions: ys, xs host arrays; d_peaks: their int32 device copies (d_ys, d_xs) where the caller has them,
    else they are pushed -> (n, d_ys, d_xs)"""
    ys, xs = np.asarray(ys), np.asarray(xs)
    n = int(ys.size)
    if d_peaks is None:
        return (n,) + tuple(push(ctx, ys.astype(np.int32), xs.astype(np.int32)))
    d_ys, d_xs = d_peaks
    if d_ys.dtype != torch.int32 or d_xs.dtype != torch.int32 or d_ys.numel() != n or d_xs.numel() != n:
        raise ValueError('d_peaks: the int32 device copies of ys, xs expected')
    return n, d_ys, d_xs
