"""The argument rules of the ctypes wrappers (blackbox_amd/_args.py) on CPU tensors: a wrapper hands bare pointers to the C ABI,
so what it refuses is all that stands between a wrong argument and a device fault.  Part 1: every rule accepts the good case
and refuses each way of being wrong.  Part 2: every wrapper that states its checks through the rules refuses a bad argument
with ctx=None, i.e. before it could have called the library or pushed anything."""
import numpy as np
import pytest
import torch

from blackbox_amd import _args
from blackbox_amd import zogy as G

NY, NX, NSUB = 8, 12, 2
F32 = torch.float32


def frame(dtype=F32, shape=(NY, NX)):
    return torch.zeros(shape, dtype=dtype)


def strided():
    """a float32 [NY, NX] view that is not contiguous"""
    return torch.zeros((NY, 2 * NX), dtype=F32)[:, ::2]


def mini():
    """a MiniImage without its device half: the rules ask only what it is, and for its ref()"""
    m = G.MiniImage.__new__(G.MiniImage)
    m.c = G._SplineImage()
    return m


BAD_FRAMES = {'dtype': lambda: frame(torch.float64), 'rank': lambda: frame(shape=(1, NY, NX)), 'strided': strided}
BAD_MASKS = {'dtype': lambda: frame(torch.int8), 'shape': lambda: frame(torch.uint8, (NY, NX + 1)), 'rank': lambda: frame(torch.uint8, (1, NY, NX)),
             'strided': lambda: torch.zeros((NY, 2 * NX), dtype=torch.uint8)[:, ::2]}
BAD_SIGMAS = {'dtype': lambda: frame(torch.float64), 'shape': lambda: frame(shape=(NY + 1, NX)), 'rank': lambda: frame(shape=(1, NY, NX)),
              'strided': strided}


# ---- part 1: the rules ----------------------------------------------------------------------------------------------
def test_frame_accepts():
    assert tuple(_args.frame(frame())) == (NY, NX)
    assert tuple(_args.frame(frame(), (NY, NX))) == (NY, NX)
    assert tuple(_args.frames(frame(), frame(), frame())) == (NY, NX)


@pytest.mark.parametrize('how', sorted(BAD_FRAMES))
def test_frame_refuses(how):
    with pytest.raises(ValueError):
        _args.frame(BAD_FRAMES[how]())
    with pytest.raises(ValueError):
        _args.frames(frame(), BAD_FRAMES[how]())


def test_frame_refuses_another_shape():
    with pytest.raises(ValueError):
        _args.frame(frame(), (NY, NX + 1))
    with pytest.raises(ValueError):
        _args.frames(frame(), frame(shape=(NY, NX + 1)))


def test_mask_accepts():
    _args.mask(None, (NY, NX))
    _args.mask(frame(torch.uint8), (NY, NX))


@pytest.mark.parametrize('how', sorted(BAD_MASKS))
def test_mask_refuses(how):
    with pytest.raises(ValueError):
        _args.mask(BAD_MASKS[how](), (NY, NX))


def test_sigma_accepts():
    a, b = frame(), frame()
    pn, pr, rn, rr = _args.sigma_maps(a, b, (NY, NX))
    assert (pn.value, pr.value, rn, rr) == (a.data_ptr(), b.data_ptr(), None, None)
    pn, pr, rn, rr = _args.sigma_maps(mini(), mini(), (NY, NX))
    assert pn is None and pr is None and rn is not None and rr is not None
    p, r = _args.sigma_map(a, (NY, NX))
    assert p.value == a.data_ptr() and r is None
    p, r = _args.sigma_map(mini(), (NY, NX))
    assert p is None and r is not None


@pytest.mark.parametrize('how', sorted(BAD_SIGMAS))
def test_sigma_refuses(how):
    with pytest.raises(ValueError):
        _args.sigma_map(BAD_SIGMAS[how](), (NY, NX))
    for pair in ((frame(), BAD_SIGMAS[how]()), (BAD_SIGMAS[how](), frame())):
        with pytest.raises(ValueError):
            _args.sigma_maps(pair[0], pair[1], (NY, NX))


def test_sigma_refuses_mixed_forms():
    for pair in ((frame(), mini()), (mini(), frame())):
        with pytest.raises(ValueError):
            _args.sigma_maps(pair[0], pair[1], (NY, NX))


def test_scal_accepts():
    s = _args.scal6(np.zeros((NSUB, 6)), NSUB)
    assert s.dtype == np.float32 and s.flags.c_contiguous and s.shape == (NSUB, 6)
    assert _args.scal6(np.zeros((2 * NSUB, 6), np.float32)[::2]).flags.c_contiguous           # (the length from scal itself)
    assert _args.scal6([[0.0] * 6] * 3).shape == (3, 6)


@pytest.mark.parametrize('shape', [(NSUB, 5), (NSUB + 1, 6), (NSUB * 6,), (1, NSUB, 6)])
def test_scal_refuses(shape):
    with pytest.raises(ValueError):
        _args.scal6(np.zeros(shape, np.float32), NSUB)


@pytest.mark.parametrize('shape', [(NSUB, 5), (NSUB * 6,), (1, NSUB, 6)])
def test_scal_of_its_own_length_refuses(shape):
    with pytest.raises(ValueError):
        _args.scal6(np.zeros(shape, np.float32))


def test_peaks_accepts_device_copies():
    ys, xs = [1, 2, 3], np.array([4, 5, 6])
    d = (torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    n, d_ys, d_xs = _args.peaks(None, ys, xs, d)                 # (ctx None: nothing is pushed)
    assert n == 3 and d_ys is d[0] and d_xs is d[1]


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('how', ['dtype', 'length'])
def test_peaks_refuses(which, how):
    d = [torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)]
    d[which] = torch.zeros(3, dtype=torch.int64) if how == 'dtype' else torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        _args.peaks(None, [1, 2, 3], [4, 5, 6], tuple(d))


# ---- part 2: the wrappers refuse before they touch the context (ctx=None) -------------------------------------------------
# thumbnail_stamps is not here: it reads ctx.device for its output tensors before it looks at its frames
def trans_args(**kw):
    a = dict(D=frame(), N=frame(), R=frame(), sig_n=frame(), sig_r=frame(), mask=frame(torch.uint8), ys=[1, 2], xs=[3, 4],
             scal=np.zeros((NSUB, 6), np.float32), d_peaks=(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)))
    a.update(kw)
    return a


TRANS_BAD = dict(frame=dict(N=frame(torch.float64)), frame_shape=dict(R=frame(shape=(NY, NX + 1))), frame_strided=dict(D=strided()),
                 mask=dict(mask=frame(torch.uint8, (NY + 1, NX))), sigma_mixed=dict(sig_r=mini()), sigma=dict(sig_n=frame(torch.float64)),
                 scal=dict(scal=np.zeros((NSUB, 5), np.float32)), peaks_dtype=dict(d_peaks=(torch.zeros(2, dtype=torch.int64),) * 2),
                 peaks_length=dict(d_peaks=(torch.zeros(3, dtype=torch.int32),) * 2))


@pytest.mark.parametrize('how', sorted(TRANS_BAD))
def test_trans_psffit_refuses_first(how):
    a = trans_args(**TRANS_BAD[how])
    with pytest.raises(ValueError):
        G.trans_psffit(None, a['D'], a['N'], a['R'], a['sig_n'], a['sig_r'], a['mask'], torch.zeros((NSUB, 5, 5)), a['ys'], a['xs'], a['scal'],
                       4, 3, d_peaks=a['d_peaks'])


@pytest.mark.parametrize('how', sorted(TRANS_BAD))
def test_trans_shapefit_refuses_first(how):
    a = trans_args(**TRANS_BAD[how])
    with pytest.raises(ValueError):
        G.trans_shapefit(None, a['D'], a['N'], a['R'], a['sig_n'], a['sig_r'], a['mask'], torch.zeros(NSUB), a['ys'], a['xs'], a['scal'],
                         4, 3, d_peaks=a['d_peaks'])


def test_pd_stamps_refuses_first():
    with pytest.raises(ValueError):
        G.pd_stamps(None, torch.zeros((NSUB, 5, 5)), torch.zeros((NSUB, 5, 5)), np.zeros((NSUB + 1, 6), np.float32))


@pytest.mark.parametrize('bad', ['frame', 'mask'])
def test_psf_optflux_centroid_refuses_first(bad):
    D = frame(torch.float64) if bad == 'frame' else frame()
    m = frame(torch.uint8, (NY, NX + 1)) if bad == 'mask' else None
    with pytest.raises(ValueError):
        G.psf_optflux_centroid(None, D, frame(), None, torch.zeros((NSUB, 5, 5)), [1], [1], torch.zeros((1, 2)), m, 1, 4)


@pytest.mark.parametrize('bad', ['frame', 'mask'])
def test_src_shapes_refuses_first(bad):
    img = strided() if bad == 'frame' else frame()
    m = frame(torch.int8) if bad == 'mask' else None
    d = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        G.src_shapes(None, img, m, d, d, torch.zeros((2, 2)), torch.zeros(NSUB), 4, 1, 2)


@pytest.mark.parametrize('bad', ['frame', 'mask'])
def test_psf_stamps_refuses_first(bad):
    img = frame(shape=(1, NY, NX)) if bad == 'frame' else frame()
    m = frame(torch.uint8, (NY, NX + 1)) if bad == 'mask' else None
    d = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        G.psf_stamps(None, img, m, d, d, torch.zeros((2, 8)), torch.zeros(2), 5, 2)


def test_win_centroid_refuses_first():
    d = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        G.win_centroid(None, frame(torch.float64), d, d, torch.zeros(NSUB), 4, 1, 2)


def test_object_mask_enqueue_refuses_first():
    with pytest.raises(ValueError):
        G.object_mask_enqueue(None, strided(), torch.zeros((2, 3)), 4)


@pytest.mark.parametrize('bad', ['frame', 'mask'])
def test_frame_clipped_stats_refuses_first(bad):
    img = frame(torch.float64) if bad == 'frame' else frame()
    m = frame(torch.uint8, (NY + 1, NX)) if bad == 'mask' else None
    with pytest.raises(ValueError):
        G.frame_clipped_stats_enqueue(None, img, m)


def test_build_psf_refuses_first():
    with pytest.raises(ValueError):
        G.build_psf(None, frame(torch.float64), 1.0, None, 4, 2, 3)


def test_ref_catalog_refuses_first():
    with pytest.raises(ValueError):
        G.RefCatalog(None, strided(), frame(), None, None, 4, 1)


def test_remap_mask_refuses_first():
    with pytest.raises(ValueError):
        G.remap_mask(None, frame(torch.int8), (NY, NX), torch.zeros((2, 2, 2), dtype=torch.float64), (NY, NX))
