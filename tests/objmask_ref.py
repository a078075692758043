"""CPU restatement of the object-mask rules (include/bbx.h, bbx_object_mask) in numpy + scipy.ndimage, and
the crowded scene the second background pass is checked on.  Shared by tests/test_objmask_host.py and tests/test_gpu_objmask.py."""
import numpy as np
from scipy import ndimage

F = np.float32

SKY, RDNOISE, SIGMA_TRUE = 300.0, 10.0, 20.0          # e-: sigma^2 = sky + rdnoise^2


def detection_image(img, filter=True):
    """the 3x3 pyramid (1 2 1 / 2 4 2 / 1 2 1) / 16 with replicated edges, in float32 and in the order of the rule"""
    img = np.ascontiguousarray(img, F)
    if not filter:
        return img
    p = np.pad(img, 1, mode='edge')
    nw, n, ne = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    w, c, e = p[1:-1, :-2], p[1:-1, 1:-1], p[1:-1, 2:]
    sw, s, se = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    with np.errstate(all='ignore'):
        filt = (((nw + ne) + (sw + se)) + F(2) * ((n + s) + (w + e)) + F(4) * c) * F(0.0625)
    assert filt.dtype == F
    return filt


def listed_pixels(img, sig_mini, box, nsigma=1.5, filter=True):
    filt = detection_image(img, filter)
    thr = F(nsigma) * np.asarray(sig_mini, F)                          # one float32 product per box
    thr = np.repeat(np.repeat(thr, box, axis=0), box, axis=1)
    assert thr.shape == filt.shape and thr.dtype == F
    with np.errstate(invalid='ignore'):
        return (thr > 0) & (filt >= thr) & (filt < np.inf)


def disk(grow):
    yy, xx = np.mgrid[-grow:grow + 1, -grow:grow + 1]
    return yy * yy + xx * xx <= grow * grow


def object_mask_ref(img, sig_mini, box, nsigma=1.5, minarea=5, grow=3, filter=True):
    """-> (objmask uint8 [ny, nx], (pixels listed, components kept, pixels set))"""
    listed = listed_pixels(img, sig_mini, box, nsigma, filter)
    lab, n = ndimage.label(listed, structure=np.ones((3, 3)))
    keep = np.bincount(lab.ravel(), minlength=n + 1) >= minarea
    keep[0] = False
    kept = keep[lab]
    mask = ndimage.binary_dilation(kept, structure=disk(grow)) if grow > 0 else kept
    return mask.astype(np.uint8), (int(listed.sum()), int(keep.sum()), int(mask.sum()))


# ---- hand-made frames: sigma 2.0 per box unless said otherwise, so the threshold at nsigma 1.5 is 3.0 exactly -------------------
BRIGHT = F(100.0)
THR = F(3.0)
BELOW = np.nextafter(THR, F(0))                        # one ulp below the threshold; a 3x3 of it filters to itself


def frame_shapes(ny=140, nx=220, box=20):
    """-> (img, sig, box, where): objects on all corners and edges, blobs touching diagonally / two pixels apart, components of
    minarea and minarea - 1 pixels, a U, a W and a comb open to the top, patches at the threshold and one ulp below, two objects
    whose disks overlap, a dropped component next to a kept one.  where: name -> the place the host test looks at"""
    assert ny >= 140 and nx >= 220
    img = np.zeros((ny, nx), F)
    sig = np.full((ny // box, nx // box), 2.0, F)
    for sl in ((slice(0, 3), slice(0, 3)), (slice(0, 3), slice(nx - 3, nx)), (slice(ny - 3, ny), slice(0, 3)), (slice(ny - 3, ny), slice(nx - 3, nx)),
               (slice(0, 2), slice(100, 104)), (slice(ny - 2, ny), slice(60, 64)), (slice(60, 64), slice(0, 2)), (slice(80, 84), slice(nx - 2, nx))):
        img[sl] = BRIGHT
    img[20:22, 20:22] = BRIGHT; img[22, 22] = BRIGHT                 # touch only diagonally: 5 pixels together
    img[20:22, 40:42] = BRIGHT; img[22, 43] = BRIGHT                 # the same two pixels apart: 4 + 1
    img[30, 60:65] = BRIGHT                                          # minarea
    img[30, 80:84] = BRIGHT                                          # minarea - 1
    img[40:48, 100] = BRIGHT; img[40:48, 104] = BRIGHT; img[48, 100:105] = BRIGHT                                # U
    for x in (120, 124, 128):
        img[40:48, x] = BRIGHT
    img[48, 120:129] = BRIGHT                                        # W
    for x in range(140, 160, 2):
        img[40:50, x] = BRIGHT
    img[50, 140:159] = BRIGHT                                        # comb: ten arms that meet only below
    img[100:105, 20:25] = THR                                        # at the threshold (filtered: its inner 3 x 3)
    img[100:105, 40:45] = BELOW                                      # one ulp below: nothing
    img[125:128, 60:63] = BRIGHT; img[125:128, 68:71] = BRIGHT       # disks of radius 3 overlap
    img[125, 90:92] = BRIGHT; img[125:128, 96:99] = BRIGHT           # a dropped component next to a kept one
    where = dict(diag=(20, 20), apart=(20, 40), minarea=(30, 60), below_minarea=(30, 80), U=(48, 100), W=(48, 120), comb=(50, 140),
                 thr=(102, 22), below=(102, 42), dropped=(125, 90), kept=(126, 97))
    return img, sig, box, where


def frame_shapes_small():
    """the same kinds of objects on 64 x 64 with boxes of 32"""
    ny = nx = 64
    img = np.zeros((ny, nx), F)
    sig = np.full((2, 2), 2.0, F)
    for sl in ((slice(0, 3), slice(0, 3)), (slice(0, 3), slice(nx - 3, nx)), (slice(ny - 3, ny), slice(0, 3)), (slice(ny - 3, ny), slice(nx - 3, nx)),
               (slice(0, 2), slice(30, 34)), (slice(ny - 2, ny), slice(24, 28)), (slice(30, 34), slice(0, 2)), (slice(20, 24), slice(nx - 2, nx))):
        img[sl] = BRIGHT
    img[10:12, 10:12] = BRIGHT; img[12, 12] = BRIGHT
    img[10:12, 20:22] = BRIGHT; img[12, 23] = BRIGHT
    img[16, 30:35] = BRIGHT
    img[16, 40:44] = BRIGHT
    img[24:30, 10] = BRIGHT; img[24:30, 14] = BRIGHT; img[30, 10:15] = BRIGHT
    for x in range(40, 52, 2):
        img[24:32, x] = BRIGHT
    img[32, 40:51] = BRIGHT
    img[40:45, 8:13] = THR
    img[40:45, 20:25] = BELOW
    img[50:53, 30:33] = BRIGHT; img[50:53, 38:41] = BRIGHT
    img[56, 8:10] = BRIGHT; img[55:58, 14:17] = BRIGHT
    return img, sig, 32


def frame_values(ny=140, nx=220, box=20):
    """-> (img, sig, box): one-pixel diagonals across the whole frame (both directions), NaN and +Inf inside a bright blob, boxes
    whose sigma is NaN, 0 or negative under bright blobs, a blob straddling two boxes of different sigma, on faint noise"""
    rs = np.random.RandomState(5)
    img = rs.normal(0.0, 0.5, (ny, nx)).astype(F)
    nby, nbx = ny // box, nx // box
    sig = np.full((nby, nbx), 2.0, F)
    k = np.arange(min(ny, nx))
    img[k, k] = BRIGHT
    img[k, nx - 1 - k] = BRIGHT
    by, bx = nby - 1, nbx // 2                                       # a bright blob with a NaN and an Inf inside
    y0, x0 = by * box + 2, bx * box + 2
    img[y0:y0 + 9, x0:x0 + 9] = BRIGHT
    img[y0 + 3, x0 + 3], img[y0 + 6, x0 + 6] = np.nan, np.inf
    for j, s in enumerate((np.nan, 0.0, -2.0)):                      # sigma that lists nothing, under a bright blob each
        by, bx = j % nby, nbx - 1 - (j // nby)
        if (by, bx) == (nby - 1, nbx // 2):
            continue
        sig[by, bx] = s
        img[by * box + box // 2 - 3:by * box + box // 2 + 3, bx * box + box // 2 - 3:bx * box + box // 2 + 3] = BRIGHT
    if nbx >= 4:                                                     # value 50 across the border of a box with threshold 60
        sig[nby // 2, 1] = 40.0
        img[(nby // 2) * box + 5:(nby // 2) * box + 11, box - 5:box + 5] = 50.0
    return img, sig, box


def moffat_scene(seed, ny=240, nx=240, nstars=120, fwhm=4.0, beta=2.5):
    """sky of 300 e-, read noise of 10 e- (true sigma 20.0), [nstars] Moffat stars (beta 2.5, FWHM 4 px, flux 10^U(3, 5.5)) at
    uniformly random positions, Poisson noise -> float32 frame (with its sky)"""
    rs = np.random.RandomState(seed)
    ys, xs = rs.uniform(0, ny, nstars), rs.uniform(0, nx, nstars)
    flux = 10.0 ** rs.uniform(3.0, 5.5, nstars)
    alpha = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / beta) - 1.0))
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    img = np.full((ny, nx), SKY)
    for y, x, f in zip(ys, xs, flux):
        img += f * (beta - 1.0) / (np.pi * alpha * alpha) * (1.0 + ((yy - y) ** 2 + (xx - x) ** 2) / (alpha * alpha)) ** -beta
    return (rs.poisson(img) + rs.normal(0.0, RDNOISE, (ny, nx))).astype(F)


def two_pass_background(data, mask, box, **kw):
    """the oracle's mesh twice (oracle/zogy_core.py): -> dict(mini1, std1, work1, objmask, counts, raw2, mini2, std2); raw2: the
    second pass's mini images before the fill (NaN = below limfrac)"""
    import zogy_core as Z
    mini1, std1 = [Z.fill_filter_mini(a) for a in Z.get_back_mini(data, mask, None, box)]
    work1 = (data - Z.mini2back(mini1, data.shape, box)).astype(F)
    objmask, counts = object_mask_ref(work1, std1, box, **kw)
    raw2 = Z.get_back_mini(data, mask, objmask, box)
    mini2, std2 = [Z.fill_filter_mini(a) for a in raw2]
    return dict(mini1=mini1, std1=std1, work1=work1, objmask=objmask, counts=counts, raw2=raw2, mini2=mini2, std2=std2)
