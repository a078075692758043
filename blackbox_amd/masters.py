"""Master calibration frames (reference create_masters / master_prep, blackbox.py:617-782, 4625-5247).

Files in, one master file out.  The host side chooses and labels the frames the way the reference
does; the per-pixel work runs on the GPU:

  selection   select_frames          reduced frames of the evening date +- cal_window days (4700-4890):
                                     name filter, QC-FLAG red, ML1's 2019-2020 evening flats, BlackGEM's
                                     evening flats, the ncal_max nearest 23:59 UT, < 5 frames / all old
  inputs      load_frames            .fits float32 (bytes up, bbx_be32) and .fits.fz (bbx_funpack_tiles);
                                     reader threads overlap the file reads with the device decodes
  stack       master_median          MEDSEC normalisation + pixel-wise median (bbx_median_stack)
  statistics  flat_statistics        STATSEC / MFMEDSEC / MFSTDSEC / MFMED / MFSTD (bbx_rect_stats,
              gain_correction_factors  bbx_rect_clipped_stats), dithering, GAINCF{c};
              master_level_stats     MB* / MD* for bias and dark
  file        master_prep            existing master (already_exists, qc_flagged), lock, header in the
                                     reference's order, qc.run_qc_check, DATEFILE, atomic write
  fallback    get_nearest_master     yesterday's master, else the nearest non-red .fits.fz master of the
                                     previous / current / next month (5291-5391)
  night       create_masters         the masters of one evening date or of a list of dates (617-782)

Deviations from the reference, all deliberate:
  * a frame present as both .fits and .fits.fz counts once (the .fz copy); the reference stacks it twice;
  * an existing master with a red QC flag is built again from the frames; the reference looks for a
    nearby master instead (master_prep 4781);
  * the header statistics use every valid pixel, not the reference's unseeded 20 % subsample
    (get_rand_indices); MFMED / MFSTD are sigma-clipped over the whole master;
  * NaN pixels of the inputs do not propagate through the median stack (bbx_median_stack sorts with
    min / max; numpy's median would give NaN);
  * the default filter list (u g q r i z) stands for set_zogy.zp_default's keys, a module that is not
    part of the reference tree; create_masters accepts an evening date or a file of dates only (the
    reference's yyyy / yyyymm forms end up in directories that do not exist);
  * dates are computed with datetime (UTC, days of 86400 s) in place of astropy's Time.
"""
import ctypes as C
import datetime
import logging
import os
import time

import numpy as np
import torch

from . import _lib, settings
from ._lib import lib, check

log = logging.getLogger(__name__)
get_par = settings.get_par


def master_median(ctx, frames, imgtype, medsec=None, bpm=None):
    """frames: list of contiguous float32 device tensors of equal shape (the reduced
    bias/dark/flat frames).  imgtype 'flat': medsec = list of the frames' MEDSEC header
    values (median over set_bb.flat_norm_sec); bpm: uint8 bad-pixel mask or None.
    -> master float32 device tensor"""
    n = len(frames)
    if n < 1 or n > 32:
        raise ValueError('1..32 frames expected, got {}'.format(n))
    shape = frames[0].shape
    for f in frames:
        if f.dtype != torch.float32 or f.shape != shape or not f.is_contiguous():
            raise ValueError('frames must be contiguous float32 tensors of equal shape')
    out = torch.empty(shape, dtype=torch.float32, device=ctx.device)
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    norm = None
    if imgtype == 'flat':
        if medsec is None or len(medsec) != n:
            raise ValueError('flat frames need their MEDSEC values')
        norm = (C.c_float * n)(*[float(m) for m in medsec])
    check(lib.bbx_median_stack(ctx.h, out.numel(), n, ptrs, norm,
                               C.c_void_p(bpm.data_ptr()) if (bpm is not None and imgtype == 'flat') else None,
                               1 if (imgtype == 'flat' and bpm is not None) else 0,
                               C.c_void_p(out.data_ptr()), ctx.stream()), 'bbx_median_stack', ctx.h)
    return out


def _rect_scale(ctx, t, y0, x0, ny, nx, factor, divide):
    NY, NX = t.shape
    if not (0 <= y0 and 0 <= x0 and ny >= 1 and nx >= 1 and y0 + ny <= NY and x0 + nx <= NX):
        raise ValueError('section outside the frame')
    check(lib.bbx_rect_scale(ctx.h, ny, nx, NX, C.c_void_p(t.data_ptr() + 4 * (y0 * NX + x0)), C.c_float(float(factor)),
                             1 if divide else 0, ctx.stream()), 'bbx_rect_scale', ctx.h)


def gain_correction_factors(ctx, master, header, ysize_chan=None, xsize_chan=None, nrows_v=200, nrows_h=2000,
                            ncols=200):
    """GAINCF{c} of a master flat (blackbox.py:5085-5161): match the channels vertically
    with the medians of the [nrows_v] rows next to the central row boundary, then
    horizontally, pair of channel columns by pair, with the medians of [ncols] columns
    either side of each boundary over 2*[nrows_h] central rows; factors normalised to a
    mean of one.  Medians are exact (bbx_rect_stats); the frame copy is scaled channel by
    channel on the device (float32, like numpy's in-place ops on the float32 master)."""
    import numpy as np
    from . import flatstats
    NY, NX = master.shape
    ysz, xsz = ysize_chan or NY // 2, xsize_chan or NX // 8
    def pyslice(start, stop, n):
        """[start:stop] of an axis of length n with Python's rules (the reference slices numpy arrays
        with these numbers; strips larger than the frame are clamped, a negative start wraps once)"""
        a, b, _ = slice(start, stop).indices(n)
        if b <= a:
            raise ValueError('empty statistics strip [{}:{}] on an axis of {}'.format(start, stop, n))
        return a, b - a
    corr = master.clone()
    med = np.zeros(16)
    for c in range(16):
        iy, ix = divmod(c, 8)
        ya, nr = pyslice(-nrows_v, None, ysz) if iy == 0 else pyslice(0, nrows_v, ysz)      # data_chan[-nrows:, :] / [0:nrows, :]
        med[c] = np.float32(flatstats.rect_stats(ctx, corr, None, iy * ysz + ya, ix * xsz, nr, xsz, nr, xsz)[0, 1])
        _rect_scale(ctx, corr, iy * ysz, ix * xsz, ysz, xsz, med[c], True)
    factor = 1.0 / med
    for i in range(1, 8):
        x_index = i * xsz
        ya, nr = pyslice(ysz - nrows_h, ysz + nrows_h, NY)
        xa, nc1 = pyslice(x_index - ncols, x_index, NX)
        xb, nc2 = pyslice(x_index, x_index + ncols, NX)
        m1 = np.float32(flatstats.rect_stats(ctx, corr, None, ya, xa, nr, nc1, nr, nc1)[0, 1])
        m2 = np.float32(flatstats.rect_stats(ctx, corr, None, ya, xb, nr, nc2, nr, nc2)[0, 1])
        ratio = np.float32(m1) / np.float32(m2)
        _rect_scale(ctx, corr, 0, i * xsz, ysz, xsz, ratio, False)
        _rect_scale(ctx, corr, ysz, i * xsz, ysz, xsz, ratio, False)
        factor[i] *= ratio
        factor[i + 8] *= ratio
    factor /= np.mean(factor)
    for c in range(16):
        header['GAINCF{}'.format(c + 1)] = (float(factor[c]), 'channel {} gain correction factor'.format(c + 1))
    return factor


def master_level_stats(ctx, master, header, imgtype, ysize_chan=None, xsize_chan=None):
    """header statistics of a master bias / dark (blackbox.py:5167-5230): sigma-clipped mean
    and sigma of the frame and of each channel, zeros masked.  Keywords MBMEAN MBRDN
    MBIASM{c} MBRDN{c} (bias) or MDMEAN MDRDN MDARKM{c} MDRDN{c} (dark)."""
    from . import flatstats
    NY, NX = master.shape
    ysz, xsz = ysize_chan or NY // 2, xsize_chan or NX // 8
    full = flatstats.rect_clipped_stats(ctx, master, None, 0, 0, NY, NX, NY, NX)[0]
    chan = flatstats.rect_clipped_stats(ctx, master, None, 0, 0, NY, NX, ysz, xsz)
    if imgtype == 'bias':
        k = ('MBMEAN', 'MBRDN', 'MBIASM{}', 'MBRDN{}', 'bias')
    elif imgtype == 'dark':
        k = ('MDMEAN', 'MDRDN', 'MDARKM{}', 'MDRDN{}', 'dark')
    else:
        raise ValueError('bias or dark expected')
    header[k[0]] = (float(full[2]), '[e-] mean master {}'.format(k[4]))
    header[k[1]] = (float(full[3]), '[e-] sigma (STD) master {}'.format(k[4]))
    for c in range(16):
        header[k[2].format(c + 1)] = (float(chan[c, 2]), '[e-] channel {} mean master {}'.format(c + 1, k[4]))
    for c in range(16):
        header[k[3].format(c + 1)] = (float(chan[c, 3]), '[e-] channel {} sigma (STD) master {}'.format(c + 1, k[4]))
    return full, chan


def flat_fix(ctx, master, bpm):
    """the master flat's edge / non-positive fix (5071-5073), in place: pixels that are BPM-edge (32) or <= 0 become 1.
    bbx_median_stack over the one frame (the median of one value is that value), so that the statistics the reference
    takes before the fix (MFMEDSEC ... MFSTD) can be taken in between"""
    if bpm.dtype != torch.uint8 or tuple(bpm.shape) != tuple(master.shape) or not bpm.is_contiguous():
        raise ValueError('bad-pixel mask: contiguous uint8 of the master\'s shape {} expected'.format(tuple(master.shape)))
    ptrs = (C.c_void_p * 1)(master.data_ptr())
    check(lib.bbx_median_stack(ctx.h, master.numel(), 1, ptrs, None, C.c_void_p(bpm.data_ptr()), 1,
                               C.c_void_p(master.data_ptr()), ctx.stream()), 'bbx_median_stack', ctx.h)


# ---- dates: astropy's Time restated on datetime (UTC; every day 86400 s) -------------------------------------
_MJD0 = datetime.datetime(1858, 11, 17)


def _mjd(dt):
    d = dt - _MJD0
    return d.days + (d.seconds + d.microseconds / 1e6) / 86400.0


def isot2mjd(s):
    """MJD of an ISO date 'yyyy-mm-dd[Thh:mm[:ss[.s]]]' (a space for the T accepted), e.g. DATE-OBS:
    Time(s, format='isot').mjd"""
    date, _, tm = str(s).strip().replace(' ', 'T').partition('T')
    y, m, d = (int(v) for v in date.split('-'))
    dt = datetime.datetime(y, m, d)
    if tm:
        p = tm.split(':')
        dt += datetime.timedelta(hours=int(p[0]), minutes=int(p[1]) if len(p) > 1 and p[1] else 0,
                                 seconds=float(p[2]) if len(p) > 2 and p[2] else 0.0)
    return _mjd(dt)


def date2mjd(date_str, time_str=None):
    """blackbox.py:5416-5441: MJD of [date_str] (yyyymmdd or yyyy-mm-dd) at [time_str] (hhmmss[.s] or hh:mm[:ss.s])"""
    date_str = str(date_str)
    if '-' not in date_str:
        date_str = '{}-{}-{}'.format(date_str[0:4], date_str[4:6], date_str[6:8])
    if time_str is not None:
        if ':' not in time_str:
            time_str = '{}:{}:{}'.format(time_str[0:2], time_str[2:4], time_str[4:])
        date_str = '{}T{}'.format(date_str, time_str)
    return isot2mjd(date_str)


def _day_path(mjd):
    """'yyyy/mm/dd' of the UTC day of [mjd] (Time(mjd, format='mjd').isot's date with slashes)"""
    return (_MJD0 + datetime.timedelta(days=float(mjd))).strftime('%Y/%m/%d')


def delta_one_month(date_eve, dmonth):
    """blackbox.py:5252-5286: 'yyyy/mm/' of the month before (-1), of (0) or after (+1) the evening date"""
    date_eve = ''.join(e for e in str(date_eve) if e.isdigit())
    if dmonth == 0:
        mjd_noon = date2mjd(date_eve, '12:00')
    elif dmonth == -1:
        mjd_noon = date2mjd(date_eve, '12:00') - (int(date_eve[6:8]) + 1)
    elif dmonth == 1:
        year, month = int(date_eve[0:4]), int(date_eve[4:6])
        year, month = (year + 1, 1) if month == 12 else (year, month + 1)
        mjd_noon = date2mjd('{}{:02}{:02}'.format(year, month, 1), '12:00')
    else:
        raise ValueError('maximum [dmonth] in [delta_one_month] is 1')
    return _day_path(mjd_noon)[0:8]


def haversine(ra1, dec1, ra2, dec2):
    """angular distance [deg] between two positions given in degrees (zogy.haversine)"""
    ra1, dec1, ra2, dec2 = (np.radians(np.asarray(a, dtype=float)) for a in (ra1, dec1, ra2, dec2))
    a = np.sin((dec2 - dec1) / 2) ** 2 + np.cos(dec1) * np.cos(dec2) * np.sin((ra2 - ra1) / 2) ** 2
    return np.degrees(2 * np.arcsin(np.sqrt(a)))


# ---- files ----------------------------------------------------------------------------------------------------
def _hv(h, key, default=None):
    v = h.get(key, default)
    return v[0] if isinstance(v, tuple) else v


def already_exists(filename, get_filename=False):
    """blackbox.py:787-805: [filename], or its .fz / .gz twin, is a file (first of those found)"""
    found = None
    for f in (filename, filename + '.fz', filename + '.gz', filename.replace('.fz', ''), filename.replace('.gz', '')):
        if os.path.isfile(f):
            found = f
            break
    if get_filename:
        return found is not None, (found or filename)
    return found is not None


def read_header(path):
    """the header of a frame without its data (read_hdulist(get_data=False)): the compressed image's header of a
    tile-compressed file, else the primary header"""
    from . import fitsio
    hdus = fitsio.read_hdus(path, headers_only=True)
    for h, _ in hdus:
        if _hv(h, 'ZIMAGE', False) is True:
            return h
    return hdus[0][0]


def qc_flagged(fits_name, flag='red'):
    """blackbox.py:5403-5412: the header's QC-FLAG is [flag]"""
    h = read_header(fits_name)
    return 'QC-FLAG' in h and _hv(h, 'QC-FLAG') == flag


class _Lock:
    """exclusive flock on <master>.lock: check -> build -> write of one master by one process at a time (the reference
    serialises master_prep with a process lock); the lock file stays"""

    def __init__(self, fits_master):
        os.makedirs(os.path.dirname(os.path.abspath(fits_master)), exist_ok=True)
        self.path = fits_master + '.lock'

    def __enter__(self):
        import fcntl
        self.f = open(self.path, 'a')
        fcntl.flock(self.f, fcntl.LOCK_EX)
        return self

    def __exit__(self, *exc):
        import fcntl
        fcntl.flock(self.f, fcntl.LOCK_UN)
        self.f.close()
        return False


# ---- selection (blackbox.py:4700-4890) ----------------------------------------------------------------------------
MJD_AVOID = ('2019-07-01T12:00:00', '2020-03-01T12:00:00')     # ML1 evening frames in this period: dome vignetting


def list_cal_files(red_dir, tel, imgtype, date_eve, filt=None, nwindow=None):
    """reduced calibration frames of [imgtype] in <red_dir>/<yyyy/mm/dd>/<imgtype>/ for the evening dates within
    +- [nwindow] (cal_window) days: names starting with <tel>_20 that contain '.fits' (flats: '<filt>.fits'), sorted.
    A frame present both as .fits and .fits.fz is listed once, as the .fz file (the reference lists -- and stacks --
    both)."""
    if nwindow is None:
        nwindow = int(get_par(settings.cal_window, tel)[imgtype])
    search = '{}.fits'.format(filt) if imgtype == 'flat' else '.fits'
    mjd_noon = date2mjd(date_eve, '12:00')
    found = []
    for n_day in range(-nwindow, nwindow + 1):
        d = os.path.join(red_dir, _day_path(mjd_noon + n_day), imgtype)
        try:
            names = os.listdir(d)
        except OSError:
            continue
        found += [os.path.join(d, n) for n in names
                  if n.startswith('{}_20'.format(tel)) and search in n and os.path.isfile(os.path.join(d, n))]
    frames = {}
    for f in sorted(found):
        key = f[:-3] if f.endswith('.fz') else f
        if key not in frames or f.endswith('.fz'):
            frames[key] = f
    return sorted(frames.values())


def select_frames(red_dir, tel, imgtype, date_eve, filt=None, create_master=True):
    """the frames master_prep would stack (4700-4890); only headers are read.
    -> dict(files, headers, mjd_obs: of the files, nearest to 23:59 UT of the evening date first; nwindow; nfound: files
    listed; nkept: after the flag / date rules; skip: None, 'few' (fewer than 5 frames) or 'old' (all from before that
    midnight, the nearest more than 0.5 d away)).  With create_master False nothing is read (the reference reads no
    header then either) and the listed files are returned."""
    nwindow = int(get_par(settings.cal_window, tel)[imgtype])
    files = list_cal_files(red_dir, tel, imgtype, date_eve, filt, nwindow)
    sel = dict(files=files, headers=[], mjd_obs=np.zeros(len(files)), nwindow=nwindow, nfound=len(files),
               nkept=len(files), skip=None)
    if not create_master:
        sel['skip'] = 'few' if len(files) < 5 else None
        return sel
    mjd_avoid = [isot2mjd(s) for s in MJD_AVOID]
    reject_eve = imgtype == 'flat' and bool(get_par(settings.flat_reject_eve, tel))
    headers, mjd_obs, keep = [], np.zeros(len(files)), np.ones(len(files), dtype=bool)
    for i, f in enumerate(files):
        h = read_header(f)
        headers.append(h)
        if 'QC-FLAG' in h and _hv(h, 'QC-FLAG') == 'red':
            keep[i] = False
        if 'MJD-OBS' in h:
            mjd_obs[i] = float(_hv(h, 'MJD-OBS'))
        if tel == 'ML1' and mjd_obs[i] % 1 > 0.5 and mjd_avoid[0] < mjd_obs[i] < mjd_avoid[1]:
            keep[i] = False
        if reject_eve and (mjd_obs[i] % 1 > 0.5 or mjd_obs[i] % 1 < 0.1):
            log.warning('rejecting evening flat %s', f)
            keep[i] = False
    idx = np.nonzero(keep)[0]
    sel['nkept'] = len(idx)
    if len(idx) < 5:
        sel.update(files=[files[i] for i in idx], headers=[headers[i] for i in idx], mjd_obs=mjd_obs[idx], skip='few')
        return sel
    nmax = int(get_par(settings.ncal_max, tel)[imgtype])
    delta = mjd_obs[idx] - date2mjd(date_eve, '23:59')
    order = idx[np.argsort(np.abs(delta), kind='stable')][:nmax]
    sel.update(files=[files[i] for i in order], headers=[headers[i] for i in order], mjd_obs=mjd_obs[order])
    delta = sel['mjd_obs'] - date2mjd(date_eve, '23:59')
    if np.amin(np.abs(delta)) > 0.5 and np.all(delta < 0):
        sel['skip'] = 'old'
    return sel


def get_nearest_master(date_eve, imgtype, fits_master, filt=None, master_dir=None, tel=None):
    """blackbox.py:5291-5391: yesterday's master if it exists and is not red-flagged, else the non-red .fits.fz master
    of [imgtype] (flats: of [filt]) nearest in date over the previous, current and next month under [master_dir]
    (<master_dir>/<yyyy/mm/dd>/<imgtype>/<tel>_<imgtype>_...); None if there is none"""
    tel = tel or os.path.basename(fits_master).split('_')[0]
    master_dir = master_dir or _master_root(fits_master)
    day = datetime.date(int(date_eve[0:4]), int(date_eve[4:6]), int(date_eve[6:8]))
    yest = day - datetime.timedelta(days=1)
    fits_yest = (fits_master.replace(date_eve, yest.strftime('%Y%m%d'))
                 .replace(day.strftime('%Y/%m/%d'), yest.strftime('%Y/%m/%d')))
    present, found = already_exists(fits_yest, get_filename=True)
    if present and not qc_flagged(found):
        return found
    start = '{}_{}_'.format(tel, imgtype)
    end = '{}.fits.fz'.format(filt) if imgtype == 'flat' else '.fits.fz'
    file_list = []
    for n_month in (-1, 0, 1):
        for root, _, names in os.walk(os.path.join(master_dir, delta_one_month(date_eve, n_month))):
            file_list += [os.path.join(root, n) for n in names if n.startswith(start) and n.endswith(end)]
    cand = []
    for f in sorted(file_list):
        parts = os.path.normpath(f).split(os.sep)
        try:
            cand.append((f, date2mjd(''.join(parts[-5:-2]))))
        except ValueError:
            continue                                     # not in a yyyy/mm/dd/<imgtype> folder
    if not cand:
        return None
    delta = np.abs(np.array([m for _, m in cand]) - date2mjd(date_eve))
    for i in np.argsort(delta, kind='stable'):
        if not qc_flagged(cand[i][0]):
            return cand[i][0]
    return None


def _master_root(fits_master):
    """<master_dir> of <master_dir>/<yyyy/mm/dd>/<imgtype>/<name>"""
    d = os.path.dirname(os.path.abspath(fits_master))
    for _ in range(4):
        d = os.path.dirname(d)
    return d


# ---- the data path ------------------------------------------------------------------------------------------------
def _read_host(path):
    """the host half of reading a frame (reader threads): the file's bytes, parsed, no GPU call"""
    from . import fitsio, fpack
    if path.endswith('.fz'):
        return 'fz', fpack.funpack_read(path)
    got = fitsio.read_image_file_order(path)
    if got is not None and got[0].dtype == np.dtype('>f4'):
        return 'be32', got[0]
    return 'host', np.ascontiguousarray(fitsio.read_image(path, dtype=np.float32))


def _to_device(ctx, kind, data):
    """the device half: float32 words put into host order on the device (bbx_be32), or the tiles decoded there"""
    from . import fpack
    from .reduce import _ptr
    if kind == 'fz':
        t, _ = fpack.funpack_decode(ctx, data)
        return t if t.dtype == torch.float32 else t.to(torch.float32)
    if kind == 'be32':
        t = torch.from_numpy(data.view(np.int32)).to(ctx.device)          # (the bytes; int32 is only the carrier)
        check(lib.bbx_be32(_ptr(t), _ptr(t), t.numel(), ctx.stream()), 'bbx_be32')
        return t.view(torch.float32)
    return torch.from_numpy(data).to(ctx.device)


def load_frames(ctx, files, shape=None, timing=None):
    """the frames as float32 device tensors, in the order of [files].  Reader threads (as many as pipeline.cpu_budget()
    allows, at most 8, a few files ahead) read and parse the files while this thread puts each one on the device as it
    arrives (.fits float32: bytes up + bbx_be32; .fits.fz: bbx_funpack_tiles).  A frame whose shape is not [shape]
    raises ValueError.  timing: dict that gets 'read' (waiting for the readers) and 'decode' seconds added"""
    from concurrent.futures import ThreadPoolExecutor
    from . import pipeline
    timing = {} if timing is None else timing
    nthreads = max(1, min(len(files), 8, pipeline.cpu_budget() // 2))
    ahead = nthreads + 2                                  # parsed files waiting in host memory at most
    out = []
    with ThreadPoolExecutor(nthreads, thread_name_prefix='bbx-master-read') as pool:
        futs = [pool.submit(_read_host, f) for f in files[:ahead]]
        try:
            for i, f in enumerate(files):
                t0 = time.time()
                kind, data = futs[i].result()
                futs[i] = None
                if i + ahead < len(files):
                    futs.append(pool.submit(_read_host, files[i + ahead]))
                t1 = time.time()
                t = _to_device(ctx, kind, data)
                del data
                timing['read'] = timing.get('read', 0.0) + (t1 - t0)
                timing['decode'] = timing.get('decode', 0.0) + (time.time() - t1)
                if shape is not None and tuple(t.shape) != tuple(shape):
                    raise ValueError('{}: frame of {} pixels, the master is {}'.format(f, tuple(t.shape), tuple(shape)))
                out.append(t)
        except BaseException:
            for fu in futs:
                if fu is not None:
                    fu.cancel()
            raise
    t0 = time.time()
    ctx.sync()
    timing['decode'] = timing.get('decode', 0.0) + (time.time() - t0)
    return out


def frame_medsec(ctx, frame, statsec):
    """np.median of a reduced flat over the normalisation section (4933-4935), when its header has no MEDSEC"""
    from . import flatstats
    y, x = statsec
    h, w = y.stop - y.start, x.stop - x.start
    return float(np.float32(flatstats.rect_stats(ctx, frame, None, y.start, x.start, h, w, h, w)[0, 1]))


def dither_offsets(ra, dec):
    """5025-5047: offsets [arcsec] of each flat from the previous one (the first from the last) -> (number of offsets
    of at least 5 arcsec, their mean or 0)"""
    ra, dec = np.asarray(ra, dtype=float), np.asarray(dec, dtype=float)
    noffset, offset_mean = 0, 0
    if len(ra) > 0 and len(dec) > 0:
        offset = 3600. * haversine(ra, dec, np.roll(ra, 1), np.roll(dec, 1))
        mask_off = offset >= 5
        noffset = int(np.sum(mask_off))
        if noffset > 0:
            offset_mean = float(np.mean(offset[mask_off]))
    return noffset, offset_mean


def flat_statistics(ctx, master, header, statsec, nfiles, ra=(), dec=()):
    """header keywords of a master flat before its edge fix (4998-5053): STATSEC, MFMEDSEC, MFSTDSEC (over STATSEC),
    MFMED, MFSTD (sigma-clipped over all non-zero pixels), N-OFFSET, OFF-MEAN, FLATDITH"""
    from . import flatstats
    y, x = statsec
    header['STATSEC'] = ('[{}:{},{}:{}]'.format(y.start + 1, y.stop + 1, x.start + 1, x.stop + 1),
                         'pre-defined statistics section [y1:y2,x1:x2]')
    h, w = y.stop - y.start, x.stop - x.start
    st = flatstats.rect_stats(ctx, master, None, y.start, x.start, h, w, h, w)[0]
    header['MFMEDSEC'] = (float(np.float32(st[1])), 'median master flat over STATSEC')
    header['MFSTDSEC'] = (float(np.float32(st[3])), 'sigma (STD) master flat over STATSEC')
    NY, NX = master.shape
    st = flatstats.rect_clipped_stats(ctx, master, None, 0, 0, NY, NX, NY, NX)[0]
    header['MFMED'] = (float(st[1]), 'median master flat')
    header['MFSTD'] = (float(st[3]), 'sigma (STD) master flat')
    dither_keywords(header, ra, dec, nfiles)


def dither_keywords(header, ra, dec, nfiles):
    """N-OFFSET, OFF-MEAN and FLATDITH (two thirds of the [nfiles] flats offset) of a master flat (5040-5053)"""
    noffset, offset_mean = dither_offsets(ra, dec)
    header['N-OFFSET'] = (noffset, 'number of flats with offsets > 5 arcsec')
    header['OFF-MEAN'] = (offset_mean, '[arcsec] mean dithering offset')
    header['FLATDITH'] = (float(noffset) / nfiles >= 0.66, 'majority of flats were dithered')
    return header


def flat_bpm_path(bpm, filt):
    """the filter's bad-pixel mask: 'bpm' -> 'bpm_<filt>' in the base name of [bpm], .fz twin accepted (5059-5062)"""
    if not bpm:
        return None
    d, b = os.path.split(bpm)
    present, f = already_exists(os.path.join(d, b.replace('bpm', 'bpm_{}'.format(filt))), get_filename=True)
    return f if present else None


FIRST_KEYS = ('IMAGETYP', 'DATE-OBS', 'FILTER', 'RA', 'DEC', 'XBINNING', 'YBINNING', 'MJD-OBS', 'AIRMASS', 'ORIGIN',
              'TELESCOP', 'PYTHON-V', 'BB-V')


def _float(v):
    try:
        return float(v)
    except (TypeError, ValueError):
        return None


def build_master(ctx, sel, imgtype, tel, data_shape, filt=None, bpm=None, statsec=None, ysize_chan=None,
                 xsize_chan=None, timing=None):
    """4906-5235 on the device for the selected frames (select_frames) -> (master float32 device tensor, header dict
    in the reference's order, without DATEFILE)"""
    from . import qc, reduce as R
    timing = {} if timing is None else timing
    files, headers = sel['files'], sel['headers']
    nfiles = len(files)
    statsec = statsec or get_par(settings.flat_norm_sec, tel)
    frames = load_frames(ctx, files, data_shape, timing)
    t0 = time.time()
    header, medsec, ra, dec = {}, [], [], []
    for i, (f, h) in enumerate(zip(files, headers)):
        if imgtype == 'flat':
            median = _float(_hv(h, 'MEDSEC')) if 'MEDSEC' in h else None
            if median is None:
                median = frame_medsec(ctx, frames[i], statsec)
            log.info('flat name: %s, median: %.1f e-', f, median)
            medsec.append(median)
            if 'RA' in h and 'DEC' in h:
                ra.append(float(_hv(h, 'RA')))
                dec.append(float(_hv(h, 'DEC')))
        if i == 0:
            for key in FIRST_KEYS:
                if key in h:
                    header[key] = h[key]
        comment = 'name reduced flat' if imgtype == 'flat' else 'name gain/os-corrected {} frame'.format(imgtype)
        header['{}{}'.format(imgtype.upper(), i + 1)] = (os.path.basename(f).split('.fits')[0], '{} {}'.format(comment, i + 1))
        if 'ORIGFILE' in h:
            header['{}OR{}'.format(imgtype.upper(), i + 1)] = (_hv(h, 'ORIGFILE'), 'name original {} {}'.format(imgtype, i + 1))
        if i == nfiles - 1:
            for key in ('DATE-END', 'MJD-END'):
                if key in h:
                    header[key] = h[key]
    master = master_median(ctx, frames, imgtype, medsec=medsec if imgtype == 'flat' else None)
    ctx.sync()
    del frames                                            # the stack's inputs go back to the allocator here
    t1 = time.time()
    timing['stack'] = timing.get('stack', 0.0) + (t1 - t0)
    header['N{}'.format(imgtype.upper())] = (nfiles, 'number of {} frames combined'.format(imgtype.lower()))
    header['{}-WIN'.format(imgtype.upper())] = (sel['nwindow'], '[days] input time window to include {} frames'
                                                .format(imgtype.lower()))
    ysz, xsz = ysize_chan or data_shape[0] // 2, xsize_chan or data_shape[1] // 8
    if imgtype == 'flat':
        flat_statistics(ctx, master, header, statsec, nfiles, ra, dec)
        fits_bpm = flat_bpm_path(bpm, filt)
        if fits_bpm is not None:
            flat_fix(ctx, master, R.image_to_device(ctx, fits_bpm, np.uint8))
        gain_correction_factors(ctx, master, header, ysize_chan=ysz, xsize_chan=xsz)
    else:
        master_level_stats(ctx, master, header, imgtype, ysize_chan=ysz, xsize_chan=xsz)
    ctx.sync()
    timing['statistics'] = timing.get('statistics', 0.0) + (time.time() - t1)
    qc.run_qc_check(header, tel)
    return master, header


def write_master(ctx, fits_master, master, header, fpack=False):
    """the master as <fits_master> (float32) or, with [fpack], <fits_master>.fz (quantisation 16, compressed on the
    device): written under a temporary name in the same folder and renamed, so that no reader sees half a file"""
    from . import fitsio, fpack as P
    d, name = os.path.split(os.path.abspath(fits_master))
    final = fits_master + '.fz' if fpack else fits_master
    tmp = os.path.join(d, '.{}.{}.tmp{}'.format(name, os.getpid(), '.fz' if fpack else ''))
    header['DATEFILE'] = (datetime.datetime.now(datetime.timezone.utc).replace(tzinfo=None).isoformat(timespec='milliseconds'),
                          'UTC date of writing file')
    try:
        if fpack:
            P.fpack_image(ctx, tmp, master, header, quant=16)
        else:
            fitsio.write_image(tmp, master.cpu().numpy(), header)
        os.replace(tmp, final)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return final


def master_prep(fits_master, data_shape, create_master, pick_alt=True, tel=None, red_dir=None, master_dir=None,
                ctx=None, bpm=None, flat_norm_sec=None, ysize_chan=None, xsize_chan=None, fpack=False, timing=None):
    """blackbox.py:4625-5247: the master <master_dir>/<yyyy/mm/dd>/<imgtype>/<tel>_<imgtype>_<date>[_<filt>].fits
    [fits_master] of shape [data_shape] -> its path (.fits or .fits.fz), or None.

    An existing master that is not red-flagged is returned as it is.  Otherwise, with [create_master], one is made from
    the reduced frames under [red_dir] (select_frames), written (write_master: .fits.fz with [fpack]) and returned.
    With too few frames, or without [create_master], a nearby master (get_nearest_master) is returned if [pick_alt],
    else None; None too when all frames are old.  An existing red master is made again (the reference searches for a
    nearby one instead).  The check, the build and the write hold <fits_master>.lock.
    bpm: path of the bad-pixel mask ('bpm' -> 'bpm_<filt>', flats only); flat_norm_sec: (slice, slice) of the flat
    normalisation / STATSEC (default settings.flat_norm_sec); timing: dict of seconds per phase (header_scan, read,
    decode, stack, statistics, write).  Errors (unreadable or wrong-shaped frames, ...) raise."""
    timing = {} if timing is None else timing
    tel = tel or os.path.basename(fits_master).split('_')[0]
    if not red_dir:
        raise ValueError('master_prep needs red_dir, the root of the reduced calibration frames')
    master_dir = master_dir or _master_root(fits_master)
    filename = os.path.basename(fits_master)
    imgtype, date_eve = filename.split('.fits')[0].split('{}_'.format(tel))[-1].split('_')[0:2]
    filt = filename.split('.fits')[0].split('_')[-1] if imgtype == 'flat' else None
    msg = 'flat in filter {}'.format(filt) if imgtype == 'flat' else imgtype
    with _Lock(fits_master):
        present, existing = already_exists(fits_master, get_filename=True)
        master_ok = True
        if present:
            log.info('master %s %s exists', imgtype, existing)
            if qc_flagged(existing):
                master_ok = False
                log.warning('existing master %s %s contains a red flag; making it again', imgtype, existing)
        if present and master_ok:
            return existing
        t0 = time.time()
        sel = select_frames(red_dir, tel, imgtype, date_eve, filt, create_master)
        timing['header_scan'] = timing.get('header_scan', 0.0) + (time.time() - t0)
        if sel['skip'] == 'few' or not create_master:
            if pick_alt or not create_master:
                near = get_nearest_master(date_eve, imgtype, fits_master, filt=filt, master_dir=master_dir, tel=tel)
                if near is not None:
                    log.warning('using %s as master for evening date %s', near, date_eve)
                else:
                    log.error('no alternative master %s found', msg)
                return near
            log.warning('too few good frames available to produce master %s for evening date %s +/- window of %d days',
                        msg, date_eve, sel['nwindow'])
            return None
        if sel['skip'] == 'old':
            log.warning('all selected calibration files closest in time to midnight of %s are from before this date and '
                        'taken longer than 12 hours ago; no point in making master %s', date_eve, fits_master)
            return None
        log.info('making %s master %s for night %s from the following files:\n%s', tel, msg, date_eve, sel['files'])
        if sel['nkept'] > len(sel['files']):
            log.warning('number of available %s frames (%d) exceeds the maximum specified (%d); using the frames closest '
                        'in time to midnight of the evening date (%s)', imgtype, sel['nkept'], len(sel['files']), date_eve)
        ctx = ctx or _process_ctx()
        master, header = build_master(ctx, sel, imgtype, tel, data_shape, filt=filt, bpm=bpm, statsec=flat_norm_sec,
                                      ysize_chan=ysize_chan, xsize_chan=xsize_chan, timing=timing)
        t0 = time.time()
        written = write_master(ctx, fits_master, master, header, fpack=fpack)
        del master
        if present and os.path.abspath(existing) != os.path.abspath(written):
            os.remove(existing)                           # the red master this one replaces, kept in the other form
        timing['write'] = timing.get('write', 0.0) + (time.time() - t0)
        return written


_CTX = {}


def _process_ctx():
    """this process's GPU context for masters made without one (create_masters' pool workers): device LOCAL_RANK"""
    if 'ctx' not in _CTX:
        from . import farm, reduce as R
        _CTX['ctx'] = R.Context(farm.rank_world()[2])
    return _CTX['ctx']


# ---- the night's masters (blackbox.py:617-782) ------------------------------------------------------------------
IMGTYPES = ('bias', 'dark', 'flat')
FILTERS = 'ugqriz'         # set_zogy.zp_default's filters (that settings module is not part of the reference tree)


def master_dates(master_date):
    """[master_date]: an evening date yyyymmdd, or a text file with one evening date per line and optionally a second
    column of filters (flats) -> [(yyyymmdd, filters or None)].  Anything else raises ValueError."""
    def _date(d, what):
        if len(d) != 8 or not d.isdigit():
            raise ValueError('{}: evening date yyyymmdd expected, got {!r}'.format(what, d))
        datetime.datetime.strptime(d, '%Y%m%d')
        return d
    if master_date is None:
        raise ValueError('master_date required')
    if os.path.isfile(master_date):
        out = []
        with open(master_date) as f:
            for ln in f:
                cols = ln.split('#')[0].split()
                if not cols:
                    continue
                out.append((_date(''.join(e for e in cols[0] if e.isdigit()), master_date), cols[1] if len(cols) > 1 else None))
        return out
    return [(_date(str(master_date), 'master_date (an evening date yyyymmdd or a file of them)'), None)]


def list_masters(master_date, master_dir, tel, imgtypes=None, filters=None):
    """the masters create_masters makes: <master_dir>/<yyyy/mm/dd>/<imgtype>/<tel>_<imgtype>_<date>[_<filt>].fits for
    every evening date of [master_date], every type of [imgtypes] ('bias,flat'; default all three) and, for flats, every
    filter of [filters] (default u g q r i z) or of the date's second column"""
    import re
    types = list(IMGTYPES)
    if imgtypes:
        asked = [t for t in re.split(r'[,\s]+', imgtypes.lower()) if t]
        for t in asked:
            if t not in IMGTYPES:
                log.warning('--imgtypes %s: masters exist for %s only', t, ', '.join(IMGTYPES))
        types = [t for t in IMGTYPES if t in asked]
    filts = re.sub(r',|-|\.|/|\s', '', filters) if filters else FILTERS
    out = []
    for date_eve, fcol in master_dates(master_date):
        path = os.path.join(master_dir, date_eve[0:4], date_eve[4:6], date_eve[6:8])
        for imgtype in types:
            if imgtype != 'flat':
                out.append(os.path.join(path, imgtype, '{}_{}_{}.fits'.format(tel, imgtype, date_eve)))
                continue
            for filt in ([f for f in fcol if f in filts] if fcol is not None else filts):
                out.append(os.path.join(path, 'flat', '{}_flat_{}_{}.fits'.format(tel, date_eve, filt)))
    return out


def make_master(fits_master, opts, ctx=None, timing=None):
    """one master of create_masters: master_prep(create_master=True, pick_alt=False) with its failure caught and logged
    -> (fits_master, path or None, None or the error).  Module level: spawned pool workers run it with their own GPU
    context."""
    try:
        return fits_master, master_prep(fits_master, opts['data_shape'], True, pick_alt=False, ctx=ctx, timing=timing,
                                        **{k: v for k, v in opts.items() if k != 'data_shape'}), None
    except Exception as e:
        log.exception('making master %s failed', fits_master)
        return fits_master, None, '{}: {}'.format(type(e).__name__, e)


def create_masters(master_date, red_dir, master_dir, tel='ML1', ctx=None, imgtypes=None, filters=None, bpm=None,
                   flat_norm_sec=None, ysize_chan=None, xsize_chan=None, fpack=False, pool=None, timing=None):
    """blackbox.py:617-782: the bias / dark / flat masters of the evening date(s) [master_date] (master_dates) under
    [master_dir] from the reduced frames under [red_dir] (list_masters, master_prep).  A master that fails is logged
    and the others go on.  pool: callable(func, items) -> results that maps make_master over the masters (the command
    line's spawn pool), else they are made one after the other on [ctx].
    -> [(fits_master, path written or found, or None; None or the error of a master that failed)]"""
    import functools
    ysz = ysize_chan or settings.ysize_chan
    xsz = xsize_chan or settings.xsize_chan
    opts = dict(data_shape=(settings.ny * ysz, settings.nx * xsz), tel=tel, red_dir=red_dir, master_dir=master_dir,
                bpm=bpm, flat_norm_sec=flat_norm_sec, ysize_chan=ysz, xsize_chan=xsz, fpack=fpack)
    names = list_masters(master_date, master_dir, tel, imgtypes, filters)
    log.info('list_masters: %s', names)
    if pool is not None:
        return pool(functools.partial(make_master, opts=opts), names)
    return [make_master(n, opts, ctx=ctx, timing=timing) for n in names]
