"""Files-to-master timing of create_masters at full size (10560 x 10560 ML1 frames).

    python tools/master_bench.py [--tag TAG] [--scratch DIR] [--nbias 20] [--nflat 15] [--repeat 2]

Untimed: [nbias] bias and [nflat] q-band flat frames are synthesised on the GPU and written as .fits.fz
(quantisation 16, like the reduced frames the reference keeps) under <scratch>/red/2024/01/05/{bias,flat}/,
with a full-size bpm_q.fits.  Timed: masters.create_masters for the bias master and for the flat master, each
into a fresh master folder -- with a cold page cache (the input files dropped with posix_fadvise after an fsync,
as far as the kernel honours it) and then warm, [repeat] times.  Per master the wall time is split into header
scan / read (waiting for the reader threads) / decode / stack / statistics / write (masters.master_prep's timing).
Writes profiles/<tag>_masters.json (and prints it) with the peak HBM held by tensors."""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from blackbox_amd import fitsio, fpack as P, masters as M, pipeline, settings   # noqa: E402
from blackbox_amd import reduce as R                                          # noqa: E402


def synthesise(ctx, red, root, nbias, nflat):
    ny, nx = settings.ny * settings.ysize_chan, settings.nx * settings.xsize_chan
    g = torch.Generator(device=ctx.device)
    g.manual_seed(7)
    chan = ((torch.arange(nx, device=ctx.device) // settings.xsize_chan)[None, :]
            + 8 * (torch.arange(ny, device=ctx.device) // settings.ysize_chan)[:, None]).float()
    files = []
    for imgtype, n in (('bias', nbias), ('flat', nflat)):
        d = os.path.join(red, '2024', '01', '05', imgtype)
        os.makedirs(d, exist_ok=True)
        for k in range(n):
            if imgtype == 'bias':
                img = 3.0 * torch.randn((ny, nx), generator=g, device=ctx.device) + 0.2 * chan
            else:
                img = (20000.0 + 700.0 * k) * (1.0 + 0.02 * torch.randn((ny, nx), generator=g, device=ctx.device)) \
                    * (1.0 + 0.004 * chan)
            img = img.contiguous()
            date_obs = '2024-01-06T0{}:{:02d}:00'.format(3 + k // 60, k % 60)
            h = {'IMAGETYP': imgtype, 'FILTER': 'q', 'QC-FLAG': 'green', 'DATE-OBS': date_obs,
                 'MJD-OBS': M.isot2mjd(date_obs), 'RA': 150.0 + 0.01 * k, 'DEC': -30.0}
            if imgtype == 'flat':
                h['MEDSEC'] = M.frame_medsec(ctx, img, settings.flat_norm_sec['ML1'])
            name = os.path.join(d, 'ML1_20240106_{}{}.fits'.format(date_obs[11:].replace(':', ''),
                                                                   '_q' if imgtype == 'flat' else ''))
            files.append(P.fpack_image(ctx, name, img, h, quant=16))
            del img
    bpm = np.zeros((ny, nx), np.uint8)
    bpm[:10] = bpm[-10:] = 32
    bpm[:, :10] = bpm[:, -10:] = 32
    fitsio.write_image(os.path.join(root, 'bpm_q.fits'), bpm)
    return files


def drop_cache(files):
    """ask the kernel to forget the input files' pages (cold read); -> whether it was possible"""
    ok = True
    for f in files:
        try:
            fd = os.open(f, os.O_RDONLY)
            try:
                os.fsync(fd)
                os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
            finally:
                os.close(fd)
        except (OSError, AttributeError):
            ok = False
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--tag', default='dev')
    ap.add_argument('--scratch', default=None, help='scratch folder for the frames (default: a new temporary folder)')
    ap.add_argument('--nbias', type=int, default=20)
    ap.add_argument('--nflat', type=int, default=15)
    ap.add_argument('--repeat', type=int, default=2, help='warm runs per master')
    ap.add_argument('--keep', action='store_true', help='keep the scratch tree')
    a = ap.parse_args()
    import tempfile
    root = a.scratch or tempfile.mkdtemp(prefix='bbx_master_bench_')
    red = os.path.join(root, 'red')
    ctx = R.Context(0)
    t0 = time.time()
    files = synthesise(ctx, red, root, a.nbias, a.nflat)
    ctx.sync()
    t_synth = time.time() - t0
    in_bytes = {t: sum(os.path.getsize(f) for f in files if '/{}/'.format(t) in f) for t in ('bias', 'flat')}
    runs = []
    torch.cuda.reset_peak_memory_stats()
    k = 0
    for imgtype in ('bias', 'flat'):
        for cold in [True] + [False] * a.repeat:
            cache_dropped = drop_cache([f for f in files if '/{}/'.format(imgtype) in f]) if cold else None
            mdir = os.path.join(root, 'masters_%d' % k)
            k += 1
            timing = {}
            t0 = time.time()
            (_, path, err), = M.create_masters('20240105', red, mdir, tel='ML1', ctx=ctx, imgtypes=imgtype, filters='q',
                                               bpm=os.path.join(root, 'bpm.fits'), timing=timing)
            wall = time.time() - t0
            if err is not None or path is None:
                raise RuntimeError('master {} failed: {}'.format(imgtype, err))
            runs.append(dict(imgtype=imgtype, nframes=a.nbias if imgtype == 'bias' else a.nflat,
                             page_cache='cold' if cold else 'warm', cache_dropped=cache_dropped,
                             files_to_master_s=round(wall, 3), phases_s={p: round(v, 3) for p, v in timing.items()},
                             input_MB=round(in_bytes[imgtype] / 1e6, 1), master_MB=round(os.path.getsize(path) / 1e6, 1)))
            print(json.dumps(runs[-1]), flush=True)
            shutil.rmtree(mdir, ignore_errors=True)
    out = dict(tag=a.tag, frame=[settings.ny * settings.ysize_chan, settings.nx * settings.xsize_chan],
               reader_threads=max(1, min(8, pipeline.cpu_budget() // 2)), cpu_budget=pipeline.cpu_budget(),
               synthesis_s=round(t_synth, 1), runs=runs,
               hbm_peak_GB_tensors=round(torch.cuda.max_memory_allocated() / 1e9, 2),
               device=torch.cuda.get_device_name(0))
    ctx.close()
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', '{}_masters.json'.format(a.tag)), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    if not a.keep and not a.scratch:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
