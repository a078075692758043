"""What the transient thumbnails add to a frame of the benchmark's scene (10560 x 10560, bench.py's ZOGY inputs).

    python tools/thumbs_bench.py [--out profiles/thumbnails.json] [--warmup 10] [--frames 30] [--no-rocprof]

One reduced frame is made once (untimed).  Then zogy.optimal_subtraction runs on it with the switches off and with
thumbnails=True, thumbnail_pngs=True, alternating, in this one process: each call between two HIP events, [warmup]
untimed calls of each leg first, the median of [frames] calls per leg.  The library's own launch timers
(bbx_profile_enable) give the time of the bbx_zogy_frame launch group in the same calls.  The two new kernels are timed by
rocprofv3 --kernel-trace --stats in a run of its own: a child process (this script with --kernels-only, directly after
`--`) that does nothing but a few switched-on frames.  The result goes to [out] and to stdout as one JSON line.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ZOGY_SLOTS = (7, 8, 9, 10, 11, 12, 13)          # launch slots of bbx_zogy_frame's kernels in bbx_profile_read (bench.py)
NSL = 14


def scene(ctx):
    """bench.py's headline scene: raw frame -> reduced frame + mask, and the keyword arguments of the subtraction"""
    import torch
    import numpy as np
    import bench as B
    from blackbox_amd import reduce as R
    dev = ctx.device
    ysz, xsz, os_y, os_x = 5280, 1320, 20, 180
    size, border, box = 1320, 40, 60
    seed = 4000
    torch.use_deterministic_algorithms(True)
    raw, flat, bpm, ex = B.synth_frame_device(torch, dev, ysz, xsz, os_y, os_x, seed, 'u16', extras=True, ntrans=50,
                                              psf_field=B.zogy_psf_field(2 * ysz // size, 8 * xsz // size, size))
    ref, ref_mask = B.synth_reference(torch, dev, ex.pop('scene0'), seed)
    torch.use_deterministic_algorithms(False)
    geom = R.geometry(raw.shape, ysz, xsz)
    kw = B.zogy_inputs(torch, dev, 2 * ysz // size, 8 * xsz // size, 49, box, 2 * ysz, 8 * xsz)
    kw.update(ref=ref, ref_mask=ref_mask, cat_extract=True, trans_extract=True, subimage_size=size, subimage_border=border,
              bkg_boxsize=box)
    rs = np.random.RandomState(0)
    coeffs = np.zeros((16, 16)); coeffs[~np.eye(16, dtype=bool)] = rs.uniform(0, 2e-4, 240)
    header, hm, tel = {}, {}, 'ML1'
    R.gain_corr(header, tel)
    sol = R.os_solve(ctx, raw, header, tel, geom)
    data, mask = R.calibrate(ctx, raw, sol, header, hm, tel, geom, mflat=flat, bpm=bpm)
    R.mask_init_finish(ctx, mask, header, hm, geom)
    R.cosmics_corr(ctx, data, header, mask, hm, tel)
    R.xtalk_corr(ctx, data, coeffs, mask, geom)
    R.sat_detect(ctx, data, header, mask, hm)
    R.mask_header(ctx, mask, hm)
    R.edge_fill(ctx, data, mask, geom)
    ctx.sync()
    del raw, flat, bpm
    return data, mask, kw


def kernels_only(frames):
    """the rocprofv3 child: [frames] switched-on calls, nothing else"""
    from blackbox_amd import reduce as R, zogy as G
    ctx = R.Context(0)
    data, mask, kw = scene(ctx)
    n = 0
    for _ in range(frames):
        res = G.optimal_subtraction(ctx, data, new_mask=mask, thumbnails=True, thumbnail_pngs=True, **kw)
        ctx.sync()
        n = len(res['transients'])
        del res
    print('THUMBS_CHILD ' + json.dumps(dict(frames=frames, candidates=n)))
    ctx.close()


def rocprof_kernels(frames):
    """-> {kernel: ms per frame} of the two new kernels from a rocprofv3 --kernel-trace --stats run of its own"""
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    out = tempfile.mkdtemp(prefix='thumbs_prof_')
    try:
        cmd = [exe, '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__),
               '--kernels-only', '--frames', str(frames)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error='rocprofv3 exit {}: {}'.format(r.returncode, (r.stderr or r.stdout)[-400:]))
        res = {}
        for fn in glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    name = row.get('Name', '')
                    for k in ('k_thumb_gather', 'k_thumb_png8'):
                        if k in name:
                            res[k] = dict(ms_per_frame=float(row['TotalDurationNs']) * 1e-6 / frames, launches=int(row['Calls']),
                                          avg_launch_ms=float(row['AverageNs']) * 1e-6)
        return res or dict(error='no kernel_stats.csv rows for the thumbnail kernels under ' + out)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'thumbnails.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--no-rocprof', action='store_true')
    ap.add_argument('--off-only', action='store_true', help='only the switched-off leg (a tree without the feature)')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.frames)
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up frames and 30 timed frames per leg')
    # the profiler run first, while this process has not touched the GPU
    prof = None if (a.no_rocprof or a.off_only) else rocprof_kernels(5)
    import torch
    from blackbox_amd import _lib, reduce as R, zogy as G
    ctx = R.Context(0)
    data, mask, kw = scene(ctx)
    legs = {'off': {}} if a.off_only else {'off': {}, 'on': dict(thumbnails=True, thumbnail_pngs=True)}
    times = {k: [] for k in legs}
    zogy_ms = {k: [0.0, 0] for k in legs}
    ncand = 0

    def frame(leg, timed):
        nonlocal ncand
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed:
            _lib.check(_lib.lib.bbx_profile_enable(ctx.h, 1), 'bbx_profile_enable')
        e0.record()
        res = G.optimal_subtraction(ctx, data, new_mask=mask, **kw, **legs[leg])
        e1.record()
        ctx.sync()
        ncand = len(res['transients'])
        del res
        if timed:
            ms, nc = (C.c_double * NSL)(), (C.c_int32 * NSL)()
            _lib.check(_lib.lib.bbx_profile_read(ctx.h, ms, nc, NSL), 'bbx_profile_read', ctx.h)
            _lib.check(_lib.lib.bbx_profile_enable(ctx.h, 0), 'bbx_profile_enable')
            zogy_ms[leg][0] += sum(ms[s] for s in ZOGY_SLOTS); zogy_ms[leg][1] += 1
            times[leg].append(e0.elapsed_time(e1))
    for _ in range(a.warmup):
        for leg in legs:
            frame(leg, False)
    for _ in range(a.frames):
        for leg in legs:
            frame(leg, True)

    def stats(v):
        v = sorted(v)
        return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))
    out = dict(what='zogy.optimal_subtraction on bench.py\'s 10560 x 10560 scene, HIP events around each call, legs alternating in one process',
               candidates=ncand, thumbnail_size=100, warmup_per_leg=a.warmup,
               optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               bbx_zogy_frame_ms_per_frame={k: v[0] / max(1, v[1]) for k, v in zogy_ms.items()},
               kernels_rocprofv3=prof)
    if 'on' in times:
        out['added_ms_per_frame'] = statistics.median(times['on']) - statistics.median(times['off'])
        out['added_fraction_of_off'] = out['added_ms_per_frame'] / statistics.median(times['off'])
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
