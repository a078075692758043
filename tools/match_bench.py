"""What the star match (fratio, dx, dy from matched stars) adds to a frame of the benchmark's scene (10560 x 10560, bench.py's
ZOGY inputs).

    python tools/match_bench.py [--out profiles/match.json] [--warmup 10] [--frames 30] [--no-rocprof]

One reduced frame is made once (untimed; tools/thumbs_bench.scene).  Then zogy.optimal_subtraction runs on it with match=False
and with match=True and the run's RefCatalog, alternating, in this one process: each call between two HIP events, [warmup]
untimed calls of each leg first, the median of [frames] calls per leg.  The three kernels of bbx_match.hip are timed by
rocprofv3 --kernel-trace --stats in a run of its own: a child process (this script with --kernels-only, directly after `--`)
that does nothing but a few switched-on frames.  The result goes to [out] and to stdout as one JSON line.
"""
import argparse
import csv
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

KERNELS = ('k_win_centroid', 'k_match_nearest', 'k_match_stats')


def prepared(ctx):
    """the scene, the reference's sigma map and catalogue as a run keeps them -> (data, mask, kw of the switched-on leg, info)"""
    import thumbs_bench as T
    from blackbox_amd import zogy as G
    data, mask, kw = T.scene(ctx)
    res = G.optimal_subtraction(ctx, data, new_mask=mask, match=True, **kw)
    ctx.sync()
    on = dict(match=True, ref_catalog=res['ref_catalog'])
    kw = dict(kw, ref_bkg_std=res['bkg_std_ref'])                 # both legs: the reference's sigma map as a run keeps it
    m = res['match']
    info = dict(sources_new=m['n_new'], sources_ref=m['n_ref'], pairs=m['n_pairs'], qualifying=int(m['table'][-1, 0]), success=m['success'],
                catalogue_reused=bool(res['ref_catalog'].matches(res['ref_bkgsub'], res['bkg_std_ref'], kw['subimage_size'], kw['subimage_border'])))
    return data, mask, kw, on, info


def kernels_only(frames):
    """the rocprofv3 child: [frames] switched-on calls, nothing else timed apart"""
    from blackbox_amd import reduce as R, zogy as G
    ctx = R.Context(0)
    data, mask, kw, on, info = prepared(ctx)
    for _ in range(frames):
        res = G.optimal_subtraction(ctx, data, new_mask=mask, **kw, **on)
        ctx.sync()
        del res
    print('MATCH_CHILD ' + json.dumps(dict(frames=frames, **info)))
    ctx.close()


def rocprof_kernels(frames):
    """-> {kernel: ms per launch ...} of the three kernels from a rocprofv3 --kernel-trace --stats run of its own"""
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    out = tempfile.mkdtemp(prefix='match_prof_')
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
                    for k in KERNELS:
                        if k in row.get('Name', ''):
                            res[k] = dict(launches=int(row['Calls']), avg_launch_ms=float(row['AverageNs']) * 1e-6,
                                          max_launch_ms=float(row['MaxNs']) * 1e-6 if row.get('MaxNs') else None)
        return res or dict(error='no kernel_stats.csv rows for the match kernels under ' + out)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--no-rocprof', action='store_true')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.frames)
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up frames and 30 timed frames per leg')
    # the profiler run first, while this process has not touched the GPU
    prof = None if a.no_rocprof else rocprof_kernels(5)
    import torch
    from blackbox_amd import reduce as R, zogy as G
    ctx = R.Context(0)
    data, mask, kw, on, info = prepared(ctx)
    legs = {'off': {}, 'on': on}
    times = {k: [] for k in legs}

    def frame(leg, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = G.optimal_subtraction(ctx, data, new_mask=mask, **kw, **legs[leg])
        e1.record()
        ctx.sync()
        del res
        if timed:
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
    out = dict(what='zogy.optimal_subtraction on bench.py\'s 10560 x 10560 scene, HIP events around each call, legs (match off / on with '
                    'the run\'s RefCatalog) alternating in one process', warmup_per_leg=a.warmup, **info,
               optimal_subtraction_ms={k: stats(v) for k, v in times.items()}, kernels_rocprofv3=prof)
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
