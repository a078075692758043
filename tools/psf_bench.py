"""What the PSF model from the frame's own stars (`_psf.fits`, the PSF-* keys; zogy.build_psf) costs.

    python tools/psf_bench.py [--out profiles/psf_build.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  given: with the scene's PSF stamps as psf_new (no kernel of bbx_psfbuild.hip is launched: the path of a run with --psf_new)
  build: with psf_new=None, psf_build=True: the model (V = settings.psf_size, degree settings.psf_poldeg, at most
         settings.psf_stars_nmax stars) is built behind the catalogue's peak search and used from there on
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then zogy.build_psf by itself on that frame's background-subtracted image with the peaks given (host
time included: it has one host wait).  The result goes to [out] and to stdout as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def stats(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))


def frames(ctx, torch, a):
    import numpy as np
    import thumbs_bench as T
    from blackbox_amd import settings, zogy as G
    data, mask, kw = T.scene(ctx)
    legs = {'given': dict(kw), 'build': dict(kw, psf_new=None, psf_build=True)}
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['build'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    hn = res['header_new']
    st = res['psf']['stars']
    info = dict(sources=st['n_sources'], qualifying=st['n_qualifying'], stride=st['stride'], stars=int(len(st.get('index', ()))),
                with_vignette=int(np.count_nonzero(st.get('ok', ()))), psf_size=settings.psf_size, psf_poldeg=settings.psf_poldeg,
                psf_stars_nmax=settings.psf_stars_nmax, catalogue=None if res['catalog'] is None else len(res['catalog']['X_POS']),
                header={k: hn[k][0] for k in hn if k.startswith('PSF-')})
    # build_psf by itself: the frame, sigma mini image and peaks of that call
    work, sdn = res['data_bkgsub'], res['bkg_std_mini_new']
    size = kw['subimage_size']
    nsy, nsx = work.shape[0] // size, work.shape[1] // size
    sstd = hn['S-BKGSTD'][0]
    peaks = G.find_peaks_arrays(ctx, work, 5.0 * sstd, max_out=200000)
    d_sdn = torch.from_numpy(np.ascontiguousarray(sdn)).to(ctx.device)
    del res
    times = {k: [] for k in legs}
    alone = []

    def frame(leg, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg])
        e1.record()
        ctx.sync()
        del r
        if timed:
            times[leg].append(e0.elapsed_time(e1))

    def build(timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        G.build_psf(ctx, work, d_sdn, mask, size, nsy, nsx, sigma_median=sstd, peaks=peaks)
        e1.record()
        ctx.sync()
        if timed:
            alone.append(e0.elapsed_time(e1))
    for _ in range(a.warmup):
        for leg in legs:
            frame(leg, False)
        build(False)
    for _ in range(a.frames):
        for leg in legs:
            frame(leg, True)
        build(True)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (PSF given / PSF built) alternating in one process; build_psf alone with the peaks given',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()}, build_psf_alone_ms=stats(alone))
    out['added_ms_per_frame'] = statistics.median(times['build']) - statistics.median(times['given'])
    out['added_fraction_of_given'] = out['added_ms_per_frame'] / statistics.median(times['given'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'psf_build.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('psf_bench.py needs a GPU: nothing is measured without one')
    from blackbox_amd import reduce as R
    ctx = R.Context(0)
    out = dict(frame=frames(ctx, torch, a))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
