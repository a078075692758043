"""What the catalogue photometry with the PSF on the centroid (zogy.optimal_subtraction(phot_centroid=True)) costs.

    python tools/phot_bench.py [--out profiles/phot_centroid.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (no kernel of bbx_psfphot.hip is launched: source_psfs + psf_optflux at the integer peaks)
  on : phot_centroid=True: bbx_win_centroid, then bbx_psf_optflux_shift with the frame's mask
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then the stages by themselves on that frame's background-subtracted image and source list, each
between two HIP events with the host's part inside (the terms or plane indices are made on the host per call):
  stamps_and_flux: source_psfs + psf_optflux (the off leg's photometry)
  centroid       : win_centroid
  fused          : psf_optflux_centroid with the centroids given (the on leg's photometry without them)
  fused_sigma_frame: the same with sigma as a full frame where the frame's is a mini image (what reading the spline per pixel costs)
The result goes to [out] and to stdout as one JSON line.
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
    from blackbox_amd import zogy as G
    from blackbox_amd._lib import push
    data, mask, kw = T.scene(ctx)
    legs = {'off': dict(kw), 'on': dict(kw, phot_centroid=True)}
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['off'])
    ctx.sync()
    ys, xs = (res['catalog']['Y_POS'] - 1).astype(np.int32), (res['catalog']['X_POS'] - 1).astype(np.int32)       # the integer peaks
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    cat = res['catalog']
    work, bstd = res['data_bkgsub'], res['bkg_std']
    size = kw['subimage_size']
    nsy, nsx = work.shape[0] // size, work.shape[1] // size
    psf_new = kw['psf_new']
    sub_pn = G.subimage_psfs(ctx, psf_new, nsy, nsx, size)
    # the stages alone at the catalogue's sources (the few peaks on masked pixels, which the frame measures and drops, are not among them)
    d_ys, d_xs = push(ctx, ys, xs)
    sigw = G.window_sigma(sub_pn)
    d_off = G.win_centroid(ctx, work, d_ys, d_xs, sigw, size, nsy, nsx)
    info = dict(sources=int(len(ys)), stamp_side=int(sub_pn.shape[1]), psf_form='model' if isinstance(psf_new, dict) else 'planes',
                sigma_form='mini image' if isinstance(bstd, G.MiniImage) else 'frame', flags_opt=np.bincount(cat['FLAGS_OPT'], minlength=8).tolist(),
                header={k: res['header_new'][k][0] for k in ('PHOT-CEN', 'NOBJECTS')})
    del res
    times = {k: [] for k in legs}
    stage = {'stamps_and_flux': [], 'centroid': [], 'fused': [], 'fused_sigma_frame': []}
    sig_frame = bstd.frame(ctx) if isinstance(bstd, G.MiniImage) else bstd

    def timed(fn, sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        ctx.sync()
        del r
        if sink is not None:
            sink.append(e0.elapsed_time(e1))
    calls = {
        'stamps_and_flux': lambda: G.psf_optflux(ctx, work, bstd, G.source_psfs(ctx, psf_new, sub_pn, ys, xs, nsx, size), ys, xs, v_is_sigma=True),
        'centroid': lambda: G.win_centroid(ctx, work, d_ys, d_xs, sigw, size, nsy, nsx),
        'fused': lambda: G.psf_optflux_centroid(ctx, work, bstd, psf_new, sub_pn, ys, xs, d_off, mask, nsx, size, d_peaks=(d_ys, d_xs)),
        'fused_sigma_frame': lambda: G.psf_optflux_centroid(ctx, work, sig_frame, psf_new, sub_pn, ys, xs, d_off, mask, nsx, size,
                                                            d_peaks=(d_ys, d_xs))}
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            timed(fn, stage[name] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (phot_centroid off / on) alternating in one process; the photometry stages alone at the catalogue\'s sources',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    smed = {k: statistics.median(v) for k, v in stage.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    out['stages_added_ms'] = smed['centroid'] + smed['fused'] - smed['stamps_and_flux']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'phot_centroid.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('phot_bench.py needs a GPU: nothing is measured without one')
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
