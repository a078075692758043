"""What the aperture photometry of the catalogue (zogy.optimal_subtraction(aper_phot=True)) costs.

    python tools/aper_bench.py [--out profiles/apphot.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (no kernel of bbx_aper.hip is launched: the path of the commit before, timed at this one)
  on : aper_phot=True: bbx_win_centroid, the frame's FWHM, bbx_aper_phot with the frame's mask, five more tensors in the copy back
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then the stages by themselves on that frame's background-subtracted image and source list, each
between two HIP events:
  centroid        : win_centroid (shared with shapes and phot_centroid where those are on)
  aper            : aper_phot with the centroids given, sigma as the frame carries it
  aper_sigma_frame: the same with sigma as a full frame where the frame's is a mini image (what reading the spline per pixel costs)
  aper_no_sky     : radii as set, the annulus shrunk to (5.0, 5.2) x FWHM: what gathering, sorting and clipping the sky sample costs
  aper_one        : the 5 x FWHM aperture alone
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
    from blackbox_amd import zogy as G, settings as S
    from blackbox_amd._lib import push
    data, mask, kw = T.scene(ctx)
    legs = {'off': dict(kw), 'on': dict(kw, aper_phot=True)}
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    cat = res['catalog']
    ys, xs = (cat['Y_POS'] - 1).astype(np.int32), (cat['X_POS'] - 1).astype(np.int32)       # the integer peaks
    work, bstd = res['data_bkgsub'], res['bkg_std']
    size = kw['subimage_size']
    nsy, nsx = work.shape[0] // size, work.shape[1] // size
    sub_pn = G.subimage_psfs(ctx, kw['psf_new'], nsy, nsx, size)
    d_ys, d_xs = push(ctx, ys, xs)
    sigw = G.window_sigma(sub_pn)
    d_off = G.win_centroid(ctx, work, d_ys, d_xs, sigw, size, nsy, nsx)
    d_fw = G.aper_fwhm(sub_pn).expand(nsy * nsx).contiguous()
    info = dict(sources=int(len(ys)), fwhm=res['aper']['fwhm'], radii=list(res['aper']['radii']), sky_inout=list(S.apphot_sky_inout),
                sigma_form='mini image' if isinstance(bstd, G.MiniImage) else 'frame',
                flags_aper=np.bincount(cat['FLAGS_APER'], minlength=64).tolist(), nsky_median=float(np.median(cat['NSKY_APER'])),
                header={k: v[0] for k, v in res['header_new'].items() if k.startswith('AP-')})
    del res
    times = {k: [] for k in legs}
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

    def aper(sig, **more):
        return lambda: G.aper_phot(ctx, work, sig, mask, d_ys, d_xs, d_off, d_fw, size, nsy, nsx, **more)
    calls = {'centroid': lambda: G.win_centroid(ctx, work, d_ys, d_xs, sigw, size, nsy, nsx),
             'aper': aper(bstd), 'aper_sigma_frame': aper(sig_frame), 'aper_no_sky': aper(bstd, sky_inout=(5.0, 5.2), sky_nmin=1),
             'aper_one': aper(bstd, radii=(5.0,))}
    stage = {k: [] for k in calls}
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            timed(fn, stage[name] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (aper_phot off / on) alternating in one process; the stages alone at the catalogue\'s sources',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'apphot.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('aper_bench.py needs a GPU: nothing is measured without one')
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
