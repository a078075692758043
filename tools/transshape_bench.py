"""What the transient shape fits (zogy.optimal_subtraction(trans_shapefit=True)) cost.

    python tools/transshape_bench.py [--out profiles/transshape.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (bbx_trans_shapefit is not launched: the parent's path)
  on : trans_shapefit=True: bbx_trans_shapefit (Gauss and Moffat) at the frame's candidates
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then the entry by itself on that frame's images and candidate list, between two HIP events with the
host's part inside:
  shapefit   : zogy.trans_shapefit, both models
  gauss      : ... the Gaussian alone
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
    from blackbox_amd import settings, zogy as G
    from blackbox_amd._lib import push
    data, mask, kw = T.scene(ctx)
    legs = {'off': dict(kw), 'on': dict(kw, trans_shapefit=True)}
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    rows, ht = res['transients'], res['header_trans']
    ys, xs = np.array([t['y'] for t in rows], np.int32), np.array([t['x'] for t in rows], np.int32)
    size = kw['subimage_size']
    nsy, nsx = data.shape[0] // size, data.shape[1] // size

    def stamps(psf):
        if isinstance(psf, dict):
            return G.subimage_psfs(ctx, psf, nsy, nsx, size).contiguous()
        return (psf if psf.dim() == 3 else psf[None].expand(nsy * nsx, -1, -1)).contiguous()
    fwhm0 = G.shape_start_fwhm(stamps(kw['psf_new']), stamps(kw['psf_ref']))
    scal = res['scal']
    frames_ = [res[k] for k in ('D', 'data_bkgsub', 'ref_bkgsub')]
    sig = (res['bkg_std'], res['bkg_std_ref'])
    if isinstance(sig[0], G.MiniImage) != isinstance(sig[1], G.MiniImage):
        sig = tuple(s.frame(ctx) if isinstance(s, G.MiniImage) else s for s in sig)
    d_peaks = push(ctx, ys, xs)
    info = dict(candidates=int(len(rows)), sub_images=int(nsy * nsx), shape_size=int(settings.trans_shape_size),
                shape_niter=int(settings.trans_shape_niter), moffat_beta=float(settings.trans_moffat_beta),
                sigma_form='mini image' if isinstance(sig[0], G.MiniImage) else 'frame',
                flags_gauss_d=np.bincount(np.array([t['flags_gauss_d'] for t in rows], np.uint8), minlength=32).tolist(),
                flags_moffat_d=np.bincount(np.array([t['flags_moffat_d'] for t in rows], np.uint8), minlength=32).tolist(),
                header={k: ht[k][0] for k in ('T-NTRANS', 'T-SHAPE', 'T-SHPSZ', 'T-MBETA', 'T-NGAUS', 'T-NMOFF', 'T-FWGMD', 'T-ELGMD')})
    del res
    times = {k: [] for k in legs}
    stage = {'shapefit': [], 'gauss': []}

    def timed(fn, sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        ctx.sync()
        del r
        if sink is not None:
            sink.append(e0.elapsed_time(e1))

    def fit(models):
        return G.trans_shapefit(ctx, frames_[0], frames_[1], frames_[2], sig[0], sig[1], mask, fwhm0, ys, xs, scal, size, nsx, models=models,
                                d_peaks=d_peaks)
    calls = {'shapefit': lambda: fit(3), 'gauss': lambda: fit(1)}
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            timed(fn, stage[name] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (trans_shapefit off / on) alternating in one process; the entry alone on that frame\'s candidates',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transshape.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('transshape_bench.py needs a GPU: nothing is measured without one')
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
