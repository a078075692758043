"""What the limiting-flux image of the reduced frame (zogy.optimal_subtraction(limmag=True)) costs.

    python tools/limflux_bench.py [--out profiles/limflux.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (no kernel of bbx_limflux.hip is launched: the path of the commit before, timed at this one)
  on : limmag=True: bbx_limflux_image, bbx_frame_clipped_stats of its image, two more tensors in the copy back
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then bbx_limflux_image by itself on that frame's sigma map, mask and PSF stamps, between two HIP events
(the window kernel and the frame kernel together), with the windows T it ran at and the share of the float32 vector peak that
2 T^2 N FLOP in that time are (157.3 TFLOP/s; where the tiles' windows differ, the sum over the tiles' pixels):
  frac_0      : the whole stamp
  frac_1e-4   : settings.limmag_psf_frac
  *_sigma_frame: the same with sigma as a full frame where the frame's is a mini image (what reading the spline per pixel costs)
  stats       : bbx_frame_clipped_stats of the image
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
PEAK_F32 = 157.3e12


def stats(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))


def frames(ctx, torch, a):
    import numpy as np
    import thumbs_bench as T
    from blackbox_amd import zogy as G
    data, mask, kw = T.scene(ctx)
    legs = {'off': dict(kw), 'on': dict(kw, limmag=True)}
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    bstd = res['bkg_std']
    size = kw['subimage_size']
    ny, nx = data.shape
    nsy, nsx = ny // size, nx // size
    sub_pn = G.subimage_psfs(ctx, kw['psf_new'], nsy, nsx, size).contiguous()
    lim = res['limflux']
    info = dict(shape=[int(ny), int(nx)], stamp_side=int(sub_pn.shape[1]), tiles=[nsy, nsx], tile_size=int(size),
                sigma_form='mini image' if isinstance(bstd, G.MiniImage) else 'frame',
                header={k: v[0] for k, v in res['header_new'].items() if k.startswith('LIM')})
    del res
    sig_frame = bstd.frame(ctx) if isinstance(bstd, G.MiniImage) else bstd

    def timed(fn, sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        ctx.sync()
        if sink is not None:
            sink.append(e0.elapsed_time(e1))
        return r

    def limflux(sig, frac):
        return lambda: G.limflux_image(ctx, sig, mask, sub_pn, size, nsy, nsx, frac=frac)
    calls = {'frac_0': limflux(bstd, 0.0), 'frac_1e-4': limflux(bstd, 1e-4)}
    if sig_frame is not bstd:
        calls.update({'frac_0_sigma_frame': limflux(sig_frame, 0.0), 'frac_1e-4_sigma_frame': limflux(sig_frame, 1e-4)})
    calls['stats'] = lambda: G.frame_clipped_stats_enqueue(ctx, lim, mask)
    times, stage, wins = {k: [] for k in legs}, {k: [] for k in calls}, {}
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            r = timed(fn, stage[name] if keep else None)
            if name != 'stats' and name not in wins:
                wins[name] = r[1].cpu().numpy()
            del r
    # the tiles' pixels: every tile size x size, the last row and column of tiles take the rest
    th = np.full(nsy, size); th[-1] = ny - (nsy - 1) * size
    tw = np.full(nsx, size); tw[-1] = nx - (nsx - 1) * size
    npx = np.outer(th, tw).reshape(-1).astype(np.float64)
    kern = {}
    for name, w in wins.items():
        flop = float((2.0 * w.astype(np.float64) ** 2 * npx).sum())
        ms = statistics.median(stage[name])
        kern[name] = dict(windows=sorted(set(w.tolist())), window_median=int(np.median(w)), flop=flop, tflops=flop / (ms * 1e-3) / 1e12,
                          fraction_of_f32_vector_peak=flop / (ms * 1e-3) / PEAK_F32)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (limmag off / on) alternating in one process; bbx_limflux_image alone on that frame (both kernels of the call)',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()}, kernel=kern)
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'limflux.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('limflux_bench.py needs a GPU: nothing is measured without one')
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
