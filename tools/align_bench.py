"""What the registration of the reference from its stars (zogy.optimal_subtraction(ref_align=True)) costs.

    python tools/align_bench.py [--out profiles/align.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword, against the scene's reference on the new frame's grid, its sigma map kept as a run keeps it (no
       kernel of bbx_align.hip is launched: the parent's path)
  on : ref_align=True against that reference moved by (+17.3, -41.6) px with the LANCZOS3 resampler, the reference's star list
       (RefStars) kept as a run keeps it: the vote, the fits and match rounds, the lattice, the mask, the resampling of the
       reference and the remapping of its sigma mini image, every frame
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then by themselves on that frame, between two HIP events with the host's part inside:
  remap_mask : zogy.remap_mask (bbx_remap_mask) of the reference's mask through the fitted lattice
  resample   : coadd.resample (bbx_resample_lanczos3) of the reference through it
  chain      : zogy.align_reference: vote, fits, match rounds, lattice, mask and its one host wait
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

SHIFT = (17.3, -41.6)            # (dy, dx): input position = output position + SHIFT, inside align_max_shift


def stats(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))


def frames(ctx, torch, a):
    import numpy as np
    import thumbs_bench as T
    from blackbox_amd import coadd, zogy as G
    data, mask, kw = T.scene(ctx)
    ny, nx = data.shape
    step = 32
    gy, gx = np.arange(0, ny + step, step, dtype=np.float64), np.arange(0, nx + step, step, dtype=np.float64)
    yy, xx = np.meshgrid(gy, gx, indexing='ij')
    moved, _ = coadd.resample(ctx, kw['ref'], torch.ones_like(kw['ref']), np.ascontiguousarray(np.stack([xx + SHIFT[1], yy + SHIFT[0]], axis=-1)),
                              (ny, nx), 1.0, step)
    legs = {'off': dict(kw), 'on': dict(kw, ref=moved, ref_align=True)}
    first = {k: G.optimal_subtraction(ctx, data, new_mask=mask, **leg) for k, leg in legs.items()}
    ctx.sync()
    legs['off']['ref_bkg_std'] = first['off'].get('bkg_std_ref')                        # the reference's sigma map as a run keeps it
    legs['on']['ref_stars'] = first['on']['ref_stars']                                  # ... and its star list
    on = first['on']
    al, ht = on['align'], on['header_trans']
    if al is None or al['flags'] != 0:
        sys.exit('the registration failed on the benchmark scene: %s' % {k: v[0] for k, v in ht.items() if k.startswith('A-')})
    # the new frame's star list for the chain by itself: the same builder on the new frame's background-subtracted image
    size = kw['subimage_size']
    nsy, nsx = ny // size, nx // size
    sig = on['bkg_std'].frame(ctx) if isinstance(on['bkg_std'], G.MiniImage) else on['bkg_std']
    new_stars = G.RefStars(ctx, on['data_bkgsub'], sig, mask, G.subimage_psfs(ctx, kw['psf_new'], nsy, nsx, size).contiguous(), nsy, nsx, size,
                           sigma_median=on['header_new']['S-BKGSTD'][0])
    ref_stars, grid = on['ref_stars'], al['grid']
    ones = torch.ones_like(moved)
    info = dict(shift_applied=dict(dy=SHIFT[0], dx=SHIFT[1]), new_sources=new_stars.n, ref_sources=ref_stars.n,
                header={k: ht[k][0] for k in ht if k.startswith('A-') or k in ('T-NOFFR', 'T-NTRANS')},
                transients=dict(off=len(first['off']['transients']), on=len(on['transients'])))
    del first, on, sig
    times = {k: [] for k in legs}
    stage = {'remap_mask': [], 'resample': [], 'chain': []}

    def timed(fn, sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        ctx.sync()
        del r
        if sink is not None:
            sink.append(e0.elapsed_time(e1))
    calls = {'remap_mask': lambda: G.remap_mask(ctx, kw['ref_mask'], (ny, nx), grid, (ny, nx), step),
             'resample': lambda: coadd.resample(ctx, moved, ones, grid, (ny, nx), 1.0, step),
             'chain': lambda: G.align_reference(ctx, new_stars.lists(), ref_stars, (ny, nx), (ny, nx), kw['ref_mask'])}
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            timed(fn, stage[name] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (ref_align off: reference on the grid / on: reference moved by a non-integer shift) alternating in one '
                    'process; three parts of the on leg alone on that frame',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    out['remap_mask_GBps'] = (ny * nx * 2 + 0.0) / (statistics.median(stage['remap_mask']) * 1e-3) / 1e9       # one byte out, about one in
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'align.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('align_bench.py needs a GPU: nothing is measured without one')
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
