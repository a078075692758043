"""What the object mask and the second background pass (--objmask) cost.

    python tools/objmask_bench.py [--out profiles/objmask.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene, 10560 x 10560; cat_extract on in both legs) through
zogy.optimal_subtraction with objmask=False and objmask=True, alternating, in this one process: each call between two HIP
events, [warmup] untimed calls of each leg first, the median of [frames] calls per leg.  The off leg launches no kernel of
bbx_objmask.hip: it is the path of a build without the switch.  Then bbx_object_mask by itself on that scene's first-pass frame,
the same way.  The result goes to [out] and to stdout as one JSON line.
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


def timed(ctx, torch, fn, warmup, frames):
    for _ in range(warmup):
        fn()
    ctx.sync()
    t = []
    for _ in range(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ctx.sync()
        t.append(e0.elapsed_time(e1))
    return stats(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'objmask.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('objmask_bench.py needs a GPU: nothing is measured without one')
    import thumbs_bench as T
    from blackbox_amd import reduce as R, settings, zogy as G
    ctx = R.Context(0)
    data, mask, kw = T.scene(ctx)
    res = G.optimal_subtraction(ctx, data, new_mask=mask, objmask=True, **kw)
    ctx.sync()
    kw = dict(kw, ref_bkg_std=res['bkg_std_ref'])                 # both legs: the reference's sigma map as a run keeps it
    hn = res['header_new']
    npix = data.numel()
    info = dict(frame=list(data.shape), sources=len(res['catalog']['X_POS']) if res.get('catalog') else None,
                header={k: hn[k][0] for k in hn if k.startswith('OBJM-') or k in ('S-BKG', 'S-BKGSTD', 'S-BKG1', 'S-BKGSD1')},
                listed_fraction=hn['OBJM-NPX'][0] / npix if hn['OBJM-P'][0] else None,
                nsigma=settings.objmask_nsigma, minarea=settings.objmask_minarea, grow=settings.objmask_grow, filter=settings.objmask_filter)
    del res
    legs = {'off': dict(objmask=False), 'on': dict(objmask=True)}
    times = {k: [] for k in legs}

    def frame(leg, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = G.optimal_subtraction(ctx, data, new_mask=mask, **kw, **legs[leg])
        e1.record()
        ctx.sync()
        del r
        if keep:
            times[leg].append(e0.elapsed_time(e1))
    for _ in range(a.warmup):
        for leg in legs:
            frame(leg, False)
    for _ in range(a.frames):
        for leg in legs:
            frame(leg, True)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each call, legs '
                    '(objmask off / on) alternating in one process', warmup_per_leg=a.warmup, **info,
               optimal_subtraction_ms={k: stats(v) for k, v in times.items()})
    out['added_ms_per_frame'] = statistics.median(times['on']) - statistics.median(times['off'])
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / statistics.median(times['off'])
    # the stages by themselves, on the first pass's frame
    box = kw.get('bkg_boxsize') or settings.bkg_boxsize
    mini, std = G.get_back(ctx, data, mask, bkg_boxsize=box)
    work = torch.empty_like(data)
    G.mini2back(ctx, mini, tuple(data.shape), bkg_boxsize=box, interp_Xchan=True, subtract_from=data, subtract_into=work)
    om, _ = G.object_mask(ctx, work, std, box)
    out['stages_ms'] = {
        'bbx_object_mask': timed(ctx, torch, lambda: G.object_mask_enqueue(ctx, work, std, box), a.warmup, a.frames),
        'get_back': timed(ctx, torch, lambda: G.get_back(ctx, data, mask, bkg_boxsize=box), a.warmup, a.frames),
        'get_back_with_objmask': timed(ctx, torch, lambda: G.get_back(ctx, data, mask, om, bkg_boxsize=box), a.warmup, a.frames),
        'mini2back_subtract': timed(ctx, torch, lambda: G.mini2back(ctx, mini, tuple(data.shape), bkg_boxsize=box, interp_Xchan=True,
                                                                     subtract_from=data, subtract_into=work), a.warmup, a.frames)}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
