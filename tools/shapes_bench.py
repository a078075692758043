"""What the source shapes (FWHM, ELONGATION, ... of `_cat.fits`, S-SEEING and its companions) cost.

    python tools/shapes_bench.py [--out profiles/shapes.json] [--warmup 10] [--frames 30] [--no-frame]

1. The two launches by themselves, bbx_src_shapes and bbx_shape_stats, for 10^4 and 10^5 sources on a 10560 x 10560 frame: a
   lattice of Gaussian stars (sigma 1.6 px, one every 32 px) on noise, the sources at the lattice points in (y, x) order, started
   from bbx_win_centroid's offsets, radius and iterations of the settings.  [launches] back-to-back launches between two HIP
   events after [warmup] untimed ones, repeated [frames] times: the median time per launch.
2. A frame of the benchmark's scene (tools/thumbs_bench.scene; cat_extract on in both legs) through zogy.optimal_subtraction with
   shapes=False and shapes=True, alternating, in this one process: each call between two HIP events, [warmup] untimed calls of
   each leg first, the median of [frames] calls per leg.
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

NY = NX = 10560
PITCH, SIGMA, SIZE = 32, 1.6, 1320


def stats(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))


def lattice(ctx, torch):
    """-> (frame float32 [NY, NX], mask uint8, ys, xs int32 of all lattice points in (y, x) order)"""
    dev = ctx.device
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    t = (torch.arange(NY, device=dev) % PITCH - PITCH // 2).to(torch.float32)
    p = torch.exp(-t * t / (2 * SIGMA * SIGMA))
    img = 2e4 * p[:, None] * p[None, :] + 10.0 * torch.randn((NY, NX), device=dev, generator=g)
    c = torch.arange(PITCH // 2, NY, PITCH, device=dev, dtype=torch.int32)
    ys, xs = c.repeat_interleave(c.numel()), c.repeat(c.numel())
    mask = torch.zeros((NY, NX), dtype=torch.uint8, device=dev)
    mask[::997, ::991] = 1                                           # a few flagged windows
    return img.contiguous(), mask, ys.contiguous(), xs.contiguous()


def launches(ctx, torch, a):
    from blackbox_amd import settings, zogy as G
    img, mask, ys_all, xs_all = lattice(ctx, torch)
    nsy, nsx = NY // SIZE, NX // SIZE
    sigw = torch.full((nsy * nsx,), SIGMA, dtype=torch.float32, device=ctx.device)
    out = {}
    for n in (10 ** 4, 10 ** 5):
        ys, xs = ys_all[:n].contiguous(), xs_all[:n].contiguous()
        off = G.win_centroid(ctx, img, ys, xs, sigw, SIZE, nsy, nsx)
        flux = torch.full((n,), 1e5, dtype=torch.float32, device=ctx.device)
        err = torch.full((n,), 1e3, dtype=torch.float32, device=ctx.device)
        shp, fl = G.src_shapes(ctx, img, mask, ys, xs, off, sigw, SIZE, nsy, nsx)
        tab = G.shape_stats(ctx, ys, xs, shp, fl, flux, err, SIZE, nsy, nsx)
        ctx.sync()
        row = tab[-1].cpu().numpy()
        legs = {'bbx_src_shapes': lambda: G.src_shapes(ctx, img, mask, ys, xs, off, sigw, SIZE, nsy, nsx),
                'bbx_shape_stats': lambda: G.shape_stats(ctx, ys, xs, shp, fl, flux, err, SIZE, nsy, nsx),
                'bbx_win_centroid': lambda: G.win_centroid(ctx, img, ys, xs, sigw, SIZE, nsy, nsx)}
        res = dict(sources=n, with_shape=int(torch.isfinite(shp[:, 5]).sum()), qualifying=int(row[0]), stride=int(row[1]),
                   med_fwhm=float(row[3]), radius=settings.centroid_radius, niter=settings.centroid_niter, launches_per_sample=a.launches)
        for name, fn in legs.items():
            for _ in range(a.warmup):
                fn()
            ctx.sync()
            t = []
            for _ in range(a.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                ctx.sync()
                t.append(e0.elapsed_time(e1) / a.launches)
            res[name + '_ms_per_launch'] = stats(t)
        out['n%d' % n] = res
    return out


def frames(ctx, torch, a):
    import thumbs_bench as T
    from blackbox_amd import zogy as G
    data, mask, kw = T.scene(ctx)
    res = G.optimal_subtraction(ctx, data, new_mask=mask, shapes=True, **kw)
    ctx.sync()
    kw = dict(kw, ref_bkg_std=res['bkg_std_ref'])                 # both legs: the reference's sigma map as a run keeps it
    hn = res['header_new']
    info = dict(sources=len(res['catalog']['X_POS']), with_shape=int((res['catalog']['FWHM'] == res['catalog']['FWHM']).sum()),
                n_good=res['shapes']['n_good'], header={k: hn[k][0] for k in hn if k.startswith('S-')})
    del res
    legs = {'off': dict(shapes=False), 'on': dict(shapes=True)}
    times = {k: [] for k in legs}

    def frame(leg, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = G.optimal_subtraction(ctx, data, new_mask=mask, **kw, **legs[leg])
        e1.record()
        ctx.sync()
        del r
        if timed:
            times[leg].append(e0.elapsed_time(e1))
    for _ in range(a.warmup):
        for leg in legs:
            frame(leg, False)
    for _ in range(a.frames):
        for leg in legs:
            frame(leg, True)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each call, legs '
                    '(shapes off / on) alternating in one process', warmup_per_leg=a.warmup, **info,
               optimal_subtraction_ms={k: stats(v) for k, v in times.items()})
    out['added_ms_per_frame'] = statistics.median(times['on']) - statistics.median(times['off'])
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / statistics.median(times['off'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shapes.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20, help='back-to-back launches per timed sample')
    ap.add_argument('--no-frame', action='store_true', help='only the two launches')
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('shapes_bench.py needs a GPU: nothing is measured without one')
    from blackbox_amd import reduce as R
    ctx = R.Context(0)
    out = dict(launches=launches(ctx, torch, a))
    if not a.no_frame:
        out['frame'] = frames(ctx, torch, a)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
