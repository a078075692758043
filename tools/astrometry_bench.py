"""What the astrometric solution from a star catalogue (zogy.optimal_subtraction(astrometry=True)) costs.

    python tools/astrometry_bench.py [--out profiles/astrometry.json] [--warmup 10] [--frames 30]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (no kernel of bbx_wcs.hip is launched: the parent's path), the reference's sigma map kept as a run keeps it
  on : astrometry=True against a catalogue of the frame's own sources -- their positions through a TAN projection about a pointing
       that is POINTING_ERR pixels off, rotated and scaled a little -- plus as many rows without a star: the catalogue's list, the
       vote, the fits and match rounds, the residuals, RA / DEC of every catalogue and transient row, every frame
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then by themselves on that frame, between two HIP events with the host's part inside:
  cat_list      : bbx_wcs_cat_list over the catalogue, and over one of 2 000 000 rows (cat_list_2M)
  pix2sky       : bbx_wcs_pix2sky at the catalogue's rows
  pair_stats    : bbx_wcs_pair_stats over the last fit's pairs
  enqueue       : astrometry.solve_enqueue: everything the solve queues, no host wait
  solve         : astrometry.solve: the same and its one copy back -- solve minus enqueue is the host wait a caller without a copy
                  back of its own would pay (optimal_subtraction rides the photometry's and pays none)
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

POINTING, POINTING_ERR, ROT, SCALE, PIXSCALE = (120.0, -30.0), (31.0, -22.0), 0.05, 1.0003, 0.564


def stats(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), min_ms=v[0], max_ms=v[-1], p25_ms=v[len(v) // 4], p75_ms=v[(3 * len(v)) // 4], n=len(v))


def frames(ctx, torch, a):
    import numpy as np
    import thumbs_bench as T
    import astrometry_ref as W                                       # (the projection in numpy, for the catalogue's truth)
    from blackbox_amd import astrometry as AST, zogy as G
    data, mask, kw = T.scene(ctx)
    ny, nx = data.shape
    first = G.optimal_subtraction(ctx, data, new_mask=mask, **kw)
    ctx.sync()
    cat0 = first['catalog']
    rs = np.random.RandomState(1)
    x, y = cat0['X_POS'].astype(np.float64) - 1.0, cat0['Y_POS'].astype(np.float64) - 1.0
    n = x.size
    x, y = np.concatenate([x, rs.uniform(0, nx - 1, n)]), np.concatenate([y, rs.uniform(0, ny - 1, n)])
    flux = np.concatenate([np.maximum(cat0['E_FLUX_OPT'], 1.0), 10 ** rs.uniform(2, 5, n)])
    ra, dec = W.true_sky(x, y, (ny, nx), POINTING, PIXSCALE, tangent_offset=(POINTING_ERR[0] * PIXSCALE / 3600.0, POINTING_ERR[1] * PIXSCALE / 3600.0),
                         rot=ROT, scale=SCALE, quad=1e-9)
    order = rs.permutation(ra.size)
    cat = AST.AstCatalog(ctx, ra[order], dec[order], (25.0 - 2.5 * np.log10(flux[order])).astype(np.float32), name='bench')
    big = AST.AstCatalog(ctx, np.resize(ra, 2000000), np.resize(dec, 2000000), np.resize(25.0 - 2.5 * np.log10(flux), 2000000), name='2M')
    legs = {'off': dict(kw, ref_bkg_std=first.get('bkg_std_ref')),
            'on': dict(kw, ref_bkg_std=first.get('bkg_std_ref'), astrometry=True, ast_catalog=cat, ast_pointing=POINTING, ast_pixscale=PIXSCALE)}
    on = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    sol = on['astrometry']
    if sol is None or not sol['ok']:
        sys.exit('the solve failed on the benchmark scene: %s' % (None if sol is None else sol['fit']))
    h = on['header_new']
    size = kw['subimage_size']
    nsy, nsx = ny // size, nx // size
    sig = on['bkg_std'].frame(ctx) if isinstance(on['bkg_std'], G.MiniImage) else on['bkg_std']
    new_stars = G.RefStars(ctx, on['data_bkgsub'], sig, mask, G.subimage_psfs(ctx, kw['psf_new'], nsy, nsx, size).contiguous(), nsy, nsx, size,
                           sigma_median=h['S-BKGSTD'][0])
    alone = AST.solve(ctx, new_stars.lists(), cat, POINTING, (ny, nx), pixscale=PIXSCALE)
    pend, cd = alone['pending'], AST.cd0(PIXSCALE)
    info = dict(catalogue_rows=cat.n, frame_sources=new_stars.n, rows_with_sky=int(len(on['catalog']['RA'])),
                transients=dict(off=len(first['transients']), on=len(on['transients'])),
                header={k: v[0] for k, v in h.items() if k.startswith('A-') or k in ('RA-CNTR', 'DEC-CNTR', 'CTYPE1', 'CRPIX1', 'CRPIX2')})
    del first, on, sig
    times = {k: [] for k in legs}
    calls = {'cat_list': lambda: AST.cat_list(ctx, cat, POINTING, (ny, nx), cd, 272.0),
             'cat_list_2M': lambda: AST.cat_list(ctx, big, POINTING, (ny, nx), cd, 272.0),
             'pix2sky': lambda: AST.pix2sky(ctx, pend['coef'], (ny, nx), cd, POINTING, ys=pend['b'][0], xs=pend['b'][1], off=pend['b'][2]),
             'pair_stats': lambda: AST.pair_stats(ctx, pend['items'], pend['kept'], new_stars.lists(), cat, pend['coef'], (ny, nx), cd, POINTING),
             'enqueue': lambda: AST.solve_enqueue(ctx, new_stars.lists(), cat, POINTING, (ny, nx), pixscale=PIXSCALE),
             'solve': lambda: AST.solve(ctx, new_stars.lists(), cat, POINTING, (ny, nx), pixscale=PIXSCALE)}
    stage = {k: [] for k in calls}

    def timed(fn, sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        ctx.sync()
        del r
        if sink is not None:
            sink.append(e0.elapsed_time(e1))
    for it in range(a.warmup + a.frames):
        keep = it >= a.warmup
        for leg in legs:
            timed(lambda: G.optimal_subtraction(ctx, data, new_mask=mask, **legs[leg]), times[leg] if keep else None)
        for name, fn in calls.items():
            timed(fn, stage[name] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (astrometry off / on) alternating in one process; the kernels and the solve alone on that frame',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    out['host_wait_ms'] = statistics.median(stage['solve']) - statistics.median(stage['enqueue'])
    out['cat_list_2M_GBps'] = 2000000 * 44.0 / (statistics.median(stage['cat_list_2M']) * 1e-3) / 1e9       # 20 bytes in, 24 out per row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'astrometry.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('astrometry_bench.py needs a GPU: nothing is measured without one')
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
