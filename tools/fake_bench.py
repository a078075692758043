"""What the fake stars (zogy.optimal_subtraction(fake_stars=N)) cost, and what comes back of them.

    python tools/fake_bench.py [--out profiles/fakestars.json] [--warmup 10] [--frames 30] [--stars 16] [--s2n 3,5,7,10,20]

A frame of the benchmark's scene (tools/thumbs_bench.scene: 10560 x 10560, cat_extract and trans_extract on in both legs)
through zogy.optimal_subtraction
  off: without the keyword (no kernel of bbx_fake.hip is launched: the parent's path)
  on : fake_stars=[stars] per sub-image (1024 in the frame at 16) of the S/N values [s2n] in turn
alternating, in this one process: each call between two HIP events, [warmup] untimed calls of each leg first, the median of
[frames] calls per leg.  Then the two entries by themselves, each between two HIP events with the host's part inside:
  inject  : zogy.fake_inject of the on leg's layout into a fresh copy of the off leg's background-subtracted frame (the copy is
            made outside the events: a frame that carries the stars already would flag every one of them FAKE_ON_SOURCE)
  recover : zogy.fake_recover on the on leg's Scorr, Fpsf, Fpsferr
and the recovery the on leg's header states: the shares found per asked S/N, T-FKFRAT, T-FKFSTD, T-FKPULL, T-FKSCRT.
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
    data, mask, kw = T.scene(ctx)
    s2n = G.fake_s2n_list(a.s2n)
    legs = {'off': dict(kw), 'on': dict(kw, fake_stars=a.stars, fake_s2n=s2n)}
    off = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['off'])
    res = G.optimal_subtraction(ctx, data, new_mask=mask, **legs['on'])
    ctx.sync()
    for leg in legs.values():
        leg['ref_bkg_std'] = res['bkg_std_ref'] if 'bkg_std_ref' in res else None          # the reference's sigma map as a run keeps it
    ht, fk = res['header_trans'], res['fakestars']
    tab, lay = fk['table'], fk['layout']
    size = kw['subimage_size']
    nsy, nsx = data.shape[0] // size, data.shape[1] // size
    psf_new = kw['psf_new']
    sub_pn = G.subimage_psfs(ctx, psf_new, nsy, nsx, size).contiguous()
    ok = tab['FLAGS_IN'] == 0
    per = {}
    for k, s in enumerate(s2n):
        sel = ok & (np.arange(ok.size) % len(s2n) == k)
        per['%g' % s] = dict(injected=int(sel.sum()), peak_above_threshold=float(((tab['FOUND'][sel] & 1) != 0).mean()),
                             found_as_candidate=float(((tab['FOUND'][sel] & 2) != 0).mean()), in_final_table=float(((tab['FOUND'][sel] & 4) != 0).mean()),
                             median_scorr=float(np.median(tab['SCORR_OUT'][sel])),
                             median_flux_out_over_real=float(np.median(tab['E_FLUX_OUT'][sel] / tab['E_FLUX_REAL'][sel])),
                             median_flux_out_at_over_real=float(np.median(tab['E_FLUX_OUT_AT'][sel] / tab['E_FLUX_REAL'][sel])))
    info = dict(stars_per_subimage=int(a.stars), stars=int(ok.size), injected=int(ok.sum()), flags_in=np.bincount(tab['FLAGS_IN'], minlength=17).tolist(),
                s2n=list(s2n), stamp_side=int(sub_pn.shape[1]), sub_images=int(nsy * nsx), radius=int(settings.fakestar_radius),
                sigma_form='mini image' if isinstance(res['bkg_std'], G.MiniImage) else 'frame',
                header={k: ht[k][0] for k in ht if k.startswith(('T-FK', 'T-NFAKE', 'T-FAKESN', 'T-NFKTR', 'T-NTRANS', 'T-NSIGMA'))},
                ntrans_off=off['header_trans']['T-NTRANS'][0], per_s2n=per)
    base, rwork, bstd = off['data_bkgsub'], off['ref_bkgsub'], off['bkg_std']
    ref_mask = kw.get('ref_mask')
    if ref_mask is not None and tuple(ref_mask.shape) != tuple(base.shape):
        ref_mask = None
    scorr, fpsf, fpsferr = res['Scorr'], res['Fpsf'], res['Fpsferr']
    del res, off
    times = {k: [] for k in legs}
    stage = {'inject': [], 'recover': []}

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
        fresh = base.clone()
        ctx.sync()
        timed(lambda: G.fake_inject(ctx, fresh, rwork, bstd, mask, ref_mask, psf_new, sub_pn, lay, nsx, size, clear_half=settings.fake_clear_half,
                                    clear_nsigma=settings.fake_clear_nsigma, noise=settings.fakestar_noise, seed=lay['seed']),
              stage['inject'] if keep else None)
        del fresh
        timed(lambda: G.fake_recover(ctx, scorr, fpsf, fpsferr, lay, settings.fakestar_radius), stage['recover'] if keep else None)
    out = dict(what='zogy.optimal_subtraction(cat_extract=True, trans_extract=True) on bench.py\'s 10560 x 10560 scene, HIP events around each '
                    'call, legs (fake_stars off / on) alternating in one process; the two entries alone with their host part',
               warmup_per_leg=a.warmup, **info, optimal_subtraction_ms={k: stats(v) for k, v in times.items()},
               stage_ms={k: stats(v) for k, v in stage.items()})
    med = {k: statistics.median(v) for k, v in times.items()}
    out['added_ms_per_frame'] = med['on'] - med['off']
    out['added_fraction_of_off'] = out['added_ms_per_frame'] / med['off']
    out['stages_added_ms'] = statistics.median(stage['inject']) + statistics.median(stage['recover'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fakestars.json'))
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--stars', type=int, default=16)
    ap.add_argument('--s2n', default='3,5,7,10,20')
    a = ap.parse_args()
    if a.warmup < 10 or a.frames < 30:
        ap.error('at least 10 warm-up and 30 timed samples per leg')
    import torch
    if not torch.cuda.is_available():
        sys.exit('fake_bench.py needs a GPU: nothing is measured without one')
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
