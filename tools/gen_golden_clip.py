#!/usr/bin/env python3
"""Golden vectors of the clipped statistics, the LDS sort and the workgroup sums: tests/golden/clip_pins.npz.

Run ONCE, on a GPU, on a build of the commit BEFORE the shared primitives (lds_sort, wg_sum_tree, wg_sum_seq of bbx_common.h;
stats_clip<BLOCK> of bbx_stats.h) -- BBX_LIB_PATH may name that build's libbbx_hip.so.  It stores what bbx_match_stats,
bbx_shape_stats, bbx_aper_phot and bbx_align_vote made of the cases of tests/test_gpu_clip_pins.py, which builds the inputs
(from seeds) for this script and for the test alike.  The test asserts the same bytes from the tree it runs in; if it fails,
an addition has moved: the kernels are to be fixed, and this script is not to be run again.

    python tools/gen_golden_clip.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out):
    import test_gpu_clip_pins as P
    from blackbox_amd import reduce as R
    from blackbox_amd._lib import LIB_PATH
    ctx = R.Context(0)
    pins = {}
    pins.update(P.match_pins(ctx))
    pins.update(P.shape_pins(ctx))
    pins.update(P.aper_pins(ctx, P.TP.case.__wrapped__()))          # (the fixtures' plain functions)
    pins.update(P.vote_pins(ctx, P.TA.scene.__wrapped__()))
    ctx.close()
    np.savez_compressed(out, **pins)
    print('{}: {} arrays from {}, {} bytes'.format(out, len(pins), LIB_PATH, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'clip_pins.npz'))
