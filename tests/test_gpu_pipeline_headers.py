"""GPU: the header cards a FramePipeline run leaves on its frames -- key, value and comment of every card of f.header and f.hm
in the order they were written (the card order of the FITS files), and f.failed -- for five runs of four frames each, against
tests/golden/pipeline_headers.json.  The fixture was recorded with record() below on the parent commit of the change that split
the device stage into stage methods and gave 'step X failed -> headers' one home (reduce.step_failed); two recordings there were
equal card by card, so no value is left out of the comparison.  And the host waits of a four-frame run with a small subtraction."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import bbx_oracle as O                                  # noqa: E402
from blackbox_amd import _lib, synth                    # noqa: E402
from blackbox_amd import reduce as R                    # noqa: E402
from blackbox_amd.pipeline import FramePipeline, HostPool   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pipeline_headers.json')
NFRAMES = 4

# name: telescope, channel rows, channel columns, trail search
SCENARIOS = {
    'ml1_sats': ('ML1', 96, 330, True),
    'bg3_two_phase': ('BG3', 2640, 330, False),          # the saturated-column step between two rounds of host fits
    'fits_fail': ('ML1', 96, 330, False),                # the host fits of frame 2 fail as a whole: results is None
    'partial_overscan': ('ML1', 96, 256, False),         # channels narrower than 300 columns: os_corr raises on channel 1
    'step_failures': ('ML1', 96, 330, True),             # frame 1: the cosmics step, frame 2: the trail step fail on the host side
}
# keys whose VALUE differed between two recordings on the parent commit (position and comment are still compared): none did
VOLATILE = ()


class FailingFits:
    """a HostPool whose result for the [frame]-th submitted set of fits raises in get()"""

    class _Raises:
        def __init__(self, res):
            self.res = res

        def ready(self):
            return self.res.ready()

        def wait(self, timeout=None):
            return self.res.wait(timeout)

        def get(self, timeout=None):
            self.res.get(timeout)                        # (the workers have finished with the slot's arena)
            raise RuntimeError('injected: the host fits of this frame failed')

    def __init__(self, pool, frame):
        self.pool, self.frame, self.nsubmitted = pool, frame, 0

    def submit(self, fn, tasks):
        res = self.pool.submit(fn, tasks)
        self.nsubmitted += 1
        return self._Raises(res) if self.nsubmitted - 1 == self.frame else res


def cards(d):
    """[key, value, comment] of every card in the order the keys entered the dict"""
    out = []
    for k, v in d.items():
        v, comment = v if isinstance(v, tuple) else (v, None)
        out.append([k, v.item() if isinstance(v, np.generic) else v, comment])
    return out


def run_scenario(name, ctx, pool, mp, lanes=2, depth=3):
    """-> per frame, in frame order: dict(failed=, header=, hm=) as they are at on_done; mp: a pytest.MonkeyPatch"""
    import threading
    tel, ys, xs, sats = SCENARIOS[name]
    dev = ctx.device
    cases = [synth.make_case(ys, xs, 100 + k, tel=tel, os_y=20, os_x=45, n_stars=60, n_sat=4, n_cr=60) for k in range(NFRAMES)]
    raws = [torch.from_numpy(c['raw']).to(dev) for c in cases]
    headers = [{} for _ in raws]
    if name == 'fits_fail':
        pool = FailingFits(pool, 2)
    if name == 'step_failures':
        # the Python calls of the two steps raise what a failed launch raises; the trail step has no frame among its arguments:
        # the cosmics step of the same frame, just before it on the same lane thread, leaves the frame's header for it
        on_lane = threading.local()
        cosmics_corr, sat_trails = R.cosmics_corr, _lib.lib.bbx_sat_trails

        def cosmics(ctx_, data, header, *a, **k):
            on_lane.header = header
            if header is headers[1]:
                raise _lib.BBXError(-1, 'cosmics_corr (injected)')
            return cosmics_corr(ctx_, data, header, *a, **k)

        def trails(*a):
            if on_lane.header is headers[2]:
                raise _lib.BBXError(-1, 'bbx_sat_trails (injected)')
            return sat_trails(*a)
        mp.setattr(R, 'cosmics_corr', cosmics)
        mp.setattr(_lib.lib, 'bbx_sat_trails', trails)
    pipe = FramePipeline(ctx, tel, R.geometry(raws[0].shape, ys, xs), mflat=torch.from_numpy(cases[0]['flat']).to(dev),
                         bpm=torch.from_numpy(cases[0]['bpm']).to(dev), xtalk_coeffs=O.xtalk_coeffs(cases[0]['xtalk']), exptime=60.0,
                         pool=pool, depth=depth, lanes=lanes, do_finish=True, detect_sats=sats)
    got = {}
    try:
        n = pipe.run(list(zip(raws, headers)), on_done=lambda i, f: got.__setitem__(
            i, dict(failed=list(f.failed), header=cards(f.header), hm=cards(f.hm))))
    finally:
        pipe.close()
        mp.undo()
    assert n == NFRAMES and sorted(got) == list(range(NFRAMES))
    return [got[i] for i in range(NFRAMES)]


def pipeline_waits(ctx, pool, mp, lanes=1, depth=3, **more):
    """four frames with the 'frame' scene of test_gpu_subtraction_waits as their subtraction (96 x 144 px: 2 x 8 channels of
    48 x 18), one lane -> (host waits inside _lib.fetch, calls of lib.bbx_wait, calls of lib.bbx_sync) over pipe.run; more: further
    arguments of the pipeline"""
    import test_gpu_subtraction_waits as W
    sc = W.make_scene(**W.SCENES['frame'])
    ys, xs = sc['shape'][0] // 2, sc['shape'][1] // 8
    dev = ctx.device
    cases = [synth.make_case(ys, xs, 100 + k, tel='ML1', os_y=20, os_x=45, n_stars=10, n_sat=1, n_cr=5) for k in range(NFRAMES)]
    raws = [torch.from_numpy(c['raw']).to(dev) for c in cases]
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ('ref', 'mask_ref', 'psf_new', 'psf_ref')}
    sub = dict(sc['kw'], ref=d['ref'], ref_mask=d['mask_ref'], psf_new=d['psf_new'], psf_ref=d['psf_ref'])
    calls = []                                           # (list.append: safe from the lane thread and the caller's at once)
    for fn in ('bbx_wait', 'bbx_sync'):
        mp.setattr(_lib.lib, fn, lambda *a, fn=fn, real=getattr(_lib.lib, fn): (calls.append(fn), real(*a))[1])
    pipe = FramePipeline(ctx, 'ML1', R.geometry(raws[0].shape, ys, xs), mflat=torch.from_numpy(cases[0]['flat']).to(dev),
                         bpm=torch.from_numpy(cases[0]['bpm']).to(dev), xtalk_coeffs=O.xtalk_coeffs(cases[0]['xtalk']), exptime=60.0,
                         pool=pool, depth=depth, lanes=lanes, do_finish=True, subtract=sub, **more)
    failed = {}
    try:
        ctx.sync()
        n0, c0 = _lib.WAIT_STATS[1], len(calls)
        n = pipe.run([(r, {}) for r in raws], on_done=lambda i, f: failed.__setitem__(i, list(f.failed)))
        waits, during = _lib.WAIT_STATS[1] - n0, calls[c0:]
    finally:
        pipe.close()
        mp.undo()
    assert n == NFRAMES and failed == {i: [] for i in range(NFRAMES)}, failed
    return waits, during.count('bbx_wait'), during.count('bbx_sync')


def record(path):
    """what made the fixture: every scenario once -> path"""
    ctx, pool = R.Context(0), HostPool(4)
    try:
        with pytest.MonkeyPatch.context() as mp:
            rec = {name: run_scenario(name, ctx, pool, mp) for name in SCENARIOS}
    finally:
        pool.close()
        ctx.close()
    write_fixture(path, rec)


def write_fixture(path, rec):
    """one card per line: {scenario: [per frame {"failed": [...], "header": [card, ...], "hm": [card, ...]}]}"""
    def frame(fr):
        parts = ['   "failed": ' + json.dumps(fr['failed'])]
        parts += ['   "%s": [\n%s\n   ]' % (k, ',\n'.join('    ' + json.dumps(c) for c in fr[k])) for k in ('header', 'hm')]
        return '  {\n' + ',\n'.join(parts) + '\n  }'
    with open(path, 'w') as fh:
        fh.write('{\n' + ',\n'.join(' %s: [\n%s\n ]' % (json.dumps(name), ',\n'.join(frame(fr) for fr in rec[name]))
                                    for name in sorted(rec)) + '\n}\n')


@pytest.fixture(scope='module')
def pool():
    p = HostPool(4)
    yield p
    p.close()


@pytest.fixture(scope='module')
def ctx():
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_headers_equal_the_recorded_ones(ctx, pool, golden, monkeypatch, name):
    got = run_scenario(name, ctx, pool, monkeypatch)
    want = golden[name]
    assert len(want) == NFRAMES
    if name == 'fits_fail':
        assert dict(map(tuple, (c[:2] for c in got[2]['header'])))['OS-P'] is False          # the scene is what it says
    if name == 'partial_overscan':
        assert all('BIAS1A0' in [c[0] for c in g['header']] and 'BIAS2A0' not in [c[0] for c in g['header']] for g in got)
    if name == 'step_failures':
        assert [g['failed'] for g in got] == [[], ['cosmics'], ['sat'], []]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g['failed'] == w['failed'], (name, i)
        for which in ('header', 'hm'):
            # (as JSON text: what the fixture holds; NaN equals NaN, True is not 1, 10.0 is not 10)
            line = lambda c: json.dumps([c[0], None, c[2]] if c[0] in VOLATILE else c)      # noqa: E731
            gl, wl = [line(c) for c in g[which]], [line(c) for c in w[which]]
            assert [json.loads(s)[0] for s in gl] == [json.loads(s)[0] for s in wl], (name, i, which, 'card order')
            assert gl == wl, (name, i, which, [(a, b) for a, b in zip(gl, wl) if a != b][:4])


# host waits of the four-frame run, MEASURED ON THE PARENT COMMIT of the change named above (two runs there gave the same
# counts): (waits inside _lib.fetch, calls of lib.bbx_wait, calls of lib.bbx_sync)
PIPELINE_WAITS = (16, 12, 4)


def test_host_waits_of_a_pipeline_run(ctx, pool, monkeypatch):
    got = pipeline_waits(ctx, pool, monkeypatch)
    assert got == PIPELINE_WAITS, '(fetch waits, bbx_wait, bbx_sync) of %d frames' % NFRAMES
