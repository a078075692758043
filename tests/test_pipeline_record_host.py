"""CPU: the layout of the frame pipeline's per-frame result record (pipeline.RECORD_FIELDS), the named views over one copy of
it, and the cards reduce.step_failed writes for a failed step."""
import pytest

torch = pytest.importorskip('torch')

from blackbox_amd import pipeline as P          # noqa: E402
from blackbox_amd import reduce as R            # noqa: E402


def test_record_layout_is_the_one_the_kernels_fill():
    """std[16] f64 | nobj i32 | stats[16] i32 | nsats i32 | cnt[6] i64 | step error words [8] i32, 288 bytes: the offsets the
    record had when they were written out by hand"""
    assert [name for name, _, _ in P.RECORD_FIELDS] == ['std', 'nobj', 'stats', 'nsats', 'cnt6', 'steps']
    assert {k: v[0] for k, v in P.RECORD_WHERE.items()} == dict(std=0, nobj=128, stats=132, nsats=196, cnt6=200, steps=248)
    assert {k: v[1] for k, v in P.RECORD_WHERE.items()} == dict(std=128, nobj=4, stats=64, nsats=4, cnt6=48, steps=32)
    assert P.RECORD_BYTES == 288
    assert len(R.STEP_SLOTS) == P.RECORD_WHERE['steps'][1] // 4
    for name, (o, nb, dt) in P.RECORD_WHERE.items():
        assert o % dt.itemsize == 0, name                              # every part aligned for its type


def test_views_alias_the_bytes_of_one_buffer():
    buf = torch.zeros(P.RECORD_BYTES, dtype=torch.uint8)
    v = P.record_views(buf)
    assert {k: (t.dtype, t.numel()) for k, t in v.items()} == dict(
        std=(torch.float64, 16), nobj=(torch.int32, 1), stats=(torch.int32, 16), nsats=(torch.int32, 1), cnt6=(torch.int64, 6),
        steps=(torch.int32, 8))
    for name, t in v.items():
        assert t.data_ptr() == buf.data_ptr() + P.RECORD_WHERE[name][0], name
    # a write through a view lands in its own bytes and nowhere else
    v['nobj'][0] = 0x01020304
    v['cnt6'][5] = -1
    v['steps'][7] = 7
    raw = buf.numpy()
    assert raw[128:132].tolist() == [4, 3, 2, 1] and raw[240:248].tolist() == [255] * 8 and raw[276:280].tolist() == [7, 0, 0, 0]
    touched = set(range(128, 132)) | set(range(240, 248)) | {276}
    assert all(raw[i] == 0 for i in range(P.RECORD_BYTES) if i not in touched)
    # and a write into the buffer shows in the view
    raw[0:8] = torch.tensor([10.0], dtype=torch.float64).numpy().view('uint8')
    assert v['std'][0].item() == 10.0


def test_reading_an_absent_part_says_so():
    v = P.record_views(torch.zeros(P.RECORD_BYTES, dtype=torch.uint8))
    rec = P.RecordParts(v, nobj=None, stats=v['stats'], nsats=None)
    assert 'nobj' not in rec and 'nsats' not in rec
    assert all(k in rec for k in ('std', 'stats', 'cnt6', 'steps'))
    assert rec.stats.data_ptr() == v['stats'].data_ptr() and rec.std.data_ptr() == v['std'].data_ptr()
    with pytest.raises(AttributeError, match="no part 'nobj'.*did not run, or failed"):
        rec.nobj
    with pytest.raises(AttributeError, match="no part 'bogus'"):
        rec.bogus
    assert all(k in P.RecordParts(v) for k in P.RECORD_WHERE)          # nothing said: everything is there


def test_step_failed_cards():
    """the one home of 'step X failed -> headers': after the frame's synchronisation the flag, then 'None' in both headers; in
    reduce_object's handler 'None' first and in the image header only; steps without a card of their own leave nothing"""
    for step, flag, count in (('cosmics', 'COSMIC-P', 'NCOSMICS'), ('sat', 'SAT-P', 'NSATS')):
        h, hm = {}, {}
        R.step_failed(h, hm, step)
        assert list(h) == [flag, count] and list(hm) == [count]
        assert h[flag][0] is False and h[count][0] == 'None' and hm[count] == h[count]
        h2, hm2 = {}, {}
        R.step_failed(h2, hm2, step, in_handler=True)
        assert list(h2) == [count, flag] and hm2 == {} and h2[flag] == h[flag] and h2[count] == h[count]
    for step, flag in (('calibrate', 'MASK-P'), ('mask', 'MASK-P'), ('xtalk', 'XTALK-P')):
        for in_handler in (False, True):
            h, hm = {}, {}
            R.step_failed(h, hm, step, in_handler=in_handler)
            assert list(h) == [flag] and h[flag][0] is False and hm == {}
    for step in ('finish', 'bkg', 'zogy'):
        h, hm = {}, {}
        R.step_failed(h, hm, step)
        assert h == {} and hm == {}
    # the device-side flags go through it, in the order of the steps
    h, hm = {}, {}
    assert R.apply_step_errors(h, hm, [0, 1, 1, 0, 1, 0, 0, 1]) == ['mask', 'cosmics', 'sat', 'zogy']
    assert list(h) == ['MASK-P', 'COSMIC-P', 'NCOSMICS', 'SAT-P', 'NSATS'] and list(hm) == ['NCOSMICS', 'NSATS']
