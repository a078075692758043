"""_lib.Readback on the host: a copy back whose parts have names, over ONE _lib.fetch call (a stub stands in for it here)."""
import numpy as np
import pytest

from blackbox_amd import _lib


@pytest.fixture
def calls(monkeypatch):
    """_lib.fetch replaced by a stub with its return convention: a bare array for one tensor, a list for more"""
    seen = []

    def stub(ctx, *tensors, check_device_errors=False):
        seen.append((ctx, tensors, check_device_errors))
        out = [np.asarray(t) * 10 for t in tensors]
        return out if len(out) > 1 else out[0]
    monkeypatch.setattr(_lib, 'fetch', stub)
    return seen


def test_empty(calls):
    assert _lib.Readback().fetch('ctx') == {}
    assert calls == []                                               # no library call, no host wait


def test_one_tensor_is_a_list_of_one(calls):
    rb = _lib.Readback()
    rb.add('lim', np.arange(3))
    got = rb.fetch('ctx')
    assert list(got) == ['lim'] and isinstance(got['lim'], list) and len(got['lim']) == 1
    assert np.array_equal(got['lim'][0], [0, 10, 20])
    assert len(calls) == 1 and len(calls[0][1]) == 1


def test_many_tensors_in_the_order_they_were_added(calls):
    a, b, c, d, e, f = (np.full(2, k) for k in range(6))
    rb = _lib.Readback()
    rb.add('phot', a, b, c)
    rb.add('aper', *[d, e])
    rb.add('none')                                                   # a name without tensors: an empty list
    rb.add('csky', f)
    got = rb.fetch('ctx', check_device_errors=True)
    assert len(calls) == 1                                           # ONE fetch over all of them
    ctx, tensors, chk = calls[0]
    assert ctx == 'ctx' and chk is True
    assert [t is w for t, w in zip(tensors, (a, b, c, d, e, f))] == [True] * 6 and len(tensors) == 6
    assert list(got) == ['phot', 'aper', 'none', 'csky']
    assert [v[0] for v in got['phot']] == [0, 10, 20] and [v[0] for v in got['aper']] == [30, 40]
    assert got['none'] == [] and [v[0] for v in got['csky']] == [50]
    assert 'aper' in got and 'lim' not in got and got.get('lim') is None


def test_names_without_tensors_make_no_call(calls):
    rb = _lib.Readback()
    rb.add('lim')
    assert rb.fetch('ctx') == {'lim': []} and calls == []


def test_duplicate_name(calls):
    rb = _lib.Readback()
    rb.add('phot', np.zeros(1))
    with pytest.raises(ValueError):
        rb.add('phot', np.ones(1))
    assert [t[0] for t in rb.fetch('ctx')['phot']] == [0]            # the first entry stands
