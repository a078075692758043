"""CPU: bench.py's --dump-outputs writer (dump_outputs) on host tensors -- float32 / float64 .npy files, the image products
as a fixed sample of their pixels, the small products whole, within the size bound -- and its check of --steps."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                   # noqa: E402


def _frame(ny, nx, with_sub=True):
    g = torch.Generator().manual_seed(3)
    sub = None
    if with_sub:
        sub = {k: torch.randn(ny, nx, generator=g) for k in ('D', 'Scorr', 'Fpsf', 'Fpsferr')}
        sub.update(bkg_mini_new=np.full((8, 12), 250.0, np.float32), bkg_std_mini_new=np.full((8, 12), 18.0, np.float32),
                   catalog=dict(X_POS=np.arange(5, dtype=np.float32) + 1, Y_POS=np.arange(5, dtype=np.float32) + 2,
                                E_FLUX_OPT=np.linspace(10, 50, 5).astype(np.float32)),
                   transients=[dict(y=7, x=9, scorr=6.5, fpsf=120.0, fpsferr=11.0)],
                   header_new={'S-BKG': (250.0, '')}, data_bkgsub=None)
    return types.SimpleNamespace(data=torch.randn(ny, nx, generator=g),
                                 mask=torch.randint(0, 64, (ny, nx), generator=g, dtype=torch.uint8), sub=sub)


def test_dump_outputs_files(tmp_path):
    f = _frame(1500, 1700)
    shapes = bench.dump_outputs(str(tmp_path / 'a'), f)
    bench.dump_outputs(str(tmp_path / 'b'), f)
    names = {'sample_index', 'red', 'mask', 'D', 'Scorr', 'Fpsf', 'Fpsferr', 'bkg_mini', 'bkg_std_mini',
             'cat_X_POS', 'cat_Y_POS', 'cat_E_FLUX_OPT', 'trans_y', 'trans_x', 'trans_scorr', 'trans_fpsf', 'trans_fpsferr'}
    assert set(shapes) == names
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(n + '.npy' for n in names)
    got = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in names}
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64), n
        assert list(a.shape) == shapes[n], n
        assert np.array_equal(a, np.load(str(tmp_path / 'b' / (n + '.npy')))), n      # the same sample in every run
    idx = got['sample_index'].astype(np.int64)
    assert idx.size > 0.5 * min(f.data.numel(), bench.DUMP_SAMPLE) and np.all(np.diff(idx) > 0)
    assert np.array_equal(got['red'], f.data.reshape(-1).numpy()[idx])
    assert np.array_equal(got['mask'], f.mask.reshape(-1).numpy()[idx].astype(np.float32))
    assert np.array_equal(got['Fpsferr'], f.sub['Fpsferr'].reshape(-1).numpy()[idx])
    assert np.array_equal(got['bkg_std_mini'], f.sub['bkg_std_mini_new'])
    assert np.array_equal(got['cat_Y_POS'], f.sub['catalog']['Y_POS'])
    assert got['trans_scorr'].tolist() == [6.5] and got['trans_x'].tolist() == [9.0]


def test_dump_outputs_without_subtraction(tmp_path):
    assert set(bench.dump_outputs(str(tmp_path), _frame(40, 50, with_sub=False))) == {'sample_index', 'red', 'mask'}


def test_dump_outputs_fits_the_bound_at_full_size():
    # a 10560 x 10560 frame: the index (float64) and six sampled images (float32), the small products well below 1 MB
    assert bench.DUMP_SAMPLE * (8 + 6 * 4) + (1 << 20) <= bench.DUMP_LIMIT


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr
