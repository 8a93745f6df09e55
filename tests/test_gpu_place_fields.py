"""cobel_activity_process and cobel_place_fields (csrc/activity.hip) against the NumPy restatement
of tests/activity_common.py, bit for bit (np.array_equal with equal_nan) on every output, in both
dtypes, with sentinels around every output.  tests/test_host_activity.py holds the restatement
against scipy.ndimage, which defines the numbering of the components."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activity_common as ac  # noqa: E402

from mlp_gpu_common import DEV, SENTINEL_U8, Framed, _dev, _host, _np, _torch_dtype  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ['f64', 'f32']
SHAPES = [(1, 1), (1, 8), (8, 1), (5, 7), (25, 25), (32, 32), (64, 64)]
I32_SENTINEL = -77777


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert DEV != 'cuda' or torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def _classify(torch, maps, name, size_threshold=0.5, cutoff=0.25):
    """cobel_place_fields on maps [M, H, W]: the five outputs as NumPy arrays, frames checked."""
    from cobel_amd import _lib
    M, H, W = maps.shape
    has = Framed(torch, (M,), torch.uint8, fill=SENTINEL_U8)
    ints = [Framed(torch, (M,), torch.int32, fill=I32_SENTINEL) for _ in range(3)]
    fields = Framed(torch, (M, H, W), _torch_dtype(torch, name))
    d_maps = _dev(torch, maps)
    before = d_maps.clone()
    _lib.check(_lib.lib().cobel_place_fields(
        _lib.ptr(d_maps), M, H, W, int(name == 'f64'), cutoff, size_threshold, _lib.ptr(has.view),
        *[_lib.ptr(f.view) for f in ints], _lib.ptr(fields.view), None))
    torch.cuda.synchronize()
    assert has.intact() and fields.intact() and all(f.intact() for f in ints)
    assert _host(d_maps).tobytes() == _host(before).tobytes()          # the maps are read only
    return (_host(has.view),) + tuple(_host(f.view) for f in ints) + (_host(fields.view),)


def _same(got, want, where):
    for g, w, what in zip(got, want, ('has_field', 'error', 'features', 'largest_area', 'fields')):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, what)
        assert np.array_equal(g, w, equal_nan=True), (where, what, g, w)


@pytest.mark.parametrize('H,W', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_named_maps(torch_cuda, name, H, W):
    named = ac.named_maps(H, W, _np(name))
    names = sorted(named)
    maps = np.stack([named[k] for k in names])
    _classify(torch_cuda, maps[:1], name)                             # (the kernel is loaded)
    start = time.perf_counter()
    got = _classify(torch_cuda, maps, name)
    seconds = time.perf_counter() - start
    _same(got, ac.classify_many(maps), (H, W, names))
    for k, key in enumerate(names):                                   # each map alone: the same
        alone = _classify(torch_cuda, maps[k:k + 1], name)
        _same(alone, tuple(g[k:k + 1] for g in got), (H, W, key))
    # a serpentine must not cost rounds in proportion to its length: one launch of all the maps,
    # allocation and copies included, stays far below a second
    assert seconds < 1.0, seconds


@pytest.mark.parametrize('name', DTYPES)
def test_other_thresholds(torch_cuda, name):
    named = ac.named_maps(5, 7, _np(name))
    maps = np.stack([named[k] for k in sorted(named)])
    for size, cutoff in ((0.3, 0.1), (0.9, 0.5), (0.05, 0.75)):
        _same(_classify(torch_cuda, maps, name, size, cutoff), ac.classify_many(maps, size, cutoff),
              (size, cutoff))


@pytest.mark.parametrize('M', [1, 63, 64, 65])
@pytest.mark.parametrize('name', DTYPES)
def test_many_maps_in_one_launch(torch_cuda, name, M):
    rng = np.random.default_rng(M)
    maps = (rng.uniform(0, 1, (M, 9, 11)) * (rng.random((M, 9, 11)) < 0.4)).astype(_np(name))
    got = _classify(torch_cuda, maps, name)
    _same(got, ac.classify_many(maps), M)
    for k in (0, M // 2, M - 1):
        _same(_classify(torch_cuda, maps[k:k + 1], name), tuple(g[k:k + 1] for g in got), (M, k))


@pytest.mark.parametrize('name', DTYPES)
def test_random_sweep(torch_cuda, name):
    """The seeded sweep the semantics were settled on (1 x 1 .. 8 x 8, three cutoffs, two size
    thresholds), 300 cases, grouped by shape and thresholds into launches."""
    groups = {}
    for a, cutoff, size in ac.random_maps(2024, 300, _np(name)):
        groups.setdefault((a.shape, cutoff, size), []).append(a)
    hit = set()
    for (shape, cutoff, size), maps in sorted(groups.items()):
        maps = np.stack(maps)
        got = _classify(torch_cuda, maps, name, size, cutoff)
        _same(got, ac.classify_many(maps, size, cutoff), (shape, cutoff, size))
        hit.update(int(e) for e in got[1])
    assert hit == {0, 1, 2, 3}


@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 625])
@pytest.mark.parametrize('name', DTYPES)
def test_process(torch_cuda, name, P):
    torch = torch_cuda
    from cobel_amd import _lib
    rows = ac.process_rows(P, _np(name))
    for R in (1, 3, 4, 5, len(rows)):
        for threshold in (0.15, 0.0, 0.5):
            frame = Framed(torch, (R, P), _torch_dtype(torch, name))
            frame.view.copy_(_dev(torch, rows[:R]))
            _lib.check(_lib.lib().cobel_activity_process(_lib.ptr(frame.view), R, P,
                                                         int(name == 'f64'), threshold, None))
            torch.cuda.synchronize()
            assert frame.intact()
            want = ac.process(rows[:R], threshold)
            got = _host(frame.view)
            assert got.dtype == want.dtype
            assert np.array_equal(got, want, equal_nan=True), (P, R, threshold, got, want)


@pytest.mark.parametrize('name', DTYPES)
def test_analysis_surface(torch_cuda, name):
    """cobel_amd.analysis.network_spatial on ndarrays and on device tensors."""
    torch = torch_cuda
    from cobel_amd.analysis import network_spatial as ns
    rows = ac.process_rows(625, _np(name))[[0, 1, 7]]
    want = ac.process(rows, 0.2)
    mine = rows.copy()
    assert ns.process_activity_maps(mine, 0.2) is mine and np.array_equal(mine, want)
    cube = _dev(torch, rows.reshape(3, 1, 625))
    assert ns.process_activity_maps(cube, 0.2) is cube
    assert np.array_equal(_host(cube).reshape(3, 625), want)
    named = ac.named_maps(5, 7, _np(name))
    for key in ('blob', 'blobs5', 'zero', 'ell'):
        has, field = ns.classify_place_field(named[key])
        ref = ac.classify(named[key])
        assert has is ref[0] and field.dtype == ref[1].dtype and np.array_equal(field, ref[1])
    maps = np.stack([named[k] for k in sorted(named)][:16]).reshape(2, 8, 5, 7)
    has, fields, info = ns.classify_place_fields(maps)
    ref = ac.classify_many(maps.reshape(-1, 5, 7))
    assert has.dtype == np.bool_ and np.array_equal(has.reshape(-1), ref[0].astype(bool))
    assert np.array_equal(fields.reshape(-1, 5, 7), ref[4], equal_nan=True)
    for k, r in (('error', ref[1]), ('features', ref[2]), ('largest_area', ref[3])):
        assert np.array_equal(info[k].reshape(-1), r)
    on_device = ns.classify_place_fields(_dev(torch, maps))
    assert on_device[1].is_cuda and np.array_equal(_host(on_device[1]), fields, equal_nan=True)
