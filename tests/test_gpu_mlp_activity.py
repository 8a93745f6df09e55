"""cobel_mlp_activity (csrc/mlp_fit.hip) against the float64 restatement of
tests/activity_common.py: every layer, every ``apply``, both hidden activations and both dtypes, at
probe counts around the tile of 32 (1, 31, 32, 33, 65), with shared and per-instance probes.

Tolerances are those of the other stacked-network kernels (tests/mlp_gpu_common.agree): float64
rtol 1e-9 / atol 1e-12; float32 within 4x of what torch's float32 on the CPU differs from the
float64 reference by on the same inputs, 64 * 2^-24 as the floor.  What only moves data is exact:
a ``units`` call equals the rows of the full call bit for bit, an instance of a stack equals the
same network alone bit for bit, and the sentinels around ``out`` are intact at every ragged P."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activity_common as ac  # noqa: E402
import mlp_common as mc  # noqa: E402

from mlp_gpu_common import (DEV, Framed, _dev, _host, _launch, _np, _stack_dev,  # noqa: E402
                            _torch_dtype, agree)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (7, 4, 3), (32, 32, 5), (7, 32, 3), (32, 1, 1)]      # D, O, n
PROBES = [1, 31, 32, 33, 65]
DTYPES = ['f64', 'f32']
FIGURES = {}


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert DEV != 'cuda' or torch.cuda.is_available(), 'GPU tests need an MI355X'
    yield torch
    for key in sorted(FIGURES):
        print('mlp-activity figure %s  kernel %.2e  torch-f32 %.2e' % ((key,) + FIGURES[key]))


def _t32_activity(torch, p, x, layer, hidden, apply):
    act = {'relu': torch.relu, 'tanh': torch.tanh, 'none': lambda v: v}
    pre = x @ p['w1'].T + p['b1']
    if layer >= 1:
        pre = act[hidden](pre) @ p['w2'].T + p['b2']
    if layer == 2:
        pre = act[hidden](pre) @ p['w3'].T + p['b3']
    return act[apply](pre).T


def _run(torch, name, dP, probes, n, P, D, O, layer, hidden, apply, units=None):
    from cobel_amd import _lib
    U = O if layer == 2 else mc.H
    K = U if units is None else len(units)
    out = Framed(torch, (n, K, P), _torch_dtype(torch, name))
    d_units = None if units is None else _dev(torch, np.asarray(units, dtype=np.int32))
    run = ac.fill_activity(_lib, dP, probes, out.view, n, P, D, O, layer, hidden, apply,
                           units=d_units, per_instance=probes.dim() == 3)
    _launch('cobel_mlp_activity', run)
    torch.cuda.synchronize()
    assert out.intact(), (P, layer, apply)
    return _host(out.view)


@pytest.mark.parametrize('D,O,n', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_activity_against_the_restatement(torch_cuda, name, D, O, n):
    torch = torch_cuda
    dt = _np(name)
    rng = np.random.default_rng(100 * D + 10 * O + n)
    stack = mc.draw_networks(rng, n, D, O, dt)
    dP = _stack_dev(torch, stack)
    for P in PROBES:
        shared = rng.standard_normal((P, D)).astype(dt)
        own = rng.standard_normal((n, P, D)).astype(dt)
        for probes in (shared, own):
            d_probes = _dev(torch, probes)
            for hidden in ('relu', 'tanh'):
                for layer in (0, 1, 2):
                    for apply in ('none', 'relu', 'tanh'):
                        got = _run(torch, name, dP, d_probes, n, P, D, O, layer, hidden, apply)
                        ref = ac.stack_activity(stack, probes, layer, hidden, apply)
                        assert got.shape == ref.shape
                        for j in range(n):
                            t32 = None
                            if name == 'f32':
                                p32 = {k: torch.from_numpy(stack[k][j]) for k in mc.KEYS}
                                x32 = torch.from_numpy(probes if probes.ndim == 2 else probes[j])
                                t32 = _t32_activity(torch, p32, x32, layer, hidden, apply)
                            agree(FIGURES, (name, layer, hidden, apply), name, got[j], ref[j], t32,
                                  where=(D, O, j, P, probes.ndim))


@pytest.mark.parametrize('name', DTYPES)
def test_units_and_instances_move_data_exactly(torch_cuda, name):
    torch = torch_cuda
    dt = _np(name)
    D, O, n = 7, 4, 5
    rng = np.random.default_rng(9)
    stack = mc.draw_networks(rng, n, D, O, dt)
    stack['b1'][:, 5] = -1e3                       # a unit that never fires: exact zeros after ReLU
    dP = _stack_dev(torch, stack)
    for P in (1, 33, 65):
        probes = rng.standard_normal((n, P, D)).astype(dt)
        d_probes = _dev(torch, probes)
        for layer, hidden, apply in ((0, 'relu', 'relu'), (1, 'tanh', 'tanh'), (2, 'relu', 'none')):
            full = _run(torch, name, dP, d_probes, n, P, D, O, layer, hidden, apply)
            U = full.shape[1]
            for units in ([0], [U - 1], [U - 1, 0, 2 % U, 0, 1 % U]):
                got = _run(torch, name, dP, d_probes, n, P, D, O, layer, hidden, apply, units)
                assert got.tobytes() == full[:, units].tobytes(), (P, layer, units)
            for j in range(n):
                alone = {k: v[j:j + 1].contiguous() for k, v in dP.items()}
                got = _run(torch, name, alone, d_probes[j:j + 1].contiguous(), 1, P, D, O, layer,
                           hidden, apply)
                assert got[0].tobytes() == full[j].tobytes(), (P, layer, j)
                shared = _run(torch, name, alone, d_probes[j].contiguous(), 1, P, D, O, layer,
                              hidden, apply)
                assert shared[0].tobytes() == full[j].tobytes(), (P, layer, j)
            if layer == 0:
                assert (full[:, 5, :] == 0).all() and not np.signbit(full[:, 5, :]).any()
                assert (full >= 0).all()


def test_refusals_that_need_a_device(torch_cuda):
    torch = torch_cuda
    from cobel_amd import _lib
    D, O, n, P = 7, 4, 2, 5
    stack = mc.draw_networks(np.random.default_rng(1), n, D, O, np.float64)
    dP = _stack_dev(torch, stack)
    probes = _dev(torch, np.zeros((P, D)))
    for layer, units, width in ((0, [0, 64], 64), (1, [-1], 64), (2, [3, 4], 4)):
        out = Framed(torch, (n, len(units), P), torch.float64)
        run = ac.fill_activity(_lib, dP, probes, out.view, n, P, D, O, layer, 'relu', 'relu',
                               units=_dev(torch, np.asarray(units, dtype=np.int32)))
        with pytest.raises(IndexError, match=r'layer %d has %d units' % (layer, width)):
            _lib.check(_lib.lib().cobel_mlp_activity(C.byref(run), None))
        torch.cuda.synchronize()
        assert out.intact() and all(out.untouched(j) for j in range(n))
