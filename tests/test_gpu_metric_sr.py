"""cobel_metric_sr on the device (csrc/metric.hip; ``SR(..., compute='device')``): bit for bit the
NumPy restatement of tests/metric_common.py on both sides of the 32-pivot panel and of the 64-wide
tile, stacks of worlds, repeatability, sentinel frames, and two worlds beyond anything the LDS forms
of SFMA know against the host path.

The two large worlds (33 x 33 and 25 x 51) are checked by bound (b) of tests/test_host_metric.py,
``e_dev <= F * max(e_host, 2^-53 max |D|)``, with the 80-bit solution by iterative refinement
(``metric_common.refined``: the 80-bit elimination of 1 089 states takes too long for a test; the
refinement is checked against it on the CPU) — so e_host is measured, not replaced by the floor."""
import numpy as np
import pytest

import metric_common as mc
from frames_common import Frames, same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 25, 31, 32, 33, 63, 64, 65, 96, 129, 272]
GAMMAS = (0.5, 0.9, 0.99)


@pytest.fixture(scope='module', autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'


@pytest.mark.parametrize('S', SIZES)
def test_bits_against_the_restatement(S):
    """Three worlds (open, walls, an isolated cell) in one call per gamma."""
    tabs = np.stack(mc.sr_worlds(S))
    for gamma in GAMMAS:
        D = mc.device_sr(tabs, gamma).cpu().numpy()
        for w in range(3):
            assert np.array_equal(D[w], mc.sr_ref(tabs[w], gamma)), (S, gamma, w)


@pytest.mark.parametrize('W', [1, 3, 5])
def test_a_world_of_a_stack_equals_the_world_alone(W):
    w, h = mc.SHAPES[65]
    tabs = np.stack([mc.maze(w, h, 0.05 * i, 300 + i)[0] for i in range(W)])
    D = mc.device_sr(tabs, 0.9)
    for i in range(W):
        assert same_bits(D[i], mc.device_sr(tabs[i:i + 1], 0.9)[0]), i
    assert np.array_equal(D[W - 1].cpu().numpy(), mc.sr_ref(tabs[W - 1], 0.9))


def test_two_runs_give_the_same_bits():
    tabs = np.stack(mc.sr_worlds(129))
    assert same_bits(mc.device_sr(tabs, 0.99), mc.device_sr(tabs, 0.99))


@pytest.mark.parametrize('S,shift', [(33, 0), (96, 16), (1, 0)])
def test_frames_stay_intact(S, shift):
    tabs = np.stack(mc.sr_worlds(S)[:2])
    frames = Frames(shift)
    D = mc.device_sr(tabs, 0.9, frames)
    frames.check()
    assert same_bits(D, mc.device_sr(tabs, 0.9))


def test_the_classes(golden):
    """One table gives [S, S], a stack [W, S, S]; a dense one-hot tensor is reduced; the golden
    worlds at the host test's tolerance; update_transitions() rewrites D where it lies."""
    import torch
    from cobel_amd.memory.utils import SR
    Z = golden('sfma_traces')
    for wname in ('sfma_5x5', 'sfma_6x7'):
        nxt = Z['world/%s/next' % wname].astype(np.int64)
        S = nxt.shape[0]
        sas = np.zeros((S, 4, S))
        sas[np.arange(S)[:, None], np.arange(4)[None, :], nxt] = 1.0
        for table in (nxt, sas):
            m = SR(table, 0.9, compute='device')
            assert m.D.is_cuda and m.D.dtype == torch.float64 and tuple(m.D.shape) == (S, S)
            assert np.array_equal(m.D.cpu().numpy(), mc.sr_ref(nxt, 0.9))
            np.testing.assert_allclose(m.D.cpu().numpy(), Z['metric/%s/SR' % wname], rtol=1e-12,
                                       atol=1e-14)
    a, b = mc.maze(6, 7, 0.1, 1)[0], mc.maze(6, 7, 0.2, 2)[0]
    tables = [a.copy(), b.copy()]
    m = SR(tables, 0.9, compute='device')
    assert tuple(m.D.shape) == (2, 42, 42)
    assert np.array_equal(m.D[1].cpu().numpy(), mc.sr_ref(b, 0.9))
    ptr = m.D.data_ptr()
    tables[0][:] = mc.open_table(6, 7)
    m.update_transitions()
    assert m.D.data_ptr() == ptr and m.version == 1
    assert np.array_equal(m.D[0].cpu().numpy(), mc.sr_ref(mc.open_table(6, 7), 0.9))
    assert np.array_equal(m.D[1].cpu().numpy(), mc.sr_ref(b, 0.9))


@pytest.mark.parametrize('w,h,walls', [(33, 33, [(34, 35), (100, 133)]),
                                       (25, 51, [(26, 27), (300, 325)])])
def test_large_worlds_against_the_host_path(w, h, walls):
    from cobel_amd.memory.utils import SR
    nxt, _ = mc.with_walls(w, h, walls)
    host = SR(nxt, 0.9).D
    dev = SR(nxt, 0.9, compute='device').D.cpu().numpy()
    e_host, e_dev, floor = mc.errors(dev, host, mc.refined(nxt, 0.9, host))
    print('%d x %d: e_host %.3g e_dev %.3g floor %.3g ratio %.2f'
          % (w, h, e_host, e_dev, floor, e_dev / max(e_host, floor)))
    assert e_dev <= mc.F * max(e_host, floor)
