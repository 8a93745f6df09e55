"""cobel_metric_dr on the device (csrc/metric.hip; ``DR(..., compute='device')``): bit for bit the
NumPy restatement of tests/metric_common.py at ranks around the 32-term staging of the update and
at the limit, worlds whose Woodbury block swaps rows, stacks of mixed ranks, the reference's golden
matrices, ``update_transitions()`` in place, and the refusal beyond the rank limit."""
import numpy as np
import pytest

import metric_common as mc
from frames_common import BIG, Frames, same_bits

pytestmark = pytest.mark.gpu

W20 = H20 = 20
RANKS = [0, 1, 2, 6, 8, 31, 32, 33, mc.MAX_RANK]


@pytest.fixture(scope='module', autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'


@pytest.fixture(scope='module')
def open20():
    """(default table, the restatement's D0, the device's D0) of the 20 x 20 field at gamma 0.9."""
    default = mc.open_table(W20, H20)
    D0 = mc.sr_ref(default, 0.9)
    dev = mc.device_sr(default[None], 0.9)[0]
    assert np.array_equal(dev.cpu().numpy(), D0)
    return default, D0, dev


@pytest.mark.parametrize('k', RANKS)
def test_bits_against_the_restatement(open20, k):
    default, D0, D0_dev = open20
    nxt, inv = mc.world_of_rank(W20, H20, k, seed=k)
    J = mc.affected(inv)
    assert len(J) == k
    frames = Frames()
    _, D, _ = mc.device_dr(D0_dev, nxt[None], default, [J], 0.9, frames)
    frames.check()
    assert np.array_equal(D[0].cpu().numpy(), mc.woodbury(D0, nxt, default, J, 0.9))


@pytest.mark.parametrize('args,gamma,swaps', [((12, 12, 0.05, 6, (0, 77)), 0.9, 3),
                                              ((12, 12, 0.2, 3, (30,)), 0.99, 2),
                                              ((11, 3, 0.3, 8, ()), 0.5, None)])
def test_worlds_whose_block_swaps_rows(args, gamma, swaps):
    """Isolated cells make the elimination of A = I + delta D0[:, J] pivot; 11 x 3 is a world whose
    edge tiles are ragged."""
    from cobel_amd.memory.utils import DR
    w, h = args[0], args[1]
    nxt, inv = mc.maze(*args)
    if swaps is not None:
        assert mc.pivot_swaps(mc.woodbury_block(w, h, nxt, inv, gamma)) == swaps
    m = DR(w, h, nxt, gamma, inv, compute='device')
    assert np.array_equal(m.D0.cpu().numpy(), mc.sr_ref(mc.open_table(w, h), gamma))
    assert np.array_equal(m.D.cpu().numpy(), mc.dr_ref(w, h, nxt, inv, gamma))


def test_a_stack_of_mixed_ranks(open20):
    default, D0, D0_dev = open20
    worlds = [mc.world_of_rank(W20, H20, k, seed=40 + k) for k in (6, 0, 33, 1, 32)]
    tabs = np.stack([w[0] for w in worlds])
    Js = [mc.affected(w[1]) for w in worlds]
    _, D, _ = mc.device_dr(D0_dev, tabs, default, Js, 0.9)
    for i, (nxt, inv) in enumerate(worlds):
        assert np.array_equal(D[i].cpu().numpy(), mc.woodbury(D0, nxt, default, Js[i], 0.9)), i
        alone = mc.device_dr(D0_dev, nxt[None], default, [Js[i]], 0.9)[1]
        assert same_bits(D[i], alone[0]), i
    assert same_bits(D[1], D0_dev)
    again = mc.device_dr(D0_dev, tabs, default, Js, 0.9)[1]
    assert same_bits(D, again)
    # the classes: one list of invalid transitions per world
    from cobel_amd.memory.utils import DR
    m = DR(W20, H20, [w[0] for w in worlds], 0.9, [w[1] for w in worlds], compute='device')
    assert tuple(m.D.shape) == (5, 400, 400) and same_bits(m.D, D)


@pytest.mark.parametrize('wname', ['sfma_5x5', 'sfma_6x7'])
def test_golden_worlds(golden, wname):
    from cobel_amd.memory.utils import DR
    Z = golden('sfma_traces')
    nxt = Z['world/%s/next' % wname].astype(np.int64)
    W, H = int(Z['world/%s/width' % wname]), int(Z['world/%s/height' % wname])
    inv = [tuple(int(x) for x in t) for t in Z['world/%s/invalid_transitions' % wname]]
    m = DR(W, H, nxt, 0.9, inv, compute='device')
    D = m.D.cpu().numpy()
    assert np.array_equal(D, mc.dr_ref(W, H, nxt, inv, 0.9))
    np.testing.assert_allclose(D, Z['metric/%s/DR' % wname], rtol=1e-12, atol=1e-14)
    assert not hasattr(m, 'T_new') and not hasattr(m, 'B')


def test_update_transitions_in_place():
    """A wall added, a wall removed, the last wall removed (rank back to 0): the same address, the
    bits of a fresh metric on the edited world."""
    from cobel_amd.memory.utils import DR
    w, h, gamma = 9, 7, 0.9
    nxt, inv = mc.with_walls(w, h, [(10, 11)])
    table, invalid = nxt.copy(), list(inv)
    m = DR(w, h, table, gamma, invalid, compute='device')
    ptr, ptr0 = m.D.data_ptr(), m.D0.data_ptr()
    d0 = m.D0.clone()
    for step, walls in enumerate(([(10, 11), (30, 39)], [(30, 39)], [])):
        nxt, inv = mc.with_walls(w, h, walls)
        table[:] = nxt
        invalid[:] = inv
        m.update_transitions()
        assert m.D.data_ptr() == ptr and m.D0.data_ptr() == ptr0 and m.version == step + 1
        fresh = DR(w, h, nxt, gamma, inv, compute='device')
        assert same_bits(m.D, fresh.D), walls
        assert np.array_equal(m.D.cpu().numpy(), mc.dr_ref(w, h, nxt, inv, gamma)), walls
        assert same_bits(m.D0, d0)
    assert same_bits(m.D, m.D0)


def test_rank_above_the_limit_is_refused_with_nothing_written(open20):
    from cobel_amd import _lib
    default, D0, D0_dev = open20
    nxt, inv = mc.world_of_rank(W20, H20, mc.MAX_RANK + 1, seed=3)
    J = mc.affected(inv)
    assert len(J) == mc.MAX_RANK + 1
    frames = Frames()
    rc, D, work = mc.device_dr(D0_dev, nxt[None], default, [J], 0.9, frames, check=False)
    assert rc == _lib.E_UNSUPPORTED
    assert 'up to %d' % mc.MAX_RANK in _lib.lib().cobel_last_error().decode()
    frames.check()
    assert bool((D == BIG).all()) and bool((work == 0x5A).all())
