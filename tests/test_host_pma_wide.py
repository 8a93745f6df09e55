"""Host logic of PMA's wide form: the wide plan and its limits, construction with ``wide=True``,
the agreement of header, ctypes and library on the additions.  (tests/test_host_pma.py pins the
default form, which does not change.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pma_common as pc
import pma_wide_common as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_wide(S, A, L):
    from cobel_amd import _lib
    out = (C.c_int32 * 4)()
    rc = _lib.lib().cobel_pma_plan_wide(S, A, L, C.byref(out))
    return rc, list(out), _lib.lib().cobel_last_error().decode()


def carve(S, A, L):
    """The wide form's LDS: three float64 tables of S x A, the need row, L + 1 step gains, L rewards,
    L 32-bit records (to 8 bytes), 16-bit successors, two byte tables of S x A, the action bits."""
    o = 24 * S * A + 8 * S + 8 * (L + 1) + 8 * max(L, 1) + 8 * ((L + 2) // 2)
    o += 2 * S * A + 2 * S * A + ((S + 7) & ~7)
    return (o + 15) & ~15


def test_exports_agree():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    assert re.search(r'COBEL_API\s+int\s+cobel_pma_plan_wide\s*\(', header)
    assert 'cobel_pma_plan_wide' in _lib.EXPORTS
    getattr(_lib.lib(), 'cobel_pma_plan_wide')
    assert _lib.PMA_MAX_STATES == 128 and _lib.PMA_WIDE_MAX_STATES == 1024
    assert re.search(r'#define COBEL_PMA_WIDE_MAX_STATES %d\b' % _lib.PMA_WIDE_MAX_STATES, header)
    assert re.search(r'#define COBEL_PMA_WIDE %du' % _lib.PMA_WIDE, header)


@pytest.mark.parametrize('S,A,L', [(132, 4, 32), (272, 4, 32), (1024, 4, 8)])
def test_wide_plan_accepts(S, A, L):
    from cobel_amd import _lib
    rc, out, _ = plan_wide(S, A, L)
    assert rc == _lib.OK
    assert out[0] == carve(S, A, L) <= 160 * 1024
    assert out[1] == 64 and out[3] == 256 and 0 < out[2] <= 160 * 1024


@pytest.mark.parametrize('S,A,L,words', [
    (1025, 4, 1, ('128 states', '8 actions', '1024 states')),
    (25, 9, 1, ('128 states', '8 actions', '1024 states')),
    (1024, 8, 8, ('B of LDS', str(160 * 1024), str(64 * 1024)))])
def test_wide_plan_refuses(S, A, L, words):
    from cobel_amd import _lib
    rc, out, msg = plan_wide(S, A, L)
    assert rc == _lib.E_UNSUPPORTED and out == [0, 0, 0, 0]
    for w in words:
        assert w in msg, (w, msg)
    if S == 1024:        # the byte count asked for is in the message
        assert str(carve(S, A, L)) in msg, msg


def test_wide_memory_constructs_at_272_states():
    from cobel_amd import _lib
    from cobel_amd.agent import PMA
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    world = pw.world_272()
    tabs, sas = pc.tables_of(world)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=True)
    ref = pc.RefPMAMemory(sas, None, gamma_q=0.99)
    assert mem.wide and (mem.nb_states, mem.nb_actions) == (272, 4)
    assert np.array_equal(mem.T, ref.T) and np.array_equal(mem.SR, ref.SR)
    assert np.array_equal(mem.update_mask, ref.update_mask)
    assert mem.flags() == 4 | 16 | _lib.PMA_WIDE
    assert mem.launch_plan(32)[0] == plan_wide(272, 4, 32)[1][0]
    agent = PMA(Discrete(272), Discrete(4), EpsilonGreedy(0.1), mem)
    assert agent.Q.shape == (272, 4) and agent.M is mem
    # the default form refuses the same world as before, and the agent follows its memory
    with pytest.raises(NotImplementedError, match='128 states and 8 actions'):
        PMAMemory(world['sas'], EpsilonGreedy(0.1))
    small = PMAMemory(pc.demo_world()['sas'], EpsilonGreedy(0.1))
    assert not small.wide and small.flags() == 4 | 16
    with pytest.raises(NotImplementedError, match='128 states and 8 actions'):
        PMA(Discrete(272), Discrete(4), EpsilonGreedy(0.1), small)


def test_wide_refusal_quotes_both_limits_and_the_bytes():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    with pytest.raises(NotImplementedError) as e:
        PMAMemory(np.zeros((1025, 4, 1025)), EpsilonGreedy(0.1), wide=True)
    assert '128 states' in str(e.value) and '1024 states' in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        PMAMemory(np.zeros((1024, 8, 1024)), EpsilonGreedy(0.1), wide=True)
    msg = str(e.value)
    assert '128 states' in msg and '1024 states' in msg and 'B of LDS' in msg
    assert str(160 * 1024) in msg and str(carve(1024, 8, 0)) in msg


def test_wide_bind_refuses_before_allocating(monkeypatch):
    """N * S^2 * 16 bytes of T and SR against the free device memory: MemoryError naming the size,
    raised before any table is made."""
    import torch
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(pw.world_272()['sas'], EpsilonGreedy(0.1), wide=True)
    need = 1000 * 272 * 272 * 16
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (need - 1, 2 * need))

    def no_allocation(*args, **kwargs):
        raise AssertionError('a table was allocated before the check')

    monkeypatch.setattr(torch, 'as_tensor', no_allocation)
    with pytest.raises(MemoryError) as e:
        mem._bind(1000, torch.device('cuda', 0))
    msg = str(e.value)
    assert str(need) in msg and '1000 instances' in msg and '272 states' in msg
    assert str(need - 1) in msg and mem._dev is None
