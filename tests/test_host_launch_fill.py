"""The host-side launch plumbing on CPU tensors: ``DeviceMonitors.fill`` for every launch struct,
the action-mask bits and the per-instance argument check of the device memories."""
import numpy as np
import pytest
import torch

from cobel_amd import _lib
from cobel_amd.agent.agent import DeviceMonitors
from cobel_amd.memory import _device

STRUCTS = ('TabRun', 'SRRun', 'SFMARun', 'PMARun', 'DQNAct')
PER_TRIAL = ('lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt')
CAP, N_ENVS = 7, 3


@pytest.mark.parametrize('present', [False, True], ids=['bare', 'resp+trace'])
@pytest.mark.parametrize('stripes', [1, 16])
@pytest.mark.parametrize('name', STRUCTS)
def test_monitors_fill_names_the_raw_tensors(name, stripes, present):
    mon = DeviceMonitors(torch.device('cpu'), 2, 25, occupancy=present, responses=present,
                         stripes=stripes)
    mon.reserve(CAP, N_ENVS, per_instance=present)
    assert mon.raw('lat_sum').shape == (stripes, CAP)
    assert (mon.raw('resp_cnt') is not None) == present and (mon.lat_trace is not None) == present
    want = {k: mon.raw(k) for k in PER_TRIAL}
    want.update(lat_trace=mon.lat_trace, occupancy=mon.occupancy, steps_done=mon.steps_done)
    want = {k: None if t is None else t.data_ptr() for k, t in want.items()}
    want.update(trial_cap=CAP, mon_stripes=stripes)

    cls = getattr(_lib, name)
    declared = {f[0] for f in cls._fields_}
    assert {'lat_sum', 'lat_cnt', 'reward_sum', 'trial_cap', 'mon_stripes'} <= declared
    if name == 'DQNAct':
        assert len(declared & set(want)) == 5
    else:
        assert set(want) <= declared
    struct = cls()
    mon.fill(struct)
    for field, value in want.items():
        if field in declared:
            assert getattr(struct, field) == value, field      # (a NULL pointer reads as None)
        else:
            assert not hasattr(struct, field), field           # nothing hung on the object either
    # every other field is as a fresh struct has it
    expect = cls()
    for field in declared & set(want):
        setattr(expect, field, want[field])
    assert bytes(struct) == bytes(expect)
    # a second call follows the monitors: grown arrays, a trace that has appeared
    mon.reserve(CAP + 5, N_ENVS, per_instance=True)
    mon.fill(struct)
    assert struct.lat_sum == mon.raw('lat_sum').data_ptr() and struct.trial_cap == CAP + 5
    if 'lat_trace' in declared:
        assert struct.lat_trace == mon.lat_trace.data_ptr()


def _bits_by_hand(mask):
    return [sum(1 << a for a, on in enumerate(row) if on) for row in mask]


@pytest.mark.parametrize('actions', [4, 8, 12])
def test_mask_bits(actions):
    rng = np.random.default_rng(actions)
    mask = rng.random((9, actions)) < 0.5
    mask[:, 0] |= ~mask.any(axis=1)
    mask[3] = True                       # every bit, the top one included
    mask[4] = False
    mask[4, actions - 1] = True          # the top bit alone
    bits = _device.mask_bits(mask, 9, actions)
    assert bits.shape == (9,)
    if actions <= 8:
        assert bits.dtype == np.uint8 and bits.itemsize == 1
        assert bits.tolist() == _bits_by_hand(mask)
    else:
        assert bits.dtype == np.int32
        assert bits.view(np.uint32).tolist() == _bits_by_hand(mask)
    assert int(bits.view(np.uint8 if actions <= 8 else np.uint32)[3]) == (1 << actions) - 1
    assert int(bits.view(np.uint8 if actions <= 8 else np.uint32)[4]) == 1 << (actions - 1)
    # the flat form the agents keep is taken as well
    assert np.array_equal(_device.mask_bits(mask.reshape(-1).tolist(), 9, actions), bits)


def test_mask_bits_at_four_actions_are_the_known_bytes():
    mask = [[1, 0, 0, 0], [0, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 1]]
    assert _device.mask_bits(mask, 4, 4).tolist() == [1, 10, 15, 8]


@pytest.mark.parametrize('actions', [4, 8, 12])
def test_mask_bits_refuse_a_row_without_actions(actions):
    mask = np.ones((5, actions), dtype=bool)
    mask[2] = False
    with pytest.raises(AssertionError, match='The action mask masks all actions!'):
        _device.mask_bits(mask, 5, actions)


def test_agents_take_their_bits_from_mask_bits():
    from cobel_amd.agent import QAgent
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    agent = QAgent(Discrete(6), Discrete(12), EpsilonGreedy(0.1))
    agent.action_mask[:, 1::2] = False
    got = agent._mask_bits()
    assert got.dtype == torch.int32
    assert got.tolist() == [0x555] * 6
    agent = QAgent(Discrete(6), Discrete(4), EpsilonGreedy(0.1))
    agent.action_mask[1, 2] = False
    got = agent._mask_bits()
    assert got.dtype == torch.uint8 and got.tolist() == [15, 11, 15, 15, 15, 15]


def test_per_instance_strict_mode():
    """SFMAMemory's: None stays None, a negative entry is out of range."""
    f = _device.per_instance
    assert f(None, 3, 'state', 25) is None
    a = f(7, 3, 'state', 25)
    assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.tolist() == [7, 7, 7]
    assert f(np.array([0, 24, 3]), 3, 'state', 25).tolist() == [0, 24, 3]
    assert f([1, 2, 3], 3, 'state', 25).tolist() == [1, 2, 3]
    for bad in (25, -1, [0, 25, 1], np.array([0, -1, 1])):
        with pytest.raises(IndexError, match=r'state outside \[0, 25\)'):
            f(bad, 3, 'state', 25)
    with pytest.raises(ValueError):
        f([1, 2], 3, 'state', 25)          # neither a scalar nor one entry per instance


def test_per_instance_none_as_minus_one():
    """PMAMemory's: None and negative entries mean "no state" and become -1."""
    f = _device.per_instance
    assert f(None, 3, 'current_state', 25, none_as=-1).tolist() == [-1, -1, -1]
    a = f(7, 3, 'current_state', 25, none_as=-1)
    assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.tolist() == [7, 7, 7]
    assert f([4, None, -3], 3, 'current_state', 25, none_as=-1).tolist() == [4, -1, -1]
    assert f(np.array([0, -7, 24]), 3, 'current_state', 25, none_as=-1).tolist() == [0, -1, 24]
    assert f(-2, 3, 'current_state', 25, none_as=-1).tolist() == [-1, -1, -1]
    for bad in (25, [0, 25, -1]):
        with pytest.raises(IndexError, match=r'current_state outside \[0, 25\)'):
            f(bad, 3, 'current_state', 25, none_as=-1)
    src = np.array([1, -5, 2])
    f(src, 3, 'current_state', 25, none_as=-1)
    assert src.tolist() == [1, -5, 2]      # the caller's array is left alone
