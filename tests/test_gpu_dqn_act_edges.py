"""cobel_dqn_act (csrc/dqn_act.hip: k_dqn_act in six instantiations, k_dqn_batch in three) against
the plain restatement of tests/dqn_act_common.py, which shares no code with the library and is
itself pinned by tests/test_host_dqn_act_reference.py.

Each case of dqn_act_common.CASES — one parameter away from a base case: launch shapes around one
wavefront and around 256 batch lanes, rings of 1 .. 40 rows that wrap, absent optional arrays,
both dtypes, monitor stripes and caps, 1 .. 8 actions, several worlds in one handle, instance
numbers and counters that wrap as uint32, and the world-model mode — runs 12 consecutive calls on
the state the library left in device memory.  The test writes a fresh Q table before every call
(ties of every size, -inf entries, NaN in the rows of frozen instances); no replay kernel runs.
After every call EVERY array is compared with np.array_equal: there are no tolerances in this
file, all quantities being integers, casts of table values, or float64 sums in a fixed order
(reward_sum, which atomics add in no fixed order, gets dyadic rewards, or one writer per cell).
Every array, inputs included, lies in a frame of sentinels that must stay intact; an instance that
is frozen keeps every byte of its rows and reports stepped = 0.

The refusals return their documented code before any launch and leave every buffer alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_act_common as dc  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_UNSUPPORTED = -1, -2, -4
PER_INSTANCE = [k for k in dc.ARRAYS if k not in ('obs_table', 'lat_sum', 'lat_cnt', 'reward_sum',
                                                  'stepped')]


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_every_array_after_every_call(torch_cuda, name):
    case = dc.make_case(name)
    dev = dc.DeviceCase(torch_cuda, case)
    try:
        before = dev.read()
        for k, (q, ref) in enumerate(case['steps']):
            dev.set_q(q)
            frozen = np.flatnonzero(before['active'] == 0)
            assert dev.launch(dev.fill()) == 0, (name, k)
            got = dev.read()
            assert dc.same(got, ref) == [], (name, k)
            assert dev.intact() == [], (name, k)
            assert not got['stepped'][frozen].any(), (name, k)
            for key in PER_INSTANCE:
                if key != 'q' and got[key] is not None:
                    assert got[key][frozen].tobytes() == before[key][frozen].tobytes(), (name, k, key)
            before = got
    finally:
        dev.close()


def _refused(dev, code, where, world=None, **changes):
    kept = dev.buffers()
    assert dev.launch(dev.fill(**changes), world) == code, where
    after = dev.buffers()
    for key, buf in kept.items():
        assert after[key].tobytes() == buf.tobytes(), (where, key)


def test_refusals_in_ring_mode(torch_cuda):
    from cobel_amd import _lib
    case = dc.make_case('base')
    dev = dc.DeviceCase(torch_cuda, case)
    worlds = []
    try:
        dev.set_q(np.zeros_like(case['qs'][0]))
        for key in ('state', 'env_ctr', 'obs_table', 'q', 'policy_ctr') + dc.RING + (
                'trial', 'step', 'trial_reward', 'active', 'stepped', 'memory_ctr'):
            # (memory_ctr: batch_slots is given, so the counter has to be)
            _refused(dev, E_ARG, key, **{key: None})
        for key, value, code in (('n_obs', 0, E_RANGE), ('slots', 0, E_RANGE), ('batch', -1, E_RANGE),
                                 ('steps_per_trial', 0, E_RANGE), ('epsilon', -0.1, E_ARG),
                                 ('epsilon', 1.5, E_ARG)):
            _refused(dev, code, (key, value), **{key: value})
        rng = np.random.default_rng(3)
        nine = dc.create_world(dc.draw_world(rng, 8, 9, 1, (2,)))
        worlds.append(nine)
        _refused(dev, E_UNSUPPORTED, 'nine actions', world=nine)
        for A in (4, 6):
            table = dc.draw_world(rng, 8, A, 1, (2,))
            drawn = dc.create_world(table)
            worlds.append(drawn)
            dc.set_one_hot_transitions(drawn, table)
            _refused(dev, E_UNSUPPORTED, ('distribution rows', A), world=drawn)
        # ... and the unchanged arguments are served
        assert dev.launch(dev.fill()) == 0
    finally:
        for handle in worlds:
            _lib.lib().cobel_world_destroy(handle)
        dev.close()


def test_refusals_in_world_model_mode(torch_cuda):
    from cobel_amd import _lib
    case = dc.make_case('model-lr0.9-batch1-f32')
    dev = dc.DeviceCase(torch_cuda, case)
    six = None
    try:
        dev.set_q(np.zeros_like(case['qs'][0]))
        for key in dc.MODEL[1:] + ('memory_ctr',):
            _refused(dev, E_ARG, key, **{key: None})
        _refused(dev, E_ARG, 'n_states', n_states=case['par']['n_states'] + 1)
        six = dc.create_world(dc.draw_world(np.random.default_rng(4), 6, 6, 1, (2,)))
        _refused(dev, E_UNSUPPORTED, 'six actions with a world model', world=six)
        assert dev.launch(dev.fill()) == 0
    finally:
        _lib.lib().cobel_world_destroy(six)
        dev.close()
