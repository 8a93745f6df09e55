"""CPU tests of tests/dqn_act_common.py, the restatement tests/test_gpu_dqn_act_edges.py holds
cobel_dqn_act against: its selection against the reference's golden rows, its ring against a
deque, its draws against a TapeRNG consumed in the same order, and every case the GPU tests draw
against the conditions that make the strict comparison mean something."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_act_common as dc  # noqa: E402
from oracle.philox import TapeRNG  # noqa: E402


def _bits(bits, A):
    return np.array([(bits >> i) & 1 for i in range(A)], dtype=bool)


def test_selection_reproduces_the_golden_rows(golden):
    """Every row of eps_greedy_kat: 'rows' (four actions, float32 and float64 values, masks, draws
    at the CDF edges) and 'rows6' (six float32 values) in action and probabilities."""
    data = golden('eps_greedy_kat')
    assert len(data['rows']) > 1000 and len(data['rows6']) > 2000
    for r in data['rows']:
        v = r[2:6].astype(np.float32 if r[0] else np.float64)
        a, p = dc.select(v, r[1], r[7], _bits(int(r[6]), 4))
        assert a == int(r[8]) and np.array_equal(p, r[9:13]), r
    for r in data['rows6']:
        a, p = dc.select(r[1:7].astype(np.float32), r[0], r[8], _bits(int(r[7]), 6))
        assert a == int(r[9]) and np.array_equal(p, r[10:16]), r


def _tiny(slots, K, n=2):
    """One world in which nothing ends a trial: every call stores."""
    spec = dict(dc.BASE, n=n, slots=slots, steps_per_trial=10 ** 6, trials_target=10 ** 6, K=K,
                batch=4, name='tiny')
    return dc._draw_case(spec, 77 + slots)


@pytest.mark.parametrize('slots', [1, 2, 5])
def test_ring_is_a_deque(slots):
    """3 slots + 1 stores: the entries in FIFO order from the head are deque(maxlen=slots) of the
    experiences, and the slots drawn for the batch name entries the deque holds."""
    case = _tiny(slots, 3 * slots + 1)
    case['world']['terminal'][:] = 0
    steps, logs = dc.simulate(case)
    n = case['par']['n']
    model = [collections.deque(maxlen=slots) for _ in range(n)]
    before = case['state']
    table = before['obs_table'].astype(np.float32)
    for (q, st), log in zip(steps, logs):
        assert len(log) == n
        for i, a, *_ in log:
            s, ns = int(before['state'][i]), int(st['state'][i])
            model[i].append((table[s].tobytes(), table[ns].tobytes(), a,
                             float(case['world']['reward'][0, ns]), 1.0))
            size, head = int(st['ring_size'][i]), int(st['ring_head'][i])
            assert size == len(model[i])
            held = [(st['ring_states'][i, r].tobytes(), st['ring_next_states'][i, r].tobytes(),
                     int(st['ring_actions'][i, r]), float(st['ring_rewards'][i, r]),
                     float(st['ring_nonterminal'][i, r]))
                    for r in ((head + k) % slots for k in range(size))]
            assert held == list(model[i])
            assert all(0 <= (r - head) % slots < size for r in st['batch_slots'][i])
        before = st
    assert all(len(m) == slots for m in model)


def test_draws_are_a_tape_consumed_in_order():
    """Policy doubles, start draws and batches of every instance equal TapeRNGs of its streams
    consumed in the order of the reference's loop, counters that wrap included."""
    spec = dict(dc.spec_of('worlds3'), ctr0=0xFFFFFFFE, n=7, K=10, name='tape')
    case = dc._draw_case(spec, 5)
    par, world, before = case['par'], case['world'], case['state']
    n, seed = par['n'], par['seed']
    g = [(par['instance_base'] + i) & dc.M32 for i in range(n)]
    tape = {(i, name): TapeRNG(seed, g[i], stream, start=int(before[ctr][i]))
            for i in range(n)
            for name, stream, ctr in (('policy', par['policy_stream'], 'policy_ctr'),
                                      ('env', dc.STREAM_ENV, 'env_ctr'),
                                      ('memory', dc.STREAM_MEMORY, 'memory_ctr'))}
    steps, logs = dc.simulate(case)
    restarts = 0
    for (q, st), log in zip(steps, logs):
        for i, a, _ties, _done, _limit, restarted, _full in log:
            # (a TapeRNG counts without end; the restatement's counters wrap as uint32)
            for name in ('policy', 'env', 'memory'):
                tape[i, name].index &= dc.M32
            assert a == dc.select(q[i], par['epsilon'], tape[i, 'policy'].random())[0]
            if restarted:
                starts = world['starts'][g[i] % 3]
                assert st['state'][i] == starts[int(tape[i, 'env'].integers(0, len(starts)))]
                restarts += 1
            pick = tape[i, 'memory'].integers(0, int(st['ring_size'][i]), par['batch'])
            assert np.array_equal(st['batch_slots'][i],
                                  (int(st['ring_head'][i]) + pick) % par['slots'])
            for name, ctr in (('policy', 'policy_ctr'), ('env', 'env_ctr'), ('memory', 'memory_ctr')):
                assert int(st[ctr][i]) == tape[i, name].index & dc.M32
    assert restarts > 5


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_cases_meet_the_input_conditions(name):
    """Every case of the GPU tests: over its K calls the selections include every action of the
    world, every tie count from 1 to A occurs, a trial ends by `done` and one by the step limit,
    an instance is frozen before call K and one still steps at call K, a ring of at most 5 rows
    has been full for 5 steps — except what the case's own parameters rule out ('waive', each with
    its reason in dqn_act_common.CASES) — and Q rows of frozen instances hold NaN."""
    case = dc.make_case(name)
    spec = case['spec']
    assert set(spec['waive']) <= {'some_active', 'some_frozen', 'ring_full5'}
    met = dc.conditions(case, case['steps'], case['logs'])
    assert set(dc.CONDITIONS) - set(spec['waive']) <= met
    state = case['state']
    for q, after in case['steps']:
        frozen = state['active'] == 0
        assert np.isnan(q[frozen]).all() and not np.isnan(q[~frozen]).any()
        assert np.array_equal(after['stepped'], (~frozen).astype(np.uint8))
        state = after
    values = np.concatenate([q[~np.isnan(q)] for q, _ in case['steps']])
    assert np.isneginf(values).any() and set(values[np.isfinite(values)]) <= {-1.0, 0.0, 0.5, 1.0}
    if spec['rewards'] == 'non-dyadic':       # reward_sum: one writer per cell
        assert spec['mon_stripes'] == spec['n'] or 'reward_sum' in spec['absent']


def test_waived_conditions_are_met_between_the_cases():
    """n = 1 cannot be frozen and active at once: the two cases of it cover both."""
    met = [dc.conditions(c, c['steps'], c['logs'])
           for c in (dc.make_case('n1-freezes'), dc.make_case('n1-active'))]
    assert 'some_frozen' in met[0] and 'some_active' in met[1]
