"""CPU: the restatement behind the policy-kernel sweep (scripts/fuzz_tabpol.py ``run_reference``)
against the records taken from the real reference (tests/golden/tabpol_sweep_traces.npz, written by
tests/golden/gen_tabpol_sweep.py), and what the slices that tests/test_gpu_fuzz_tabpol.py runs
contain — on the restatement alone, for exactly their seeds."""
import os

import numpy as np
import pytest

import fuzz_tabpol_common as fa
import tabpol_common as tc
from conftest import GOLDEN


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'tabpol_sweep_traces.npz'))


@pytest.fixture(scope='module')
def slices():
    """{seed: (case, restatement)} of the slices, computed once and left unchanged."""
    import fuzz_tabpol as fz
    out = {}
    for seed in fa.seeds():
        case = fz.draw_case(seed)
        out[seed] = (case, fz.run_reference(case))
    return out


def compare(Z, name, got, keys):
    """(``td`` of a QAgent is left out, as in tests/test_host_tabpol.py: the reference's step callback
    sees the experience after the replay, which rewrites the ``td`` of an entry it draws again)"""
    seen = 0
    for k in keys:
        key = '%s/%s' % (name, k)
        if key in Z.files and not (k == 'td' and 'log' in got):
            assert k in got, (name, k)
            assert np.array_equal(np.asarray(got[k]), Z[key]), (name, k)
            seen += 1
    return seen


@pytest.mark.parametrize('seed', fa.TABPOL_RECORDED)
def test_restatement_equals_the_recorded_reference(Z, seed):
    """Instance 0 after the whole script: every step of every session, per trial latencies, rewards
    and Q, the tables, the carried state and the counter of every policy object."""
    import fuzz_tabpol as fz
    case = fz.draw_case(seed)
    out = fz.run_reference(case, instances=[0])
    assert compare(Z, 'seed%d' % seed, out[0][-1], tc.SWEEP_EXACT) >= 18
    assert out['margin'] > tc.MARGIN


def test_recorded_seeds_cover_the_extensions():
    """A QAgent test session under a Softmax, Dyna-Q test sessions under Exclusive and Random, an
    edit between two sessions, a mask under a policy that reads it, graphs of three and of eight
    actions, training under an EpsilonGreedy."""
    import fuzz_tabpol as fz
    seen = set()
    for seed in fa.TABPOL_RECORDED:
        c = fz.draw_case(seed)
        ops = [o['op'] for o in c['ops']]
        kinds = ({c['policy'][0]} if 'test_default' in ops else set()) | \
            ({c['second'][0]} if 'test_second' in ops else set())
        seen |= {(c['agent'], 'test', k) for k in kinds}
        sessions = [k for k, o in enumerate(ops) if o != 'edit']
        if any(sessions[0] < k < sessions[-1] for k, o in enumerate(ops) if o == 'edit'):
            seen.add('edit')
        if c['mask_seed'] is not None and c['policy'][0] != tc.RANDOM:
            seen.add('mask')
        if c['world'] == 'graph':
            seen.add('A%d' % c['A'])
        seen |= set(ops)
    assert {('q', 'test', tc.SOFTMAX), ('dynaq', 'test', tc.EXCLUSIVE), ('dynaq', 'test', tc.RANDOM),
            'edit', 'mask', 'A3', 'A8', 'train_eps', 'test_eps', 'train_budget'} <= seen


@pytest.mark.parametrize('name', sorted(tc.TEST_CASES))
def test_test_session_cases_equal_the_recorded_reference(Z, name):
    from cobel_amd.misc import gridworld_tools
    got = tc.restate_test_case(name, tc.world_tables(tc.grid4(gridworld_tools)))
    assert compare(Z, name, got, tc.EXACT + ('env_state',)) >= 16
    assert np.any(got['Q'] != 0), 'the training session learnt something'
    c = tc.session_case(name)
    n = int(got['n_train_steps'])
    assert 0 < n < len(got['state']), 'both sessions moved'
    if c['test'] is None:      # the shared object: one stream, one counter
        assert got['ctr_policy_test'] == 0 and got['ctr_policy'] == len(got['state'])
    else:
        assert got['ctr_policy'] == n and got['ctr_policy_test'] == len(got['state']) - n


def test_what_the_slices_contain(slices):
    cases = [c for c, _ in slices.values()]
    assert len(cases) == len(fa.TABPOL_FIRSTS) * fa.TABPOL_CHUNK == 200
    kinds = (tc.SOFTMAX, tc.EXCLUSIVE, tc.RANDOM)
    assert {(c['agent'], c['policy'][0]) for c in cases} == {(a, k) for a in ('dynaq', 'q') for k in kinds}
    assert {c['A'] for c in cases} == set(range(1, 9))
    sizes = [c['S'] for c in cases]
    assert 1 in sizes and 1023 in sizes and 1024 in sizes and max(sizes) == 1024
    off = [c for c in cases if c['extra_worlds'] and c['base'] % (1 + c['extra_worlds']) != 0]
    assert len(off) >= 2
    assert any(c['psets'] and c['psets']['shared'] for c in cases), 'shared parameter sets'
    assert any(c['psets'] and not c['psets']['shared'] for c in cases), 'all-distinct parameter sets'
    shared = [c for c in cases if c['psets'] and c['psets']['shared']]
    assert any(len(set(zip(c['psets']['par'], c['psets']['alpha'], c['psets']['gamma']))) < c['n']
               for c in shared), 'several instances on one set'
    ops = set(o['op'] for c in cases for o in c['ops'])
    assert ops == {'train', 'train_budget', 'test_default', 'test_second', 'test_eps', 'edit', 'train_eps'}
    as_test = set()
    for c in cases:
        for o in c['ops']:
            if o['op'] == 'test_default':
                as_test.add(c['policy'][0])
            elif o['op'] == 'test_second':
                as_test.add(c['second'][0])
    assert as_test == set(kinds)
    assert {0, 1, 62} <= {c['batch'] for c in cases}
    assert sum(c['mask_seed'] is not None and c['policy'][0] != tc.RANDOM for c in cases) >= 5
    assert {o['budget'] for c in cases for o in c['ops'] if o['op'] == 'train_budget'} == {1, 7}
    assert any(c['no_replay'] for c in cases)
    assert {c['n'] for c in cases} == {1, 2, 3, 7, 8, 9, 63, 64, 65, 130, 257}
    assert {c['base'] for c in cases} == {0, 5, 1 << 20}


def test_what_the_slices_exercise(slices):
    """On the restated instances: budgeted launches that end inside a trial, tables that learnt
    something (some of it negative), Softmax probabilities that underflowed to exact zeros."""
    mid = sum(fa.ends_mid_trial(c, out[0]) for c, out in slices.values())
    assert mid >= 10
    final = [out[0][-1]['Q'] for _, out in slices.values()]
    assert sum(bool(np.any(q != 0)) for q in final) >= 10
    assert sum(bool(np.any(q < 0)) for q in final) >= 3
    under = [c['seed'] for c, out in slices.values() if out['underflow']]
    assert len(under) >= 3 and all(
        tc.SOFTMAX in (slices[s][0]['policy'][0], slices[s][0]['second'][0]) for s in under)
    # (the restated instances: never more than ten, always 0, 1 and n - 1 and each world's first)
    import fuzz_tabpol as fz
    for c, out in slices.values():
        inst = fz.restated_instances(c)
        assert len(inst) <= fz.MAX_RESTATED and {0, min(1, c['n'] - 1), c['n'] - 1} <= set(inst)
        worlds = 1 + c['extra_worlds']
        assert {(c['base'] + i) % worlds for i in inst} == {(c['base'] + i) % worlds for i in range(c['n'])}


def test_no_slice_seed_is_left_out(slices):
    """Every draw of every slice seed lies at least SWEEP_MARGIN from every edge of its CDF."""
    worst = min(out['margin'] for _, out in slices.values())
    assert worst >= tc.SWEEP_MARGIN, worst
    for ipw in (1, 2, 4):      # (whatever the planner hands out, the other restated instances too)
        import fuzz_tabpol as fz
        for seed in (3, 4, 9, 23):
            c = slices[seed][0]
            assert fz.run_reference(c, ipw)['margin'] >= tc.SWEEP_MARGIN


def test_the_generator_is_pinned():
    import fuzz_tabpol as fz
    assert fz.draw_case(5) == {
        'seed': 5, 'world': 'graph', 'A': 2,
        'graph': {'S': 9, 'nbr': [[0, 0], [3, 2], [4, 7], [8, 6], [7, 6], [2, 0], [6, 0], [7, 8], [3, 8]],
                  'terminal': [True, False, False, False, False, False, False, False, False],
                  'reward': [-0.5, 0.001, 0.0, 0.5, 0.0, 0.0, 0.0, 0.5, 0.0], 'starts': [2]},
        'S': 9, 'extra_worlds': 0, 'world_seed': 138414407, 'base': 5, 'agent': 'q',
        'policy': ('exclusive', 0.3), 'alpha': 1.0, 'gamma': 0.9, 'n': 2, 'batch': 32, 'no_replay': False,
        'mask_seed': None, 'psets': None, 'second': ('exclusive', 0.3), 'eps_test': 0.0, 'eps_train': 0.0,
        'ops': [{'op': 'edit', 'edit_seed': 1148342785}, {'op': 'edit', 'edit_seed': 1977433572},
                {'op': 'train_budget', 'trials': 1, 'steps': 2, 'budget': 1},
                {'op': 'edit', 'edit_seed': 57622175}, {'op': 'train', 'trials': 1, 'steps': 24}]}
    # the graphs come from the generator of scripts/fuzz_topology.py, which still draws what it drew
    import fuzz_topology as ft
    t = ft.draw_case(7)
    assert (t['S'], t['A'], t['n'], t['batch'], t['starts']) == (56, 1, 1, 0, [0])
    assert int(t['nbr'].sum()) == 1324 and float(t['reward'].sum()) == 13.0
