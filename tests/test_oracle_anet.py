"""The restatement of tests/anet_common.py (AssociativeNetwork and EpsilonGreedy in plain floats,
with the device's summation order) against the traces recorded from the real reference
(tests/golden/anet_traces.npz)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anet_common as ac  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'anet_traces.npz')
SPARSE = [n for n, c in ac.CASES.items() if not c['dense']]


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def test_the_fixture_holds_every_case(Z):
    assert sorted({k.split('/')[0] for k in Z.files}) == sorted(ac.CASES)
    for name, c in ac.CASES.items():
        assert float(Z[name + '/margin']) > 1e-12, name
        assert not c['dense'] or float(Z[name + '/gap']) > 1e-9, name
        assert Z[name + '/index'][2] == 0, 'policy_test must never be drawn from'


@pytest.mark.parametrize('name', SPARSE)
def test_sparse_cases_equal_the_reference_exactly(Z, name):
    """Observations of at most two non-zero components, each a power of two: every product is exact
    and any summation order, fused or not, gives BLAS's sum."""
    for o in ac.CASES[name]['design']()[1].values():
        nz = np.asarray(o)[np.asarray(o) != 0]
        assert len(nz) <= 2 and all(np.frexp(v)[0] == 0.5 for v in nz)
    ac.assert_same_record(ac.restated(name), Z, name + '/', what=name)


def test_dense_case_within_the_measured_bound(Z):
    """D = 6, dense observations: the tree sum differs from BLAS's in the last bits of the outputs.
    Measured by tests/golden/gen_anet.py: the largest |q difference| is 1.07e-14, the bound the next
    power of two above it, 2^-46; weights and final predictions do not see the sums and are equal.
    Both sides are deterministic."""
    out = ac.restated('dense6')
    ac.assert_same_record(out, Z, 'dense6/', what='dense6', keys=ac.DISCRETE)
    for key, names in (('W', ('We', 'Wi')), ('q', ('q',)), ('predict', ('predict',))):
        measured, bound = ac.DENSE_MEASURED[key], ac.DENSE_BOUND[key]
        assert measured == bound == 0.0 or measured < bound <= 2 * measured, key
        diff = max(float(np.abs(out[k] - Z['dense6/' + k]).max()) for k in names)
        print('dense6: largest |%s difference| %.17g' % (key, diff))
        assert diff <= bound, key
    active = [int(((o != 0) & (np.frexp(o)[0] != 0.5)).sum())
              for o in ac.CASES['dense6']['design']()[1].values()]
    assert min(active) >= 3


def test_cases_cover_what_they_are_meant_to(Z):
    # A - 1 outputs, and one policy draw per step also where there is one output only
    assert Z['single_output/q'].shape[1] == 1 and Z['eight_outputs/q'].shape[1] == 8
    assert Z['single_output/index'].tolist() == [24, 24, 0]
    assert not Z['single_output/action'].any()
    assert Z['eight_outputs/index'][0] == 8 * len(Z['eight_outputs/action'])
    assert len(set(Z['eight_outputs/action'].tolist())) >= 5
    # the four unit variants differ, and the dict entries are all distinct
    finals = [Z[n + '/We'][-1].tobytes() + Z[n + '/Wi'][-1].tobytes()
              for n in ('unit', 'unit_linear', 'unit_saturation', 'unit_rates')]
    assert len(set(finals)) == 4
    for n, key in (('unit_saturation', 'saturation'), ('unit_rates', 'learning_rate')):
        d = ac.CASES[n]['agent_kw'][key]
        assert len({float(v) for k in ac.KEYS for v in d[k].reshape(-1)}) == 8
    # test sessions leave the weights alone
    assert np.array_equal(Z['unit/We'][9], Z['unit/We'][-1])
    # multi-step trials: some cut by the cap, some ended; rewards of every sign; both matrices move
    cut = Z['multistep_cut/end']
    assert cut.any() and not cut.all()
    steps = Z['multistep_cut/steps']
    assert steps.max() == 2 and (steps[:6] <= 1).all()
    r = Z['multistep_cut/reward']
    assert (r > 0).any() and (r == 0).any() and (r < 0).any()
    assert Z['multistep_cut/We'][-1].any() and Z['multistep_cut/Wi'][-1].any()
    # ties: all three outputs tie on the first step, two tie exactly on a later one
    q = np.sort(Z['ties/q'], axis=1)
    assert q[0, 0] == q[0, 2] == 0.0
    assert ((q[1:, 2] == q[1:, 1]) & (q[1:, 1] != q[1:, 0])).any()
    # the mask tests for non-zero: a component of 0.5 or 2.0 takes the same increment as one of 1.0
    c = ac.CASES['mask_nonzero']
    first = Z['mask_nonzero/We'][0] + Z['mask_nonzero/Wi'][0]
    inc = c['agent_kw']['learning_rate'] * c['agent_kw']['saturation']
    assert sorted(first[first != 0].tolist()) == [inc, inc]
    # between sessions: the prediction drew from the agent's stream
    assert Z['between_sessions/mid_predict'].shape == (1, 2, 2)
    assert Z['between_sessions/index'][0] == 2 * 20 + 4


def test_noise_tape_draws_consecutive_indices(Z):
    """``random(k)`` takes k consecutive indices — and that is how the fixture was recorded: with
    zero weights the first outputs of the reference are ``noise_amplitude`` times the first draws."""
    a = ac.NoiseTape(ac.SEED, 3, ac.STREAM_AGENT)
    b = ac.NoiseTape(ac.SEED, 3, ac.STREAM_AGENT)
    u = a.random(5)
    assert u.tolist() == [b.random() for _ in range(5)] and a.index == b.index == 5
    for name in ('unit', 'eight_outputs'):
        c = ac.CASES[name]
        tape = ac.NoiseTape(ac.SEED, c['inst'], ac.STREAM_AGENT)
        noise = c['agent_kw'].get('noise', 1.0)
        want = [noise * tape.random() for _ in range(c['n_actions'] - 1)]
        assert Z[name + '/q'][0].tolist() == want, name
