"""The NumPy restatement of PMAMemory and of the PMA trial loop (tests/pma_common.py, as it is: it
holds no 8-bit assumption) equals the fixture recorded from the reference on worlds of 132 and 272
states (tests/golden/gen_pma_wide.py) bit for bit.  The SR row of every replay and the need vector
of the ``current_state=None`` replay are LAPACK's: they are taken from the fixture."""
import os

import numpy as np
import pytest

import pma_common as pc
import pma_wide_common as pw
from oracle.ref_loop import RefEpsilonGreedy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pma_wide_traces.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def case_of(golden, name):
    return {k.split('/', 1)[1]: golden[k] for k in golden.files if k.startswith(name + '/')}


@pytest.mark.parametrize('name', sorted(pw.MEMORY_CASES))
def test_memory_restatement_equals_reference(golden, name):
    want = case_of(golden, name)
    tabs, sas = pc.tables_of(pw.WORLDS[pw.MEMORY_CASES[name][0]]())
    S = sas.shape[0]
    ops = pc.loads(want['ops'])
    states = pw.replay_states(ops)
    rm, rp = pc.memory_rngs(pw.SEED, int(want['cfg'][0]))
    mem = pc.RefPMAMemory(sas, RefEpsilonGreedy(0.1, rp), gamma_q=0.99, rng=rm)

    def give_sr(k):
        mem.SR = pw.sr_of_row(S, states[k], want['SR'][k])

    def give_need(k):
        mem.need_given = np.array(want['need'][k])

    got = pc.ScriptMemory(mem, pc.masked_actions(tabs), sr=give_sr, need=give_need,
                          index=lambda m: (m.rng.index, m.policy.rng.index)).run(ops)
    pc.assert_same_record(got, want, what=name)
    past = 255 if S > 256 else 127
    rep = want['replayed']
    assert (rep[:, 1] > past).any() and (rep[:, 4] > past).any() and len(rep) > 100
    assert len(want['need']) >= 1


def test_agent_restatement_equals_reference(golden):
    want = case_of(golden, 'agent_wide')
    tabs, sas = pc.tables_of(pw.WORLDS[pw.AGENT_WORLD]())
    S = sas.shape[0]
    env, agent, mem = pc.make_ref_agent(tabs, sas, pw.SEED, pw.AGENT_INSTANCE)
    agent.mask_actions = True
    k = [0]

    def give_sr():
        sr = np.zeros((S, S))
        sr[want['sr_states']] = want['sr_rows'][k[0]]
        mem.SR = sr
        k[0] += 1

    agent.update_sr = give_sr
    tr = pc.new_trace()
    agent.train(env, len(want['steps']), pw.AGENT_STEPS, pw.AGENT_BATCH, False, trace=tr)
    assert np.array_equal(np.array(tr['steps']), want['steps'])
    assert np.array_equal(np.array(tr['replay_start']), want['replay_start'])
    assert np.array_equal(np.array(tr['replay_end']), want['replay_end'])
    assert np.array_equal(np.array(tr['q_start']), want['q_replay'][0::2])
    assert np.array_equal(np.array(tr['q_end']), want['q_end'])
    assert np.array_equal(mem.T, want['T']) and np.array_equal(mem.rewards, want['rewards'])
    assert np.array_equal(mem.states, want['states']) and np.array_equal(mem.terminals, want['terminals'])
    assert [env.rng.index, agent.policy.rng.index, mem.rng.index,
            mem.policy.rng.index] == want['index'].tolist()
    assert (np.array(tr['last']) == want['sr_states'][1]).all()
