"""The NumPy restatement of PMAMemory and of the PMA trial loop (tests/pma_common.py) equals the
fixture recorded from the reference (tests/golden/gen_pma.py) bit for bit.  The SR of every replay
and the need vector of the ``current_state=None`` replays are LAPACK's: they are taken from the
fixture, not recomputed."""
import os

import numpy as np
import pytest

import pma_common as pc
from oracle.philox import TapeRNG  # noqa: F401
from oracle.ref_loop import RefEpsilonGreedy

SEED = 0xC0BE1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pma_traces.npz')
MEMORY_CASES = {'mem_demo_5x5': 'demo_5x5', 'mem_small_3x4': 'small_3x4'}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def case_of(golden, name):
    return {k.split('/', 1)[1]: golden[k] for k in golden.files if k.startswith(name + '/')}


@pytest.mark.parametrize('name', sorted(MEMORY_CASES))
def test_memory_restatement_equals_reference(golden, name):
    want = case_of(golden, name)
    tabs, sas = pc.tables_of(pc.WORLDS[MEMORY_CASES[name]]())
    inst = int(want['cfg'][0])
    rm, rp = pc.memory_rngs(SEED, inst)
    mem = pc.RefPMAMemory(sas, RefEpsilonGreedy(0.1, rp), gamma_q=0.99, rng=rm)

    def give_sr(k):
        mem.SR = np.array(want['SR'][k])

    def give_need(k):
        mem.need_given = np.array(want['need'][k])

    got = pc.ScriptMemory(mem, pc.masked_actions(tabs), sr=give_sr, need=give_need,
                          index=lambda m: (m.rng.index, m.policy.rng.index)).run(pc.loads(want['ops']))
    pc.assert_same_record(got, want, what=name)
    assert len(want['need']) >= 1 and len(want['replayed']) > 100


def run_agent(want, no_replay, trials, steps=400, batch=8):
    tabs, sas = pc.tables_of(pc.demo_world())
    env, agent, mem = pc.make_ref_agent(tabs, sas, SEED, 0)
    agent.mask_actions = True
    k = [0]

    def give_sr():
        mem.SR = np.array(want['sr'][k[0]])
        k[0] += 1

    agent.update_sr = give_sr
    tr = pc.new_trace()
    agent.train(env, trials, steps, batch, no_replay, trace=tr)
    return env, agent, mem, tr


def test_agent_restatement_equals_reference(golden):
    want = case_of(golden, 'agent_demo')
    env, agent, mem, tr = run_agent(want, False, len(want['steps']))
    assert np.array_equal(np.array(tr['steps']), want['steps'])
    assert np.array_equal(np.array(tr['replay_start']), want['replay_start'])
    assert np.array_equal(np.array(tr['replay_end']), want['replay_end'])
    assert np.array_equal(np.array(tr['q_start']), want['q_replay'][0::2])
    assert np.array_equal(np.array(tr['q_end']), want['q_replay'][1::2])
    assert np.array_equal(np.array(tr['q_end']), want['q_end'])
    assert np.array_equal(mem.T, want['T']) and np.array_equal(mem.rewards, want['rewards'])
    assert np.array_equal(mem.states, want['states']) and np.array_equal(mem.terminals, want['terminals'])
    assert [env.rng.index, agent.policy.rng.index, mem.rng.index,
            mem.policy.rng.index] == want['index'].tolist()
    assert (np.array(tr['last']) == 4).all()


def test_agent_no_replay_restatement_equals_reference(golden):
    want = case_of(golden, 'agent_no_replay')
    env, agent, mem, tr = run_agent(want, True, len(want['steps']))
    assert np.array_equal(np.array(tr['steps']), want['steps'])
    assert np.array_equal(np.array(tr['q_end']), want['q_end'])
    assert np.array_equal(mem.T, want['T'])
    assert [env.rng.index, agent.policy.rng.index, mem.rng.index,
            mem.policy.rng.index] == want['index'].tolist()
