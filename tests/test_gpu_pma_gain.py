"""PMAMemory's observables on the device (csrc/pma_gain.hip) — ``compute_gain_batch``,
``compute_gain``, ``action_probs_batch``, ``update_q`` and ``PMA.update_q`` — against the NumPy
restatement of tests/pma_common.py, which tests/test_host_pma_gain.py holds against the real
reference.  Every comparison is ``np.array_equal``.  The cases are those of
tests/pma_gain_common.py: worlds of 48, 100, 72 (eight actions), 6 (one action) and 528 (132 states,
a wide memory) backups; three instances at ``instance_base`` 3, each filled by its own walk; with
and without an action mask; Q tables that are zero, random per instance, tied, and that do and do
not change the greedy action; sequences of 1 .. ``PMA_MAX_SEQ`` steps in both gain modes.  The
restatement of a case is computed once and shared."""
import numpy as np
import pytest
import torch

import pma_common as pc
import pma_gain_common as gc
from conftest import SEED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('as_tensor', [False, True], ids=['numpy', 'tensor'])
@pytest.mark.parametrize('name', list(gc.WORLDS))
def test_observables_match_the_restatement(name, as_tensor):
    """All four methods on every table, mask, mode and sequence of the case; the Q tables as NumPy
    arrays or as device tensors, ``[S, A]`` shared or ``[N, S, A]``; counters at rest."""
    case = gc.build(name)
    assert (case['S'] > 128) == case['wide']
    gc.assert_same(gc.device_observables(case, SEED, as_tensor), gc.expected(name), name)


def test_results_have_the_documented_forms():
    case = gc.build('small_3x4')
    S, A = case['S'], case['A']
    mem = gc.device_memory(case, SEED)
    g = mem.compute_gain_batch(case['Q']['zero'], None)
    assert torch.is_tensor(g) and g.dtype == torch.float64 and tuple(g.shape) == (gc.N, A * S)
    g = mem.compute_gain(case['Q']['zero'], None, [case['seqs']['len2'], case['seqs']['len1']])
    assert torch.is_tensor(g) and g.dtype == torch.float64 and tuple(g.shape) == (gc.N, 2)
    assert tuple(mem.compute_gain(case['Q']['zero'], None, []).shape) == (gc.N, 0)
    one = gc.device_memory(case, SEED, n=1)
    want = gc.expected('small_3x4')
    g = one.compute_gain_batch(case['Q']['ties'], case['mask'])
    assert isinstance(g, np.ndarray) and g.shape == (A * S,)
    assert np.array_equal(g, want['gain_batch/masked/ties'][0])
    g = one.compute_gain(case['Q']['flip'], None, [case['seqs'][k] for k in gc.seq_names('flip')])
    assert isinstance(g, np.ndarray) and np.array_equal(g, want['gain_seq/original/plain/flip'][0])
    Q = np.array(case['Q']['random'][0])
    back = one.update_q(Q, case['seqs']['len7'])            # [S, A] on a memory of one instance
    assert back is Q and np.array_equal(Q, want['update_q/len7'][0])
    for m in (mem, one):
        gc.assert_counters_rest(m)


@pytest.mark.parametrize('name', ['demo_5x5', 'eight_9x8'])
@pytest.mark.parametrize('mode', gc.MODES)
def test_per_instance_sequences_of_different_lengths(name, mode):
    """Three instances score / apply three different sequences (7, 2 and 32 steps) in one call."""
    case = gc.build(name)
    seqs = [case['seqs'][k] for k in ('len7', 'len2', 'len32')]
    other = [case['seqs'][k] for k in ('dead1', 'repeat', 'twice')]
    mem = gc.device_memory(case, SEED, mode)
    refs = gc.restatement_memories(case, mode)
    Q = case['Q']['random']
    for mask in (None, case['mask']):
        got = gc.host(mem.compute_gain(Q, mask, [gc.per_instance(seqs), gc.per_instance(other),
                                                 case['seqs']['len2']]))
        want = np.array([[refs[i].compute_gain(Q[i], mask, u[i]) for u in (seqs, other)]
                         + [refs[i].compute_gain(Q[i], mask, case['seqs']['len2'])]
                         for i in range(gc.N)])
        assert np.array_equal(got, want)
    for group in (seqs, other):
        got = torch.as_tensor(np.array(Q), device=mem.device)
        mem.update_q(got, gc.per_instance(group))
        want = np.array([refs[i].update_q(np.array(Q[i]), group[i]) for i in range(gc.N)])
        assert np.array_equal(gc.host(got), want)
        assert not np.array_equal(want[2], Q[2])
    gc.assert_counters_rest(mem)


@pytest.mark.parametrize('name', ['small_3x4', 'demo_5x5'])
def test_one_step_sequences_of_the_memory_s_records(name):
    """``compute_gain([[record of (s, a)]])`` beside ``compute_gain_batch[a * S + s]``, what the
    replay puts in the same slot of its gain vector: each against its own restatement (they
    normalise differently), for every pair the first walk stored."""
    case = gc.build(name)
    S = case['S']
    mem = gc.device_memory(case, SEED)
    refs = gc.restatement_memories(case)
    Q = case['Q']['random']
    pairs = sorted({(r[0], r[1]) for r in case['stores'][0]})
    ups = [[{k: [refs[i]._step(a * S + s)[k] for i in range(gc.N)] for k in pc.KEYS}]
           for s, a in pairs]
    for mask in (None, case['mask']):
        seq = gc.host(mem.compute_gain(Q, mask, ups))
        batch = gc.host(mem.compute_gain_batch(Q, mask))
        for i in range(gc.N):
            want_batch = refs[i].compute_gain_batch(Q[i], mask)
            for k, (s, a) in enumerate(pairs):
                assert seq[i, k] == refs[i].compute_gain(Q[i], mask, [refs[i]._step(a * S + s)])
                assert batch[i, a * S + s] == want_batch[a * S + s]
    gc.assert_counters_rest(mem)


def test_the_replay_performs_the_arg_max_of_the_exposed_maps():
    """One round of ``replay`` on the 5 x 5 case: the backup it performs is the arg-max of
    ``compute_gain_batch * compute_need * update_mask`` from the new call, in every instance."""
    case = gc.build('demo_5x5')
    S = case['S']
    mem = gc.device_memory(case, SEED)
    mem.compute_update_mask()
    Q, state = case['Q']['random'], 12
    gain = gc.host(mem.compute_gain_batch(Q, case['mask']))
    utility = gain * np.asarray(mem.compute_need(state)) * np.asarray(mem.update_mask)
    top = np.sort(utility, axis=1)
    assert (top[:, -1] > top[:, -2]).all(), 'a tie at the top: the draw would decide'
    gc.assert_counters_rest(mem)
    ups, _ = mem.replay(Q, case['mask'], 1, state)
    for i in range(gc.N):
        e = ups[i][0]
        assert e['action'] * S + e['state'] == int(np.argmax(utility[i])), i
    assert len({(u[0]['state'], u[0]['action']) for u in ups}) > 1, 'every instance chose alike'


@pytest.mark.parametrize('sname', ['len1', 'len7', 'twice', 'break', 'dead1', 'lenmax'])
def test_agent_update_q_equals_the_host_loop(sname):
    """``PMA.update_q`` on a bound agent of three instances (one device call) and the host loop of
    the unbound agent, instance by instance: the same bits."""
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    case = gc.build('demo_5x5')
    world = pc.demo_world()
    update = case['seqs'][sname]
    Q = case['Q']['random']

    def agent(env):
        mem = PMAMemory(world['sas'], EpsilonGreedy(gc.EPS), gamma_q=gc.GAMMA_Q)
        return PMA(env.observation_space, env.action_space, EpsilonGreedy(0.3), mem,
                   learning_rate=0.7, gamma=0.95)

    env = Gridworld(world, n_envs=gc.N, seed=SEED, instance_base=gc.BASE)
    bound = agent(env)
    bound._bind(env)
    assert bound._q is not None
    bound.Q = Q
    bound.update_q(update)
    got = bound.Q.cpu().numpy()
    for i in range(gc.N):
        loop = agent(env)
        assert loop._q is None
        loop.Q = Q[i]
        loop.update_q(update)
        assert np.array_equal(got[i], loop.Q), i
    assert np.array_equal(got, Q) == (sname == 'break')
    assert not bool(bound.M.counter.any())


@pytest.mark.parametrize('A', gc.PROB_ACTIONS)
@pytest.mark.parametrize('rows', gc.PROB_ROWS)
def test_action_probs_batch(rows, A):
    """Tables of 1, 63, 64, 65 and 257 rows and 1, 4 and 8 actions, with and without a mask,
    NumPy in and out and tensor in and out, on a memory that was never bound."""
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(gc.build('small_3x4')['sas'], EpsilonGreedy(gc.EPS))
    for masked in (False, True):
        q, mask = gc.prob_case(rows, A, masked)
        want = gc.probs_restated(q, mask)
        got = mem.action_probs_batch(q, mask)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert np.array_equal(got, want), (rows, A, masked)
        got = mem.action_probs_batch(torch.as_tensor(q, device='cuda'), mask)
        assert torch.is_tensor(got) and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert mem.counter is None and mem.policy.counter is None
