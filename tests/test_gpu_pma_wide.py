"""PMA's wide form on the device (csrc/pma.hip's second instantiation, csrc/pma_sr.hip): worlds of
132, 272 and 1 024 states against the fixture recorded from the reference and against the NumPy
restatement, bit for bit; a narrow-size script through the wide instantiation; the blocked
update_sr against the LDS kernel and an element-wise restatement bit for bit, and against
numpy.linalg.inv within the derived bound."""
import os

import numpy as np
import pytest

import pma_common as pc
import pma_wide_common as pw
from pma_common import gauss_jordan
from oracle.ref_loop import RefEpsilonGreedy

pytestmark = pytest.mark.gpu

SEED = pw.SEED
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'pma_wide_traces.npz'))


def case_of(golden, name):
    return {k.split('/', 1)[1]: golden[k] for k in golden.files if k.startswith(name + '/')}


def device_memory(world, n, base, wide=True, gamma=0.9):
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma=gamma, gamma_q=0.99, wide=wide)
    mem.bind(n, seed=SEED, instance_base=base)
    return mem


def dev_index(pick):
    return lambda m: (int(m.counter[pick].item()), int(m.policy.counter[pick].item()))


@pytest.mark.parametrize('n_envs', [1, 8])
@pytest.mark.parametrize('name', sorted(pw.MEMORY_CASES))
def test_memory_equals_reference(golden, name, n_envs):
    """The fixture's script of stores and replays on 132 and 272 states; instance 0 is the
    fixture's.  The SR row of each replay and the need vector of the ``None`` replay are uploaded
    from the fixture."""
    want = case_of(golden, name)
    world = pw.WORLDS[pw.MEMORY_CASES[name][0]]()
    tabs, _ = pc.tables_of(world)
    S = int(world['states'])
    ops = pc.loads(want['ops'])
    states = pw.replay_states(ops)
    mem = device_memory(world, n_envs, int(want['cfg'][0]))

    def give_sr(k):
        mem.SR = pw.sr_of_row(S, states[k], want['SR'][k])

    def give_need(k):
        mem.compute_need = lambda state=None, instances=None: np.array(want['need'][k])

    got = pc.ScriptMemory(mem, pc.masked_actions(tabs), pick=None if n_envs == 1 else 0,
                          sr=give_sr, need=give_need, index=dev_index(0)).run(ops)
    pc.assert_same_record(got, want, what=name)


@pytest.mark.parametrize('n_envs', [1, 8])
def test_agent_equals_reference(golden, n_envs):
    """PMA.train on the 132-state world with mask_actions; instance 0 is the fixture's.
    ``M.update_sr`` is replaced by a method that uploads trial k's recorded SR rows."""
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    want = case_of(golden, 'agent_wide')
    trials = len(want['steps'])
    tr = []
    first = (lambda x: x) if n_envs == 1 else (lambda x: x[0])
    env = Gridworld(pw.WORLDS[pw.AGENT_WORLD](), n_envs=n_envs, seed=SEED)
    mem = PMAMemory(env.world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=True)
    agent = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem,
                custom_callbacks={'on_replay_end': [
                    lambda logs: tr.append(pc.rows_of(first(logs['replay'])))]})
    agent.mask_actions = True
    agent.track_instances = True
    S = mem.nb_states
    k = [0]

    def give_sr():
        sr = np.array(mem.SR).reshape(n_envs, S, S)
        sr[0] = 0.0
        sr[0][want['sr_states']] = want['sr_rows'][k[0]]
        mem.SR = sr
        k[0] += 1

    mem.update_sr = give_sr
    agent.train(env, trials, pw.AGENT_STEPS, pw.AGENT_BATCH)
    q = np.array(agent.Q.cpu().numpy()[0] if n_envs > 1 else agent.Q)
    lat = agent.monitors.lat_trace.cpu().numpy()[0]
    assert np.array_equal(lat[:trials], want['steps'])
    assert np.array_equal(np.array(tr[0::2]), want['replay_start'])
    assert np.array_equal(np.array(tr[1::2]), want['replay_end'])
    assert np.array_equal(q, want['q_end'][-1])
    pick = (lambda a: np.asarray(a)) if n_envs == 1 else (lambda a: np.asarray(a)[0])
    assert np.array_equal(pick(mem.T), want['T'])
    assert np.array_equal(pick(mem.rewards), want['rewards'])
    assert np.array_equal(pick(mem.states), want['states'])
    assert np.array_equal(pick(mem.terminals), want['terminals'])
    idx = [int(env.env_ctr[0].item()), int(agent.policy.counter[0].item()),
           int(mem.counter[0].item()), int(mem.policy.counter[0].item())]
    assert idx == want['index'].tolist()


def test_narrow_script_through_the_wide_form():
    """The 5 x 5 demo script of the narrow fixture (read only) run through the wide instantiation:
    the same records, Q, tables and generator indices."""
    narrow = np.load(os.path.join(HERE, 'golden', 'pma_traces.npz'))
    want = case_of(narrow, 'mem_demo_5x5')
    world = pc.demo_world()
    tabs, _ = pc.tables_of(world)
    mem = device_memory(world, 1, int(want['cfg'][0]))
    assert mem.wide

    def give_sr(k):
        mem.SR = want['SR'][k]

    def give_need(k):
        mem.compute_need = lambda state=None, instances=None: np.array(want['need'][k])

    got = pc.ScriptMemory(mem, pc.masked_actions(tabs), sr=give_sr, need=give_need,
                          index=dev_index(0)).run(pc.loads(want['ops']))
    pc.assert_same_record(got, want, what='demo script, wide form')


def filled(world, n, wide, gamma=0.9, stores=40):
    tabs, _ = pc.tables_of(world)
    mem = device_memory(world, n, 0, wide=wide, gamma=gamma)
    rows = pc.walk_stores(tabs, stores, seed=3)
    for s, a, r, ns, t in rows:
        # instance 1 sees another experience: its T differs from instance 0's
        mem.store({'state': [s, rows[0][0]][:n], 'action': [a, rows[0][1]][:n], 'reward': r,
                   'next_state': [ns, rows[0][3]][:n], 'terminal': t})
    return mem


@pytest.mark.parametrize('shape', [(5, 5), (8, 16)])
def test_blocked_update_sr_equals_the_lds_kernel(shape, monkeypatch):
    """S = 25 (less than one panel of 32 pivots: the diagonal block is the whole matrix, so only
    k_pma_sr_diag runs) and S = 128 (four whole panels, 2 x 2 tiles, all three kernels): the blocked
    kernels, forced, give the LDS kernel's SR bit for bit.  Partial panels and partial tiles are
    test_blocked_update_sr_beyond_the_lds's."""
    world = pc.demo_world() if shape == (5, 5) else pc.seeded_world(8, 16, seed=8)
    mem = filled(world, 2, wide=False)
    mem.update_sr()
    lds = np.array(mem.SR)
    mem.SR = np.zeros_like(lds)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PMA_SR', 'blocked')
    mem.update_sr()
    blocked = np.array(mem.SR)
    monkeypatch.delenv('COBEL_DEBUG_PMA_SR')
    monkeypatch.delenv('COBEL_DEBUG')
    assert np.isfinite(lds).all() and not np.array_equal(lds[0], lds[1])
    assert np.array_equal(blocked, lds)


@pytest.mark.parametrize('world,gamma', [('wide_12x11', 0.9), ('wide_12x11', 0.99),
                                         ('wide_17x16', 0.9)])
def test_blocked_update_sr_beyond_the_lds(world, gamma):
    """S = 132 and 272, no multiples of the 64-wide tile nor of the 32-pivot panel (132 = 4 panels + 4
    pivots, 272 = 8 panels + 16 pivots): against numpy.linalg.inv within the derived bound, and
    against the element-wise restatement of the LDS kernel bit for bit."""
    mem = filled(pw.WORLDS[world](), 2, wide=True, gamma=gamma)
    mem.update_sr()
    T, SR = np.asarray(mem.T), np.asarray(mem.SR)
    S = T.shape[1]
    tol = pw.sr_bound(S, gamma)
    for i in range(2):
        want = np.linalg.inv(np.eye(S) - gamma * T[i])
        err = np.abs(SR[i] - want).max()
        print('update_sr S = %d gamma %g: max abs error %.3e (bound %.3e)' % (S, gamma, err, tol))
        assert err <= tol
        assert np.array_equal(SR[i], gauss_jordan(T[i], gamma))


def test_top_of_the_range_32x32():
    """1 024 states, four actions, replay_length 8: the plan accepts it; one store walk plus one
    replay equals the restatement; one update_sr meets the bound against numpy.linalg.inv."""
    world = pw.world_1024()
    tabs, sas = pc.tables_of(world)
    S, L, inst = 1024, 8, 4
    mem = device_memory(world, 1, inst)
    plan = mem.launch_plan(L)
    assert 120 * 1024 < plan[0] <= 160 * 1024 and plan[1] == 64
    rm, rp = pc.memory_rngs(SEED, inst)
    ref = pc.RefPMAMemory(sas, RefEpsilonGreedy(0.1, rp), gamma_q=0.99, rng=rm)
    stores = pc.walk_stores(tabs, 40, seed=7, repeat=(5, 2))
    assert any(r[4] == 0 for r in stores) and all(r[0] > 255 for r in stores)
    start = int(tabs['starts'][0])
    ops = [['store'] + r for r in stores] + [['replay', L, start, None, True]]
    mask = pc.masked_actions(tabs)
    want = pc.ScriptMemory(ref, mask, index=lambda m: (m.rng.index, m.policy.rng.index)).run(ops)
    got = pc.ScriptMemory(mem, mask, index=dev_index(0)).run(ops)
    pc.assert_same_record(got, want, keys=pc.RECORD_KEYS + ('SR',), what='32 x 32')
    assert (want['replayed'][:, 1] > 255).all()
    mem.update_sr()
    T, SR = np.asarray(mem.T), np.asarray(mem.SR)
    err = np.abs(SR - np.linalg.inv(np.eye(S) - 0.9 * T)).max()
    print('update_sr S = 1024: max abs error %.3e (bound %.3e)' % (err, pw.sr_bound(S, 0.9)))
    assert err <= pw.sr_bound(S, 0.9)
