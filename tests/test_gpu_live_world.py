"""Worlds edited between calls, on the GPU: every golden case of tests/golden/gen_live_world.py
bit for bit (the reference's own runs with float32 tables), all instances against the C oracle
whose world the test swaps between phases, the environment's own step / reset with edits between
single steps, the update's stream order and its refusal.

Every test here runs under its own time limit (``_time_limit`` below): a kernel that hung behind
a bad update ends the process with a traceback instead of hanging the suite."""
import faulthandler

import numpy as np
import pytest

import live_world_common as L
from conftest import SEED

pytestmark = pytest.mark.gpu

D = L.load()


@pytest.fixture(autouse=True)
def _time_limit():
    """300 s per test (the slowest, the headline shape, takes a few seconds): past it the
    interpreter dumps every thread's traceback and exits."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def _setup(golden_worlds, name, n, base, stream_rows=False, callbacks=None):
    from cobel_amd.agent import SR, DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    kind, inst, B, phases = L.case(D, name)
    world = L.product_world(golden_worlds('walls_8x8'), L.tables(D, name, 0))
    env = Gridworld(world, n_envs=n, seed=SEED, instance_base=base)
    cls = SR if kind == 'sr' else DynaQ
    agent = cls(env.observation_space, env.action_space, EpsilonGreedy(0.1),
                custom_callbacks=callbacks)
    agent.track_instances = True
    if kind == 'sr':
        agent.stream_rows = stream_rows
    return kind, inst, B, phases, world, env, agent


def _train(kind, agent, env, trials, steps, B):
    if kind == 'sr':
        agent.train(env, trials, steps)
    else:
        agent.train(env, trials, steps, B)


def _tables_of(kind, agent):
    if kind == 'sr':
        return dict(SR=agent._sr.cpu().numpy().astype(np.float64),
                    RW=agent._rw.cpu().numpy().astype(np.float64),
                    T=agent._T.cpu().numpy().astype(np.int64))
    r, s, t = L.unpack_model(agent.M.table.cpu().numpy())
    return dict(Q=agent._q.cpu().numpy().astype(np.float64), M_rewards=r, M_states=s,
                M_terminals=t)


def _oracle(kind, name, n, base, total):
    from oracle import c_oracle
    w0 = c_oracle.OracleWorld([L.tables(D, name, 0)])
    if kind == 'sr':
        return c_oracle.SROracle(w0, n, SEED, True, instance_base=base, trial_cap=total)
    return c_oracle.TabOracle(w0, n, c_oracle.AG_DYNAQ, SEED, True, instance_base=base,
                              trial_cap=total)


def _oracle_tables(kind, o):
    if kind == 'sr':
        return dict(SR=o.SR, RW=o.RW, T=o.T)
    return dict(Q=o.Q, M_rewards=o.MR, M_states=o.MS, M_terminals=o.MT)


def _oracle_phase(kind, o, name, p, done, steps, B):
    from oracle import c_oracle
    if p:
        o.world = c_oracle.OracleWorld([L.tables(D, name, p)])
    if kind == 'sr':
        o.run(done, steps)
    else:
        o.run(done, steps, B)


@pytest.mark.parametrize('name,stream_rows', [(n, False) for n in L.DETERMINISTIC + L.SLIPPERY] +
                         [('sr_rewards_1_3_9', True), ('sr_turns_slippery', True)])
def test_golden_and_oracle_eight_instances(torch_cuda, golden_worlds, name, stream_rows):
    """n_envs = 8: the golden's instance against the reference after every phase, and all eight
    against the C oracle — for the worlds of tables only: the C oracle steps transition tables
    and cannot draw a successor (oracle/cobel_oracle.c has no distribution rows), so the slippery
    cases are checked against the reference's own instance here and in the two tests below."""
    kind, inst, B, phases, world, env, agent = _setup(golden_worlds, name, 8, 0, stream_rows)
    total = sum(t for t, _ in phases)
    o = _oracle(kind, name, 8, 0, total) if name in L.DETERMINISTIC else None
    done = 0
    for p, (trials, steps) in enumerate(phases):
        if p:
            L.edit_world(world, L.tables(D, name, p))
        _train(kind, agent, env, trials, steps, B)
        done += trials
        got = _tables_of(kind, agent)
        for key, v in got.items():
            assert np.array_equal(v[inst], D['%s/phase%d/%s' % (name, p, key)]), (p, key)
        if o is not None:
            _oracle_phase(kind, o, name, p, done, steps, B)
            for key, v in _oracle_tables(kind, o).items():
                assert np.array_equal(got[key], v), (p, key)
    lat = agent.monitors.lat_trace.cpu().numpy()
    assert np.array_equal(lat[inst, :total], D[name + '/steps'])
    if o is not None:
        assert np.array_equal(lat[:, :total], o.lat_trace[:, :total])
    assert env.handle.stochastic == (name in L.SLIPPERY)


@pytest.mark.parametrize('name', L.DETERMINISTIC + L.SLIPPERY)
def test_golden_single_instance(torch_cuda, golden_worlds, name):
    """n_envs = 1, one launch per phase."""
    inst = L.case(D, name)[1]             # (instance number = instance_base + 0)
    kind, inst, B, phases, world, env, agent = _setup(golden_worlds, name, 1, inst)
    for p, (trials, steps) in enumerate(phases):
        if p:
            L.edit_world(world, L.tables(D, name, p))
        _train(kind, agent, env, trials, steps, B)
        for key, v in _tables_of(kind, agent).items():
            assert np.array_equal(v[0], D['%s/phase%d/%s' % (name, p, key)]), (p, key)
    total = sum(t for t, _ in phases)
    assert np.array_equal(agent.monitors.lat_trace.cpu().numpy()[0, :total], D[name + '/steps'])


@pytest.mark.parametrize('name', L.DETERMINISTIC + L.SLIPPERY)
def test_edit_from_a_trial_callback(torch_cuda, golden_worlds, name):
    """ONE train() call over all phases; the edits are made by an on_trial_end callback at the
    last trial of each phase, so the sync in front of the next trial's launch has to see them —
    the reference would at its very next reset."""
    kind, inst, B, phases = L.case(D, name)
    ends, acc = {}, 0
    for p, (trials, _) in enumerate(phases[:-1]):
        acc += trials
        ends[acc - 1] = p + 1
    box = {}

    def on_trial_end(logs):
        p = ends.get(int(logs['trial']))
        if p is not None:
            L.edit_world(box['world'], L.tables(D, name, p))
        return logs

    kind, inst, B, phases, world, env, agent = _setup(
        golden_worlds, name, 1, inst, callbacks={'on_trial_end': [on_trial_end]})
    box['world'] = world
    total = sum(t for t, _ in phases)
    _train(kind, agent, env, total, phases[0][1], B)
    last = len(phases) - 1
    for key, v in _tables_of(kind, agent).items():
        assert np.array_equal(v[0], D['%s/phase%d/%s' % (name, last, key)]), key
    assert np.array_equal(agent.monitors.lat_trace.cpu().numpy()[0, :total], D[name + '/steps'])


def test_gridworld_step_and_reset_known_answers(torch_cuda, golden_worlds):
    """Gridworld.step / reset themselves, edits between single steps."""
    from cobel_amd.interface import Gridworld
    t0 = L.tables(D, 'dynaq_reversal', 0)
    world = L.product_world(golden_worlds('walls_8x8'), t0)
    env = Gridworld(world, n_envs=1, seed=SEED, instance_base=int(D['env_kat/instance']))
    for op, arg, s, r, end in D['env_kat/rows']:
        if op == 2:
            L.edit_world(world, L.tables(D, 'env_kat', int(arg), prefix='edit'))
            assert env.current_state == int(s)
        elif op == 0:
            assert env.reset()[0] == int(s)
        else:
            assert env.step(int(arg))[:3] == (int(s), r, bool(end))


def test_topology_step_and_reset_follow_the_nodes(torch_cuda):
    """Topology.step / reset read the node dictionary and starting_nodes anew (topology.py:126-172):
    a three-neighbour ring, answers worked out by hand."""
    from cobel_amd.interface import Topology
    ids = ['a', 'b', 'c', 'd']
    nodes = {k: dict(pose=(float(i), 0.0, 0.0, 0.0, 0.0, 0.0), reward=0.0, terminal=False,
                     neighbors=[ids[(i + 1) % 4], ids[(i + 3) % 4], k]) for i, k in enumerate(ids)}
    nodes['d'].update(reward=1.0, terminal=True)
    env = Topology(nodes, starting_nodes=['a'], seed=5)
    assert env.current_node == 'a'
    assert env.step(0)[1:3] == (0.0, False) and env.current_node == 'b'
    nodes['c'].update(reward=0.5, terminal=True)           # edited in place
    assert env.step(0)[1:3] == (0.5, True) and env.current_node == 'c'
    nodes['d'].update(reward=-2.0, terminal=False)
    assert env.step(0)[1:3] == (-2.0, False) and env.current_node == 'd'
    env.starting_nodes = ['c']                              # replaced
    env.reset()
    assert env.current_node == 'c'
    nodes['c']['neighbors'][0] = 'a'                        # rewired: c --0--> a
    assert env.step(0)[1:3] == (0.0, False) and env.current_node == 'a'
    assert env.sync_world() is False
    nodes['a']['neighbors'].append('b')
    with pytest.raises(ValueError):
        env.step(0)


def test_back_to_back_and_a_refused_update(torch_cuda, golden_worlds):
    """train, edit + sync_world, train, with no read of the device in between: the phase boundary
    is the launch boundary.  (train() itself ends with a check of its launch that waits for the
    stream, so the update here follows a drained stream; the order of an update against launches
    still IN FLIGHT is what test_headline_shape_reward_moved_in_every_maze pins: three _launch
    calls, sync_world, three more, one synchronize.)  Then an update the library refuses (a
    successor outside the world) returns its error and leaves the world as it was: the next run
    equals the oracle on the old world."""
    torch = torch_cuda
    from cobel_amd import _lib
    name = 'dynaq_reversal'
    kind, inst, B, phases, world, env, agent = _setup(golden_worlds, name, 8, 0)
    (t0, steps), (t1, _) = phases
    o = _oracle(kind, name, 8, 0, t0 + 2 * t1)
    agent.train(env, t0, steps, B)
    L.edit_world(world, L.tables(D, name, 1))
    assert env.sync_world() is True and env.sync_world() is False
    agent.train(env, t1, steps, B)
    torch.cuda.synchronize()
    _oracle_phase(kind, o, name, 0, t0, steps, B)
    _oracle_phase(kind, o, name, 1, t0 + t1, steps, B)
    for key, v in _oracle_tables(kind, o).items():
        assert np.array_equal(_tables_of(kind, agent)[key], v), key
    host = {k: v.copy() for k, v in env.handle._host.items() if k != 'lists'}
    host['next'][0, 17, 2] = 64
    rc = _lib.lib().cobel_world_update(
        env.handle.ptr, host['next'].ctypes.data, host['reward'].ctypes.data,
        host['terminal'].ctypes.data, host['starts'].ctypes.data, host['off'].ctypes.data,
        _lib.current_stream(env.device))
    assert rc == _lib.E_RANGE
    host['next'][0, 17, 2] = 17
    host['starts'][0] = 64
    with pytest.raises(IndexError):
        env.handle._push_tables(host, _lib.current_stream(env.device))
    agent.train(env, t1, steps, B)
    o.run(t0 + 2 * t1, steps, B)
    for key, v in _oracle_tables(kind, o).items():
        assert np.array_equal(_tables_of(kind, agent)[key], v), key
    assert np.array_equal(agent.monitors.lat_trace.cpu().numpy(), o.lat_trace)


def test_headline_shape_reward_moved_in_every_maze(torch_cuda):
    """Dyna-Q at the headline's shape (32x32 obstacle mazes, 64 worlds, 65 536 instances on the
    persistent-workgroup kernel): the reward moved in every maze between two launches; a fixed
    sample of instances against the C oracle."""
    torch = torch_cuda
    import bench
    from oracle import c_oracle
    n = 65536
    cfg = dict(bench.CONFIGS['C3'])
    env, agent = bench.build_agent('C3', cfg, n, 0, torch.device('cuda', 0))
    runner = bench.Runner(cfg, env, agent)
    assert runner.describe()['kernel'] == runner._lib.TAB_KERNEL_PWG

    def oracle_world():
        return c_oracle.OracleWorld([dict(next=w['next'], reward=w['rewards'],
                                          terminal=w['terminals'], starts=w['starting_states'])
                                     for w in env.worlds])
    worlds = [oracle_world()]
    for _ in range(3):
        runner.launch()
    for k, w in enumerate(env.worlds):          # goal (and its terminal flag) to another free cell
        free = [int(s) for s in w['starting_states']]
        new = free[(37 * k + 11) % len(free)]
        old = int(np.flatnonzero(w['rewards'])[0])
        w['rewards'][old], w['rewards'][new] = 0.0, 1.0
        w['terminals'][old], w['terminals'][new] = 0, 1
        w['starting_states'] = np.array([s for s in free if s != new] + [old])
    assert env.sync_world() is True
    worlds.append(oracle_world())
    for _ in range(3):
        runner.launch()
    torch.cuda.synchronize()
    ids = np.unique(np.concatenate([np.arange(0, n, 4099), [1, 63, 64, n - 1]]))[:16]
    sel = torch.as_tensor(ids, device='cuda')
    q = agent._q[sel].cpu().numpy().astype(np.float64)
    m_r, m_s, m_t = L.unpack_model(agent.M.table[sel].cpu().numpy())
    inst = agent.inst[sel].cpu().numpy()
    for k, g in enumerate(ids):
        o = c_oracle.TabOracle(worlds[0], 1, c_oracle.AG_DYNAQ, env.seed, True, instance_base=int(g))
        for launch in range(6):
            o.world = worlds[launch // 3]
            o.run(0x7fffffff, cfg['steps_per_trial'], cfg['batch'],
                  step_budget=cfg['env_steps_per_launch'])
        assert np.array_equal(q[k], o.Q[0]), g
        assert np.array_equal(m_r[k], o.MR[0]) and np.array_equal(m_s[k], o.MS[0]), g
        assert np.array_equal(m_t[k], o.MT[0]), g
        for col, key in ((0, 'state'), (1, 'step'), (2, 'trial'), (3, 'ctr_env'),
                         (4, 'ctr_policy'), (5, 'ctr_memory')):
            assert int(inst[k, col]) == int(o.inst[key][0]), (g, key)


# ---------------------------------------------------------------------------------------------
# QAgent on a hexagonal Topology (six actions: cobel_world_create_n handle, the wavefront kernel of
# csrc/tabular_nact.hip or the general kernel), nodes edited and starting_nodes replaced.
def _hex_setup(n, base):
    from cobel_amd.agent import QAgent
    from cobel_amd.interface import Topology
    from cobel_amd.policy import EpsilonGreedy
    nodes, starts = L.hex_nodes()
    ids = [str(k) for k in D[L.HEX + '/ids']]
    assert list(nodes.keys()) == ids
    env = Topology(nodes, starts, n_envs=n, seed=SEED, instance_base=base)
    assert int(env.action_space.n) == 6 and env.handle.n_actions == 6
    t0 = L.tables(D, L.HEX, 0)
    assert np.array_equal(env.handle._host['next'][0], t0['next'])
    assert np.array_equal(env.handle._host['starts'], t0['starts'])
    agent = QAgent(env.observation_space, env.action_space, EpsilonGreedy(0.1))
    agent.track_instances = True
    return env, agent, ids


@pytest.mark.parametrize('n', [1, 8])
def test_qagent_on_an_edited_hexagonal_topology(torch_cuda, n):
    """Every phase against the reference's run (instance `inst`: alone at n_envs = 1, one of
    eight at n_envs = 8), and at n_envs = 8 every instance against oracle/ref_loop.py driven by
    that instance's streams."""
    from test_oracle_live_world import hex_ref_run
    name = L.HEX
    _, inst, B, phases = L.case(D, name)
    env, agent, ids = _hex_setup(n, inst if n == 1 else 0)
    row = 0 if n == 1 else inst
    for p, (trials, steps) in enumerate(phases):
        if p:
            L.edit_nodes(env, ids, L.tables(D, name, p))
        agent.train(env, trials, steps, B)
        q = agent._q.cpu().numpy().astype(np.float64)
        assert np.array_equal(q[row], D['%s/phase%d/Q' % (name, p)]), p
        assert int(agent.inst[row, 6].item()) == int(D['%s/phase%d/log_len' % (name, p)])
    total = sum(t for t, _ in phases)
    lat = agent.monitors.lat_trace.cpu().numpy()
    assert np.array_equal(lat[row, :total], D[name + '/steps'])
    if n > 1:
        for g in range(n):
            ag, tr, qs = hex_ref_run(D, g)
            assert np.array_equal(q[g], qs[-1]), g
            assert np.array_equal(lat[g, :total], tr['steps']), g


# ---------------------------------------------------------------------------------------------
# The branches of the update that move buffers: a start list outgrowing its capacity, successor
# lists put aside and taken back, successor lists outgrowing theirs.
def test_start_list_and_successor_lists_outgrow_their_buffers(torch_cuda):
    torch = torch_cuda
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_gridworld
    world = make_gridworld(8, 8, terminals=[7], rewards=np.array([[7, 1.0]]), starting_states=[3, 9])
    env = Gridworld(world, n_envs=4096, seed=77)
    assert set(env.state.cpu().numpy().tolist()) == {3, 9}
    many = np.arange(10, 60)                       # 2 -> 50 starts: a larger device buffer
    world['starting_states'] = many
    env.reset()
    assert set(env.state.cpu().numpy().tolist()) == set(many.tolist())
    world['starting_states'] = np.arange(8, 64)     # 56 > 50: it grows once more
    env.reset()
    assert set(env.state.cpu().numpy().tolist()) == set(range(8, 64))
    world['starting_states'] = np.array([20])
    env.reset()
    assert (env.state == 20).all()

    def step_counts(action):
        env.reset()
        ns = env.step(torch.full((4096,), action, dtype=torch.uint8, device='cuda'))[0]
        return {int(k): int(v) for k, v in zip(*np.unique(ns.cpu().numpy(), return_counts=True))}

    assert step_counts(2) == {21: 4096}             # tables: right of 20
    sas = world['sas']
    sas[20, 2, 21], sas[20, 2, 12] = 0.5, 0.5       # slippery (lists on a handle that had none)
    world['deterministic'] = False
    c = step_counts(2)
    assert set(c) == {12, 21} and min(c.values()) > 1700 and env.handle.stochastic
    sas[20, 2, 21], sas[20, 2, 12] = 1.0, 0.0       # one-hot again: the lists are put aside
    assert step_counts(2) == {21: 4096} and not env.handle.stochastic
    sas[20, 2, 21], sas[20, 2, 12] = 0.25, 0.75     # taken back, same length
    c = step_counts(2)
    assert set(c) == {12, 21} and c[12] > 2 * c[21] and env.handle.stochastic
    for s in range(64):                             # every row spreads: lists outgrow their buffers
        for a in range(4):
            row = sas[s, a]
            row[:] = 0.0
            row[[s, (s + 1) % 64, (s + 9) % 64, (s + 17) % 64]] = 0.25
    c = step_counts(1)
    assert set(c) == {20, 21, 29, 37} and min(c.values()) > 800
    sas[20, 1, :] = 0.0
    sas[20, 1, 5] = 1.0                             # in place again, shorter
    assert step_counts(1) == {5: 4096}
    world['deterministic'] = True                   # argmax of the rows: tables again
    assert step_counts(1) == {5: 4096} and not env.handle.stochastic


# ---------------------------------------------------------------------------------------------
# The network agents take interface.handle.ptr themselves (cobel_dqn_act).
def _mlp(n_in, n_out):
    """The 64-64 ReLU network of the reference's demos, in the form the two-kernel loop takes."""
    import torch
    from collections import OrderedDict
    return torch.nn.Sequential(OrderedDict([
        ('flatten', torch.nn.Flatten()),
        ('dense_1', torch.nn.Linear(n_in, 64)), ('relu_1', torch.nn.ReLU()),
        ('dense_2', torch.nn.Linear(64, 64)), ('relu_2', torch.nn.ReLU()),
        ('output', torch.nn.Linear(64, n_out))])).double()


def test_dqn_ring_holds_the_edited_rewards_and_terminals(torch_cuda):
    """DQN on a Topology (the two-kernel loop): what cobel_dqn_act writes into the replay ring
    after an edit of the nodes is the NEW table's reward and terminal flag of the node entered;
    what it wrote before stays the old table's."""
    torch = torch_cuda
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Topology
    from cobel_amd.misc.topology_tools import linear_track
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    nodes, starts = linear_track(10, 2, 1.0, 20, 'right')
    env = Topology(nodes, starts, n_envs=8, seed=SEED)
    ids = env.ids
    agent = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.3),
                TorchNetwork(_mlp(6, int(env.action_space.n))))
    tables = []

    def table():
        return (np.array([nodes[k]['reward'] for k in ids], dtype=np.float64),
                np.array([bool(nodes[k]['terminal']) for k in ids]))

    tables.append(table())
    agent.train(env, 4, 25, 32)
    fused0 = agent.fused_steps
    assert fused0 > 0
    size0 = agent.M.size.cpu().numpy().copy()
    goal = [k for k in ids if nodes[k]['terminal']]
    for i, k in enumerate(ids):                      # every node pays something of its own
        nodes[k]['reward'] = (i + 1) / 64.0
        nodes[k]['terminal'] = False
    nodes[ids[len(ids) // 2]]['terminal'] = True      # the end moves to the middle
    assert goal and not nodes[goal[0]]['terminal']
    tables.append(table())
    agent.train(env, 4, 25, 32)
    assert agent.fused_steps > fused0
    size1 = agent.M.size.cpu().numpy()
    assert (agent.M.head.cpu().numpy() == 0).all() and (size1 > size0).all()
    pose = np.asarray(env.pose)
    nxt = agent.M.next_states.cpu().numpy()
    rew = agent.M.rewards.cpu().numpy()
    nonterm = agent.M.terminals.cpu().numpy()
    for i in range(8):
        for lo, hi, (r_tab, t_tab) in ((0, size0[i], tables[0]), (size0[i], size1[i], tables[1])):
            rows = nxt[i, lo:hi].reshape(hi - lo, -1)
            node = np.array([int(np.flatnonzero((pose == row).all(axis=1))[0]) for row in rows])
            assert np.array_equal(rew[i, lo:hi], r_tab[node]), (i, lo)
            assert np.array_equal(nonterm[i, lo:hi], 1.0 - t_tab[node]), (i, lo)
    assert rew[:, :size0.min()].max() <= 20.0 and (rew[0, size0[0]:size1[0]] < 1.0).all()


def test_dyna_dqn_model_follows_edits_and_a_world_turning_slippery(torch_cuda):
    """DynaDQN on a Gridworld, model learning rate 1 so that a stored entry IS the reward of the
    state entered: entries written after an edit hold the new table's values (two-kernel loop);
    after the world turns slippery handle.stochastic sends the session to the PyTorch loop — the
    branch is taken AFTER the edit — and its entries hold the newest table's values."""
    torch = torch_cuda
    from cobel_amd.agent import DynaDQN
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_open_field
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    world = make_open_field(5, 5, 0, 1)
    env = Gridworld(world, n_envs=8, seed=SEED)
    agent = DynaDQN(env.observation_space, env.action_space, EpsilonGreedy(0.3),
                    TorchNetwork(_mlp(25, 4)), gamma=0.8)
    agent.M.learning_rate = 1.0

    def snapshot():
        return (agent.M.rewards.cpu().numpy().copy(), agent.M.states.cpu().numpy().copy(),
                agent.M.terminals.cpu().numpy().copy())

    def written_since(before, reward_tab, terminal_tab):
        r, s, t = snapshot()
        changed = (r != before[0]) | (s != before[1]) | (t != before[2])
        assert changed.sum() > 40
        assert np.array_equal(r[changed], reward_tab[s[changed]])
        assert np.array_equal(t[changed], 1.0 - terminal_tab[s[changed]])

    agent.train(env, 4, 20, 32)
    fused0 = agent.fused_steps
    assert fused0 > 0 and not env.handle.stochastic
    before = snapshot()
    world['rewards'][:] = (np.arange(25) + 1) / 64.0          # in place
    world['terminals'][:] = 0
    world['terminals'][12] = 1
    agent.train(env, 4, 20, 32)
    fused1 = agent.fused_steps
    assert fused1 > fused0
    written_since(before, world['rewards'], world['terminals'] != 0)
    before = snapshot()
    world['sas'] = L.slippery_sas(np.asarray(world['next']), 0.4)
    world['deterministic'] = False
    world['rewards'][:] = -(np.arange(25) + 1) / 128.0
    world['terminals'][12], world['terminals'][24] = 0, 1
    agent.train(env, 4, 20, 32)
    assert env.handle.stochastic and agent.fused_steps == fused1
    written_since(before, world['rewards'], world['terminals'] != 0)
