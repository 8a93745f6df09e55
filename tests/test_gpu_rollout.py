"""``agent.rollout`` on the device: the fixture's trajectories, a twin run of ``test()``, the record's
own consistency, the per-instance restatement, composition of sessions, drawn successors and the
launch plan.  Every comparison is of integers or bit patterns.  The record's four tensors and ``Q``
sit inside sentinel frames (tests/frames_common.py) in every launch made here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import frames_common as fc
import rollout_common as rc
from conftest import GOLDEN, SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'rollout_traces.npz'))


# -- worlds ----------------------------------------------------------------------------------------------
def _grid(name):
    from cobel_amd.misc import gridworld_tools as gt
    if name in ('open5', 'walls8'):
        return [rc.grid_world(gt, name)]
    if name == 'tiny':          # 1 x 2: one move ends the trial, the others stay
        return [gt.make_gridworld(1, 2, terminals=[1], rewards=np.array([[1, 1.0]]), goals=[1],
                                  starting_states=[0])]
    if name == 'slippery':      # every row a distribution: the intended move, or staying put
        w = gt.make_open_field(5, 5, 0, 1)
        sas = w['sas']
        stay = np.zeros_like(sas)
        stay[np.arange(25), :, np.arange(25)] = 1.0
        sas[:] = 0.75 * sas + 0.25 * stay
        w['deterministic'] = False
        return [w]
    assert name == 'stack3'     # three different 5 x 5 worlds
    return [gt.make_open_field(5, 5, 0, 1),
            gt.make_gridworld(5, 5, terminals=[24], rewards=np.array([[24, 1.0], [12, 0.5]]),
                              goals=[24], invalid_states=[6, 7, 17], starting_states=[0, 4, 20]),
            gt.make_gridworld(5, 5, terminals=[12, 2], rewards=np.array([[12, 2.0], [2, -1.0]]),
                              goals=[12], invalid_transitions=[(0, 1), (1, 0)],
                              starting_states=[24, 20, 4, 10])]


def _setup(world, kind, n, eps, base=0, test_policy=True, mask=False, q_seed=1, seed=SEED):
    """Environment, agent (bound, a table of small multiples of 0.25 planted per instance: ties of
    every order) and the policy a test session selects with."""
    from cobel_amd.agent import DynaQ, QAgent
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.misc import topology_tools as tt
    from cobel_amd.policy import EpsilonGreedy
    if world in ('hex', 'track4'):
        nodes, starts = tt.hexagonal(4, (0.0, 1.0), 1.0, None) if world == 'hex' \
            else tt.linear_track(4, 1)
        env = Topology(nodes, starts, None, n_envs=n, seed=seed, instance_base=base)
    else:
        env = Gridworld(_grid(world), n_envs=n, seed=seed, instance_base=base)
    pol = EpsilonGreedy(eps)
    pol_test = EpsilonGreedy(eps) if test_policy else None
    cls = DynaQ if kind == 'dynaq' else QAgent
    ag = cls(env.observation_space, env.action_space, pol, pol_test)
    ag.track_instances = ag.track_occupancy = ag.track_responses = True
    ag._bind(env)
    if mask:
        ag.mask_actions = True
        ag.action_mask = rc.bump_mask(env.handle._host['next'][0])
    if q_seed is not None:
        g = torch.Generator(device='cuda').manual_seed(q_seed)
        ag.Q = torch.randint(0, 3, (n, ag.n_states, ag.n_actions), generator=g,
                             device='cuda').to(torch.float32) * 0.25
    return env, ag, ag.policy_test


def _framed_rollout(monkeypatch, ag, env, trials, steps, shift=0):
    """``ag.rollout`` with ``Q`` and the four tensors of the record inside sentinel frames, the
    guards checked after the launch."""
    from cobel_amd.monitor import trajectory
    frames = fc.Frames(shift)
    frames.swap(ag, '_q', fc.BIG)
    base = trajectory.TrajectoryRecord

    class Framed(base):
        def __init__(self, *args, **kwargs):
            base.__init__(self, *args, **kwargs)
            for name, poison in (('start', 0), ('states', 0), ('actions', 0), ('length', fc.MARK)):
                frames.swap(self, name, poison)

    monkeypatch.setattr(trajectory, 'TrajectoryRecord', Framed)
    rec = ag.rollout(env, trials, steps)
    monkeypatch.setattr(trajectory, 'TrajectoryRecord', base)
    torch.cuda.synchronize()
    frames.check()
    rec._frames = ag._frames = frames       # (the framed buffers live as long as their users)
    return rec


def _state(ag, env, pol) -> dict:
    """Everything a test session leaves behind, stripes folded."""
    mon = ag.monitors
    d = {k: getattr(mon, k) for k in ('lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt', 'lat_trace',
                                      'occupancy', 'steps_done')}
    d.update(inst=ag.inst, policy_counter=pol.counter, env_ctr=env.env_ctr, env_state=env.state,
             Q=ag._q, current_trial=np.int64(ag.current_trial))
    if hasattr(getattr(ag, 'M', None), 'counter'):       # Dyna-Q's memory draws from a stream
        d['memory_counter'] = ag.M.counter
    return {k: (v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v))
            for k, v in d.items()}


def _arrays(rec) -> dict:
    return {k: getattr(rec, k).cpu().numpy() for k in ('start', 'states', 'actions', 'length')}


def _consistent(rec, env, ag, drawn=False):
    """The record against the world's own tables."""
    a = _arrays(rec)
    host = env.handle._host
    n_worlds, steps = env.handle.n_worlds, rec.steps
    k = np.arange(steps)[None, None, :]
    live = k < a['length'][:, :, None]
    assert (a['length'] >= 1).all() and (a['length'] <= steps).all()
    assert (a['states'][~live] == rc.PAD_STATE).all()
    assert (a['actions'][~live] == rc.PAD_ACTION).all()
    assert (a['states'][live] >= 0).all() and (a['actions'][live] < ag.n_actions).all()
    world = (env.instance_base + np.arange(rec.n_envs)) % n_worlds
    w3 = np.broadcast_to(world[:, None, None], live.shape)
    prev = np.concatenate([a['start'][:, :, None], a['states'][:, :, :-1]], axis=2).astype(np.int64)
    st, ac = a['states'].astype(np.int64), a['actions'].astype(np.int64)
    starts = [set(host['starts'][host['off'][w]:host['off'][w + 1]].tolist())
              for w in range(n_worlds)]
    assert all(int(s) in starts[w] for w, row in zip(world, a['start']) for s in row)
    if not drawn:
        assert (host['next'][w3[live], prev[live], ac[live]] == st[live]).all()
    # a terminal state appears only at length - 1, and a shorter trial ends in one
    term = host['terminal'][w3[live], st[live]] != 0
    last = np.broadcast_to(k == a['length'][:, :, None] - 1, live.shape)[live]
    assert not term[~last].any()
    assert (term[last] | (np.broadcast_to(a['length'][:, :, None], live.shape)[live][last]
                          == steps)).all()
    if ag.mask_actions:
        assert np.asarray(ag.action_mask)[prev[live], ac[live]].all()
    return a


# -- golden ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_rollout_reproduces_the_reference(Z, name, monkeypatch):
    c = rc.case(name)
    env, ag, _ = _setup(c['world'], c['agent'], 1, c['eps'], base=c['inst'],
                        test_policy=c['test_policy'], mask=c['mask'], q_seed=None)
    host = env.handle._host
    assert np.array_equal(host['next'][0], Z[name + '/world/next'])
    assert np.array_equal(host['starts'], Z[name + '/world/starts'])
    assert np.array_equal(host['terminal'][0], Z[name + '/world/terminal'])
    ag.Q = Z[name + '/Q']
    ag.rollout_element_stores = c['inst'] % 2 == 1      # both store forms over the cases
    rec = _framed_rollout(monkeypatch, ag, env, c['trials'], c['steps'])
    got = _consistent(rec, env, ag)
    for k in ('start', 'states', 'actions', 'length'):
        want = Z['%s/%s' % (name, k)]
        assert got[k][0].dtype == want.dtype and got[k][0].tobytes() == want.tobytes(), (name, k)
    at, positions = 0, Z[name + '/positions']
    for t in range(c['trials']):
        traj = rec.trajectory(0, t)
        assert np.array_equal(np.asarray(traj), positions[at:at + len(traj)]), (name, t)
        at += len(traj)
    assert at == len(positions)
    assert ag.Q.tobytes() == Z[name + '/Q'].tobytes()


# -- twin --------------------------------------------------------------------------------------------------
TWINS = [
    # world, agent, N, steps, trials, epsilon, instance_base, mask, policy_test, element stores
    ('tiny', 'q', 1, 1, 1, 1.0, 0, False, True, False),
    ('tiny', 'dynaq', 65, 7, 3, 0.1, 3, False, False, False),
    ('open5', 'dynaq', 1, 50, 3, 0.1, 3, False, True, False),
    ('open5', 'q', 64, 7, 1, 0.0, 0, False, True, True),
    ('open5', 'dynaq', 65, 1, 3, 1.0, 3, False, False, False),
    ('open5', 'q', 130, 50, 3, 0.1, 3, False, True, False),
    ('walls8', 'dynaq', 64, 50, 3, 0.1, 3, True, True, False),
    ('walls8', 'q', 130, 7, 1, 1.0, 0, True, False, True),
    ('stack3', 'dynaq', 65, 7, 3, 0.1, 3, False, True, False),
    ('stack3', 'q', 65, 50, 1, 0.0, 0, False, False, True),
    ('hex', 'q', 130, 7, 3, 0.1, 3, False, True, False),
    ('hex', 'q', 65, 50, 1, 1.0, 0, False, False, True),
    ('track4', 'q', 64, 7, 3, 0.1, 3, False, True, False),
    ('slippery', 'dynaq', 65, 7, 3, 0.1, 3, False, True, False),      # drawn successors
    # striped monitors (from 4 096 instances on); workgroups of full waves (from 524 288 on)
    ('open5', 'dynaq', 4100, 7, 2, 0.1, 3, False, True, False),
    ('open5', 'q', 524289, 3, 1, 0.1, 3, False, True, False),
]


@pytest.mark.parametrize('case', TWINS, ids=['%s-%s-n%d-s%d-t%d-e%g' % c[:6] for c in TWINS])
def test_twin_of_test(case, monkeypatch):
    """Two agents and environments built alike, one runs test(), the other rollout(): afterwards
    everything a session leaves is bit-identical, and the record agrees with the world, with the
    latency traces and with the visit counts."""
    world, kind, n, steps, trials, eps, base, mask, test_policy, element = case
    env_a, ag_a, pol_a = _setup(world, kind, n, eps, base, test_policy, mask)
    env_b, ag_b, pol_b = _setup(world, kind, n, eps, base, test_policy, mask)
    # (a session in front, so that the recorded one does not start at trial 0 and counter 1)
    ag_a.test(env_a, 2, 5)
    ag_b.test(env_b, 2, 5)
    before = _state(ag_b, env_b, pol_b)
    ag_a.test(env_a, trials, steps)
    ag_b.rollout_element_stores = element
    rec = _framed_rollout(monkeypatch, ag_b, env_b, trials, steps, shift=16 if n == 65 else 0)
    want, got = _state(ag_a, env_a, pol_a), _state(ag_b, env_b, pol_b)
    assert want.keys() == got.keys()
    for k in want:
        assert fc.same_bits(want[k], got[k]), k
    assert got['Q'].tobytes() == before['Q'].tobytes()
    a = _consistent(rec, env_b, ag_b, drawn=world == 'slippery')
    assert rec.first_trial == 2 and (rec.n_envs, rec.trials, rec.steps) == (n, trials, steps)
    assert np.array_equal(a['length'] - 1, got['lat_trace'][:, 2:2 + trials])
    assert int(a['length'].sum()) == int(got['steps_done'][0] - before['steps_done'][0])
    counts = rec.visit_counts()
    assert counts.dtype == torch.int64 and counts.shape == ag_b.monitors.occupancy.shape
    assert np.array_equal(counts.cpu().numpy(), got['occupancy'] - before['occupancy'])
    # the plan is what the launch used: workgroups of `threads` lanes, one lane per instance
    plan = ag_b.rollout_plan
    threads = 64        # (cobel_tab_general_plan's rule: narrower workgroups for smaller launches)
    while threads > 8 and n < 8192 * threads:
        threads >>= 1
    assert plan == {'lds_bytes': 0, 'threads_per_workgroup': threads,
                    'instances_per_workgroup': threads, 'workgroups': -(-n // threads)}


def test_occupancy_maps_agree(monkeypatch):
    """get_occupancy_map on the trajectories and occupancy_from_counts on the visit counts."""
    from cobel_amd.analysis.behavior_spatial import get_occupancy_map, occupancy_from_counts
    from cobel_amd.monitor import TrajectoryMonitor
    env, ag, _ = _setup('open5', 'dynaq', 65, 0.3)
    rec = _framed_rollout(monkeypatch, ag, env, 3, 12)
    mon = TrajectoryMonitor(3, env)
    mon.update_from_device(rec)
    assert len(mon.get_trace()) == 65 * 3
    lengths = rec.length.cpu().numpy().reshape(-1)
    assert [len(t) for t in mon.get_trace()] == lengths.tolist()
    world = env.worlds[0]
    from_lists = get_occupancy_map(mon.get_trace(), 5.0, 5.0, 1.0)
    from_counts = occupancy_from_counts(rec.visit_counts()[0], world['coordinates'], 5.0, 5.0, 1.0)
    assert from_lists.sum() == lengths.sum() and np.array_equal(from_lists, from_counts)


# -- restatement -------------------------------------------------------------------------------------------
def test_per_instance_restatement(monkeypatch):
    """130 instances on the stack of three worlds against one NumPy session each, with the global
    instance id in the Philox key."""
    n, trials, steps, eps, base = 130, 3, 7, 0.1, 3
    env, ag, _ = _setup('stack3', 'dynaq', n, eps, base)
    q = ag.Q.cpu().numpy()
    rec = _framed_rollout(monkeypatch, ag, env, trials, steps)
    got = _arrays(rec)
    host = env.handle._host
    for i in range(n):
        w = (base + i) % 3
        tabs = dict(next=host['next'][w], reward=host['reward'][w], terminal=host['terminal'][w],
                    starts=host['starts'][host['off'][w]:host['off'][w + 1]])
        want = rc.restate(tabs, q[i], base + i, eps, trials, steps, True)[0]
        for k in want:
            assert got[k][i].tobytes() == want[k].tobytes(), (i, k)


# -- sessions compose --------------------------------------------------------------------------------------
def test_two_sessions_equal_one(monkeypatch):
    env_a, ag_a, pol_a = _setup('walls8', 'dynaq', 65, 0.1, 3, mask=True)
    env_b, ag_b, pol_b = _setup('walls8', 'dynaq', 65, 0.1, 3, mask=True)
    whole = _arrays(_framed_rollout(monkeypatch, ag_a, env_a, 4, 9))
    first = _arrays(_framed_rollout(monkeypatch, ag_b, env_b, 2, 9))
    second = _arrays(_framed_rollout(monkeypatch, ag_b, env_b, 2, 9))
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]], axis=1)), k
    want, got = _state(ag_a, env_a, pol_a), _state(ag_b, env_b, pol_b)
    for k in want:
        assert fc.same_bits(want[k], got[k]), k


@pytest.mark.parametrize('kind', ['dynaq', 'q'])
def test_rollout_between_training_sessions(kind, monkeypatch):
    """train(), rollout(), train() leaves the tables train(), test(), train() leaves."""
    def run(record):
        env, ag, pol = _setup('open5', kind, 65, 0.1, 3, test_policy=False, q_seed=None)
        ag.train(env, 3, 20, 8)
        if record:
            _framed_rollout(monkeypatch, ag, env, 2, 20)
        else:
            ag.test(env, 2, 20)
        ag.train(env, 3, 20, 8)
        torch.cuda.synchronize()
        out = _state(ag, env, pol)
        if kind == 'dynaq':
            out['model'] = ag.M.table.cpu().numpy()
        return out
    want, got = run(False), run(True)
    assert np.count_nonzero(want['Q']) > 0
    for k in want:
        assert fc.same_bits(want[k], got[k]), k


# -- callbacks, refusals on the device ---------------------------------------------------------------------
def test_trial_callbacks_fire_as_in_a_vectorised_session(monkeypatch):
    seen = {}
    env_a, ag_a, _ = _setup('open5', 'q', 65, 0.1)
    env_b, ag_b, _ = _setup('open5', 'q', 65, 0.1)
    for ag, key in ((ag_a, 'test'), (ag_b, 'rollout')):
        seen[key] = {'begin': [], 'end': []}
        ag.callbacks.custom_callbacks = {
            'on_trial_begin': [lambda logs, s=seen[key]: s['begin'].append(
                (logs['trial'], logs['trial_session']))],
            'on_trial_end': [lambda logs, s=seen[key]: s['end'].append(
                (logs['trial'], logs['trial_session'], logs['steps'], logs['trial_reward'],
                 logs['count']))]}
    ag_a.test(env_a, 3, 12)
    _framed_rollout(monkeypatch, ag_b, env_b, 3, 12)
    assert seen['test'] == seen['rollout'] and len(seen['rollout']['end']) == 3


def test_refusals_with_a_real_handle_and_the_handle_mirror():
    """The mirror tests/rollout_common.py keeps of the world handle's head reads a real handle; a
    misaligned table is refused before the launch; trials and steps below one raise."""
    from cobel_amd import _lib
    env, ag, _ = _setup('hex', 'q', 8, 0.1)
    head = rc.FakeWorld.from_address(env.handle.ptr.value)
    assert (head.n_states, head.n_worlds, head.n_actions) == (ag.n_states, 1, 6)
    for trials, steps in ((0, 5), (2, 0)):
        with pytest.raises(IndexError):
            ag.rollout(env, trials, steps)
    assert ag.current_trial == 0
    env4, ag4, _ = _setup('open5', 'dynaq', 8, 0.1)
    whole = torch.zeros(8 * 25 * 4 + 4, dtype=torch.float32, device='cuda')
    ag4._q = whole[1:1 + 8 * 25 * 4].view(8, 25, 4)        # 4 bytes off a 16-byte boundary
    with pytest.raises(AssertionError, match='q is misaligned'):
        ag4.rollout(env4, 1, 5)
    # the plan entry point answers for the same struct without a launch
    out = (C.c_int32 * 4)()
    ag.rollout(env, 1, 5)
    assert ag.rollout_plan['workgroups'] == 1 and ag.rollout_plan['threads_per_workgroup'] == 8
    assert _lib.lib().cobel_tab_rollout_plan(env.handle.ptr, None, out) == _lib.E_ARG
