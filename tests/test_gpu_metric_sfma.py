"""SFMA on a device metric (``SR`` / ``DR`` with ``compute='device'``): the memory launches on the
metric's own tensor, and a run equals — Q, model, strengths, stamps, latencies, bit for bit — the
same run handed a host copy of the same matrix; so does the detour sequence (train, close a
passage, ``metric.update_transitions()``, train).  No run is compared with one on the LAPACK
matrix: the two matrices differ in their last bits, and a replay draw may differ with them."""
import numpy as np
import pytest

from conftest import SEED
from frames_common import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'


def field(h, w, goal, walls=()):
    from cobel_amd.misc.gridworld_tools import make_gridworld
    inv = [p for a, b in walls for p in ((a, b), (b, a))]
    return make_gridworld(h, w, terminals=[goal], rewards=np.array([[goal, 1.0]]), goals=[goal],
                          invalid_transitions=inv)


def agent_on(worlds, metric, n_envs, mode):
    from cobel_amd.agent import SFMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(worlds, n_envs=n_envs, seed=SEED, instance_base=3)
    mem = SFMAMemory(metric, env.observation_space.n, 4)
    agent = SFMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    agent.M.mode = mode
    agent.track_instances = True
    return env, agent


def tables(agent):
    import torch
    torch.cuda.synchronize()
    return {'Q': agent._q.clone(), 'model': agent.M.table.clone(),
            'strength': agent.M.strength.clone(), 'stamp': agent.M.stamp.clone(),
            'latencies': agent.monitors.lat_trace.clone()}


def assert_equal_runs(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert same_bits(a[key], b[key]), key
    assert float(a['strength'].sum()) > 0 and float(a['Q'].abs().sum()) > 0


def test_the_memory_launches_on_the_metrics_own_tensor():
    from cobel_amd.memory.utils import DR, SR
    world = field(7, 7, 6, [(8, 9)])
    m = DR(7, 7, world['next'], 0.9, world['invalid_transitions'], compute='device')
    env, agent = agent_on(world, m, 4, 'reverse')
    assert agent.M._metric_on(env.device, 1).data_ptr() == m.D.data_ptr()
    agent.train(env, 2, 20, 8)
    assert agent.M._metric_on(env.device, 1).data_ptr() == m.D.data_ptr()
    assert agent.M._metric_dev is None
    # a stack is used where it lies; one matrix for two worlds is expanded, and again after an update
    wa, wb = field(6, 6, 5, [(7, 8)]), field(6, 6, 30, [(13, 19)])
    stack = SR([wa['next'], wb['next']], 0.9, compute='device')
    env, agent = agent_on([wa, wb], stack, 4, 'default')
    assert agent.M._metric_on(env.device, 2).data_ptr() == stack.D.data_ptr()
    one = SR(wa['next'], 0.9, compute='device')
    env, agent = agent_on([wa, wb], one, 4, 'default')
    exp = agent.M._metric_on(env.device, 2)
    assert tuple(exp.shape) == (2, 36, 36) and same_bits(exp[0], one.D) and same_bits(exp[1], one.D)
    assert agent.M._metric_on(env.device, 2).data_ptr() == exp.data_ptr()
    wa['next'][7, :] = 7
    one.update_transitions()
    again = agent.M._metric_on(env.device, 2)
    assert again.data_ptr() == exp.data_ptr() and same_bits(again[1], one.D)


@pytest.mark.parametrize('h,w,kind,mode,n', [(7, 7, 'DR', 'reverse', 6), (36, 36, 'SR', 'default', 3)])
def test_train_equals_the_run_on_a_host_copy(h, w, kind, mode, n):
    """7 x 7 is served by the LDS form, 36 x 36 (1 296 states) by the streaming form."""
    import ctypes as C
    from cobel_amd import _lib
    from cobel_amd.memory.utils import DR, SR
    walls = [(w + 1, w + 2), (2 * w + 1, 2 * w + 2)]
    world = field(h, w, w - 1, walls)
    out = (C.c_int32 * 4)()
    _lib.check(_lib.lib().cobel_sfma_plan(h * w, 0, C.byref(out)))
    assert out[0] == (1 if h * w > 1274 else 0)
    if kind == 'DR':
        m = DR(w, h, world['next'], 0.9, world['invalid_transitions'], compute='device')
    else:
        m = SR(world['next'], 0.9, compute='device')
    runs = []
    for metric in (m, m.D.cpu().numpy()):
        env, agent = agent_on(field(h, w, w - 1, walls), metric, n, mode)
        agent.train(env, 3, 40, 16)
        runs.append(tables(agent))
    assert_equal_runs(*runs)


def test_three_worlds_with_their_own_metrics():
    from cobel_amd.memory.utils import DR
    walls = ([(7, 8)], [(13, 19), (14, 20)], [])
    make = lambda: [field(6, 6, g, wl) for g, wl in zip((5, 30, 35), walls)]   # noqa: E731
    worlds = make()
    m = DR(6, 6, [x['next'] for x in worlds], 0.9, [x['invalid_transitions'] for x in worlds],
           compute='device')
    assert tuple(m.D.shape) == (3, 36, 36) and same_bits(m.D[2], m.D0)
    runs = []
    for metric in (m, m.D.cpu().numpy()):
        env, agent = agent_on(make(), metric, 9, 'reverse')
        agent.train(env, 4, 30, 16)
        runs.append(tables(agent))
    assert_equal_runs(*runs)


def test_the_detour_sequence():
    """train, close a passage in env.world, metric.update_transitions(), train — against the same
    sequence on host copies of the same two matrices."""
    from cobel_amd.memory.utils import DR

    def close(world):
        nxt = world['next']
        for s, t in ((24, 25), (25, 24)):
            nxt[s, np.asarray(nxt[s]) == t] = s
            world['invalid_transitions'].append((s, t))

    world = field(7, 7, 6, [(8, 9)])
    env, agent = agent_on(world, None, 5, 'reverse')
    m = DR(7, 7, env.world['next'], 0.9, env.world['invalid_transitions'], compute='device')
    agent.M.metric = m
    ptr = m.D.data_ptr()
    agent.train(env, 3, 30, 16)
    before = m.D.cpu().numpy()
    close(env.world)
    m.update_transitions()
    assert m.D.data_ptr() == ptr
    agent.train(env, 3, 30, 16)
    dev = tables(agent)
    after = m.D.cpu().numpy()
    assert not np.array_equal(before, after)
    fresh = DR(7, 7, env.world['next'], 0.9, env.world['invalid_transitions'], compute='device')
    assert same_bits(m.D, fresh.D)

    world = field(7, 7, 6, [(8, 9)])
    env, agent = agent_on(world, before, 5, 'reverse')
    agent.train(env, 3, 30, 16)
    close(env.world)
    agent.M.metric = after
    agent.train(env, 3, 30, 16)
    assert_equal_runs(dev, tables(agent))
