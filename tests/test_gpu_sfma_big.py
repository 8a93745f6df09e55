"""GPU tests of the streaming form of the SFMA kernel (csrc/sfma_big.hip): worlds of 1 275 ...
16 383 states, whose tables do not fit the LDS, and any world under ``force_stream_kernel``.

Bar as in test_gpu_sfma.py: replayed experiences, Q, strengths, model and recency bit-exact —
against the reference's recorded runs (tests/golden/sfma_traces.npz) on the small worlds, against
the LDS-resident form where both forms run, and against the NumPy restatement
(oracle/sfma_loop.py) beyond the LDS.  No instance is skipped or tolerated."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_sfma as ts
from conftest import SEED
from sfma_common import sfma_case

pytestmark = pytest.mark.gpu

Z = ts.Z
RP_KEYS = ('rp_trial', 'rp_kind', 'rp_state', 'rp_action', 'rp_reward', 'rp_next',
           'rp_nonterminal', 'rp_td')
FIXED = 512 + 384 + 128     # cross-wave scratch, epsilon-greedy thresholds, constants


def _plan(n_states, flags=0):
    from cobel_amd import _lib
    out = (C.c_int32 * 4)()
    _lib.check(_lib.lib().cobel_sfma_plan(n_states, flags, C.byref(out)))
    return list(out)


def _align16(n):
    return (n + 15) & ~15


@functools.lru_cache(maxsize=None)
def _world(h, w):
    walls = [(w + 1, w + 2), (w + 2, w + 1), (2 * w + 1, 2 * w + 2), (2 * w + 2, 2 * w + 1)]
    world = ts._field(h, w, w - 1, 1.0, walls)
    tab = dict(world.compact(), height=h, width=w, coordinates=world['coordinates'])
    return world, tab, ts._oracle_world(world)


@functools.lru_cache(maxsize=None)
def _metric(kind, h, w):
    from cobel_amd.memory.utils import DR, SR, Euclidean
    world = _world(h, w)[0]
    if kind == 'DR':
        return DR(w, h, world['next'], 0.9, world['invalid_transitions']).D
    if kind == 'SR':
        return SR(world['next'], 0.9).D
    return Euclidean(w, h).D


def _against_oracle(agent, env, ow, D, opts, base, picks, trials, steps, B, n_trials=None):
    """The comparison list of test_sfma_vs_oracle_larger_worlds for the instances `picks`."""
    from oracle import sfma_loop
    for i in picks:
        ag, oenv = sfma_loop.run_case(ow, D, SEED, base + i, True, opts['mode'], opts, trials,
                                      steps, B)
        n = n_trials or trials
        assert np.array_equal(agent.monitors.lat_trace[i].cpu().numpy()[:n], ag.steps), i
        rp = np.array(ag.replayed, dtype=np.float64).reshape(-1, 8)
        ts.check_events(ts.events_of(agent, i), rp)
        assert np.array_equal(agent.Q[i].cpu().numpy(), ag.Q), i
        assert np.array_equal(agent.M.rewards[i], ag.M.rewards), i
        assert np.array_equal(agent.M.states[i], ag.M.states), i
        assert np.array_equal(agent.M.C[i], ag.M.C), i
        assert np.array_equal(agent.M.T[i], ag.M.T), i
        assert agent.td[i] == float(ag.td), i
        assert int(env.env_ctr[i].item()) == oenv.rng.index, i


# ---------------------------------------------------------------------------------------------
# 1. the reference's recorded runs through the streaming form (fewer experiences than threads)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ts.F32_CASES)
def test_stream_form_reproduces_reference_goldens(Z, name):
    g, world, D, opts = sfma_case(Z, name)
    inst, f32, trials, steps, B = [int(x) for x in g('cfg')]
    env, agent = ts.build(world, D, opts, 2, inst)
    agent.force_stream_kernel = True
    ts.run_schedule(env, agent, opts, trials, steps, B)
    assert list(agent.launch_plan)[0] == 1
    rp = np.stack([g(k).astype(np.float64) for k in RP_KEYS], axis=1)
    ts.check_events(ts.events_of(agent, 0), rp)
    assert np.array_equal(agent.Q[0].cpu().numpy().astype(np.float64), g('Q'))
    assert np.array_equal(agent.M.C[0], g('C'))
    n_trials = len(g('steps'))
    assert np.array_equal(agent.monitors.lat_trace[0].cpu().numpy()[:n_trials], g('steps'))


# ---------------------------------------------------------------------------------------------
# 2. streaming form = LDS form (256 threads at 15 x 15, 1 024 at 23 x 23)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', [15, 23])
@pytest.mark.parametrize('opts', [
    {'mode': 'blend_reverse', 'recency': True},
    {'mode': 'sweeping', 'dynamic': True, 'start_replay': True},
], ids=['blend_reverse_recency', 'sweeping_dynamic_start'])
def test_stream_form_equals_lds_form(side, opts):
    import torch
    tab = _world(side, side)[1]
    D = _metric('DR', side, side)
    assert _plan(side * side, 4096)[2] == (256 if side == 15 else 1024)
    runs = []
    for stream in (False, True):
        env, agent = ts.build(tab, D, opts, 24, 300)
        agent.force_stream_kernel = stream
        agent.train(env, 4, 60, 20)
        torch.cuda.synchronize()
        assert list(agent.launch_plan)[0] == int(stream)
        runs.append(agent)
    a, b = runs
    assert torch.equal(a._q, b._q) and torch.equal(a.M.strength, b.M.strength)
    assert torch.equal(a.M.table, b.M.table) and torch.equal(a.M.stamp, b.M.stamp)
    assert torch.equal(a.inst, b.inst) and torch.equal(a.M.state, b.M.state)
    for i in (0, 23):
        ea, eb = ts.events_of(a, i), ts.events_of(b, i)
        # (bytes: the TD error of a trial-start reactivation is NaN)
        assert len(ea) > 50 and ea.tobytes() == eb.tobytes()


# ---------------------------------------------------------------------------------------------
# 3. beyond the LDS against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [
    # the first square world the LDS form refuses (NotImplementedError before the streaming form)
    dict(h=36, w=36, metric='DR', mode='default', steps=80, B=16, opts={}),
    dict(h=35, w=37, metric='Euclidean', mode='interpolate', steps=70, B=12,
         opts={'C_normalize': True, 'reward_mod': True, 'decay_strength': 0.97}),
    # 1 275 states, the first refused size
    dict(h=25, w=51, metric='SR', mode='reverse', steps=70, B=14,
         opts={'recency': True, 'D_normalize': True}),
    # per-state vectors and the successor table still fit the LDS
    dict(h=64, w=64, metric='Euclidean', mode='default', steps=120, B=12, opts={'random': True},
         n=8, picks=(0, 7)),
], ids=['36x36_dr', '35x37_eu_interp_mods', '25x51_sr_reverse_recency', '64x64_eu_random'])
def test_stream_form_vs_oracle_beyond_the_lds(cfg):
    h, w = cfg['h'], cfg['w']
    world, tab, ow = _world(h, w)
    D = _metric(cfg['metric'], h, w)
    opts = dict(cfg['opts'], mode=cfg['mode'])
    n = cfg.get('n', 16)
    env, agent = ts.build(tab, D, opts, n, 1000)
    trials = 3
    ts.run_schedule(env, agent, opts, trials, cfg['steps'], cfg['B'])
    assert list(agent.launch_plan)[:3] == [1, 32 * h * w + FIXED, 1024]
    _against_oracle(agent, env, ow, D, opts, 1000, cfg.get('picks', (0, 5, 10, 15)), trials,
                    cfg['steps'], cfg['B'])


@pytest.mark.parametrize('cfg', [
    # the scan itself where a thread owns 16 experiences (`random` above replays uniform batches)
    dict(h=64, w=64, mode='blend_reverse', per_state=32, opts={'recency': True}),
    # the smallest size of each further tier of the plan, as a production launch
    dict(h=7, w=727, mode='reverse', per_state=24, opts={}),                        # 5 089 states
    dict(h=59, w=115, mode='sweeping', per_state=8, opts={'D_normalize': True}),    # 6 785 states
], ids=['64x64_blend_reverse_recency', 'records_5089_reverse', 'rows_in_place_6785_sweeping'])
def test_stream_form_at_the_tier_boundaries_vs_oracle(cfg):
    h, w = cfg['h'], cfg['w']
    S = h * w
    if cfg['per_state'] < 32:
        assert _plan(S - 1)[1] > _plan(S)[1]           # the smallest size of its tier
    assert _plan(S)[:3] == [1, _align16(cfg['per_state'] * S) + FIXED, 1024]
    world, tab, ow = _world(h, w)
    D = _metric('Euclidean', h, w)
    opts = dict(cfg['opts'], mode=cfg['mode'])
    env, agent = ts.build(tab, D, opts, 4, 1000)
    ts.run_schedule(env, agent, opts, 3, 80, 12)
    assert list(agent.launch_plan)[:3] == _plan(S)[:3]
    _against_oracle(agent, env, ow, D, opts, 1000, (3,), 3, 80, 12)


@pytest.mark.parametrize('cfg', [
    # extras: the same tiers on small worlds, reached by lowering the LDS the streaming form may
    # take to 48 KiB: 32 B per state up to 1 504 states, 24 B up to 2 005, 8 B beyond
    dict(h=35, w=43, mode='blend_reverse', per_state=24, opts={}),                 # 1 505 states
    dict(h=34, w=59, mode='sweeping', per_state=8, opts={'D_normalize': True}),    # 2 006 states
    dict(h=34, w=59, mode='forward', per_state=8, opts={'recency': True}),
], ids=['rows_in_lds_1505', 'rows_in_place_2006_sweeping', 'rows_in_place_2006_forward'])
def test_stream_form_tiers_vs_oracle(cfg, monkeypatch):
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_SFMA_STREAM_LDS', str(48 * 1024))
    h, w = cfg['h'], cfg['w']
    S = h * w
    assert _plan(S - 1)[1] > _plan(S)[1]           # the smallest size of its tier
    assert _plan(S)[:3] == [1, _align16(cfg['per_state'] * S) + FIXED, 1024]
    world, tab, ow = _world(h, w)
    D = _metric('Euclidean', h, w)
    opts = dict(cfg['opts'], mode=cfg['mode'])
    env, agent = ts.build(tab, D, opts, 4, 1000)
    ts.run_schedule(env, agent, opts, 3, 80, 12)
    _against_oracle(agent, env, ow, D, opts, 1000, (3,), 3, 80, 12)


def test_stream_form_on_drawn_successors():
    """36 x 36 with slip 0.2: the successor of every step is drawn (cobel_world_set_transitions)."""
    world, tab, ow = _world(36, 36)
    D = _metric('DR', 36, 36)
    sas = np.array(world['sas'])
    slip = 0.8 * sas + 0.1 * sas[:, [1, 2, 3, 0]] + 0.1 * sas[:, [3, 0, 1, 2]]
    from conftest import as_world
    made = as_world(tab)
    made['sas'] = slip
    made['deterministic'] = False
    opts = {'mode': 'reverse'}
    env, agent = ts.build(made, D, opts, 16, 500, made=True)
    assert env.handle.stochastic
    ts.run_schedule(env, agent, opts, 3, 80, 16)
    assert list(agent.launch_plan)[0] == 1
    _against_oracle(agent, env, dict(ow, sas=slip), D, opts, 500, (0, 6, 11, 15), 3, 80, 16)


def test_stream_form_with_an_action_mask():
    world, tab, ow = _world(36, 36)
    D = _metric('DR', 36, 36)
    mask = np.ones((36 * 36, 4), dtype=bool)
    mask[::3, 2] = False
    mask[1::5, 0] = False
    opts = {'mode': 'blend_forward', 'mask': mask}
    env, agent = ts.build(tab, D, opts, 16, 700)
    ts.run_schedule(env, agent, opts, 3, 80, 16)
    _against_oracle(agent, env, ow, D, opts, 700, (0, 5, 9, 15), 3, 80, 16)


# ---------------------------------------------------------------------------------------------
# 4. plan and boundary
# ---------------------------------------------------------------------------------------------
def test_plan_and_boundaries(Z):
    from cobel_amd import _lib
    lib = _lib.lib()
    STREAM = _lib.F_SFMA_STREAM
    assert STREAM == 4096
    assert _plan(1274) == [0, 128 * 1274 + 768, 256, 0]
    assert _plan(25) == [0, _align16(128 * 25) + 768, 64, 0]
    assert _plan(1275) == [1, _align16(32 * 1275) + FIXED, 1024, 0]
    assert _plan(1274, STREAM)[0] == 1 and _plan(25, STREAM)[:3] == [1, 32 * 25 + FIXED, 256]
    # what the plan keeps in LDS, by room: 160 KiB less the fixed part
    assert _plan(5088)[1] == 32 * 5088 + FIXED and _plan(5089)[1] == _align16(24 * 5089) + FIXED
    assert _plan(6784)[1] == 24 * 6784 + FIXED and _plan(6785)[1] == _align16(8 * 6785) + FIXED
    assert _plan(16383) == [1, _align16(8 * 16383) + FIXED, 1024, 0]
    assert max(_plan(s)[1] for s in (1275, 5088, 6784, 16383)) <= 160 * 1024
    out = (C.c_int32 * 4)()
    assert lib.cobel_sfma_plan(16384, 0, C.byref(out)) == _lib.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='15-bit'):
        _lib.check(lib.cobel_sfma_plan(16384, 0, C.byref(out)))
    assert lib.cobel_sfma_plan(0, 0, C.byref(out)) == _lib.E_RANGE
    with pytest.raises(IndexError):
        _lib.check(lib.cobel_sfma_plan(0, STREAM, C.byref(out)))
    lds = C.c_int32()
    with pytest.raises(NotImplementedError):                 # the resident form keeps its answer
        _lib.check(lib.cobel_sfma_query(1600, C.byref(lds)))
    assert lib.cobel_sfma_query(1274, C.byref(lds)) == 0 and lds.value == 160 * 1024

    # n = 0 on a world of the streaming form: OK without a launch
    import torch
    tab = _world(36, 36)[1]
    env, agent = ts.build(tab, _metric('DR', 36, 36), {'mode': 'default'}, 2, 0)
    agent.train(env, 0, 10, 8)
    z = torch.zeros(64, dtype=torch.int64, device='cuda')
    run = _lib.SFMARun()
    for f in ('q', 'model', 'strength', 'stamp', 'inst', 'sfma_inst', 'metric'):
        setattr(run, f, _lib.ptr(z))
    run.n, run.steps_per_trial, run.epsilon, run.batch, run.nb_replays = 0, 5, 0.1, 4, 1
    _lib.check(lib.cobel_sfma_run(env.handle.ptr, C.byref(run), None))
    torch.cuda.synchronize()
    assert int(z.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------
# 5. cuts and shards, 6. Agent.test
# ---------------------------------------------------------------------------------------------
def test_stream_form_cuts_and_shards_at_36x36():
    tab = _world(36, 36)[1]
    D = _metric('DR', 36, 36)
    opts = {'mode': 'reverse', 'recency': True}
    steps, B = 60, 16

    def tables(agents):
        return [np.concatenate([f(a) for a in agents]) for f in (
            lambda a: a.Q.cpu().numpy(), lambda a: a.M.C, lambda a: a.M.table.cpu().numpy(),
            lambda a: a.M.stamp.cpu().numpy(), lambda a: a.M.state.cpu().numpy())]

    env, ref = ts.build(tab, D, opts, 16, 1000)
    ref.train(env, 6, steps, B)
    env2, cut = ts.build(tab, D, opts, 16, 1000)
    cut.train(env2, 2, steps, B)
    cut.train(env2, 4, steps, B)
    parts = []
    for base in (1000, 1008):
        e, a = ts.build(tab, D, opts, 8, base)
        a.train(e, 6, steps, B)
        parts.append(a)
    want = tables([ref])
    for got in (tables([cut]), tables(parts)):
        for x, y in zip(want, got):
            assert np.array_equal(x, y)
    first, last = ts.events_of(ref, 0), ts.events_of(ref, 15)
    assert len(first) > 50 and len(last) > 50
    assert first.tobytes() == ts.events_of(cut, 0).tobytes()
    assert last.tobytes() == ts.events_of(cut, 15).tobytes()
    assert first.tobytes() == ts.events_of(parts[0], 0).tobytes()
    assert last.tobytes() == ts.events_of(parts[1], 7).tobytes()


def test_stream_form_agent_test_at_36x36():
    """Agent.test after a short training: act only, on the test stream."""
    world, tab, ow = _world(36, 36)
    D = _metric('DR', 36, 36)
    opts = {'mode': 'default', 'test_trials': 3}
    env, agent = ts.build(tab, D, opts, 16, 1000)
    before = None
    agent.train(env, 3, 80, 16)
    before = (agent._q.clone(), agent.M.strength.clone(), agent.M.table.clone())
    agent.test(env, 3, 80)
    import torch
    assert torch.equal(before[0], agent._q) and torch.equal(before[1], agent.M.strength)
    assert torch.equal(before[2], agent.M.table)
    _against_oracle(agent, env, ow, D, opts, 1000, (0, 4, 11, 15), 3, 80, 16, n_trials=6)
