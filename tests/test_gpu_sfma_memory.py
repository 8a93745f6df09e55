"""GPU tests of SFMAMemory's own methods (csrc/sfma_mem.hip through cobel_amd.memory.SFMAMemory):
store / replay / retrieve_random_batch against the reference's recorded scripts
(tests/golden/sfma_memory_traces.npz) and against the NumPy restatement on seeded store lists, in
every launch form; replay_batch against restatements positioned at each replay's place on the
memory stream; memory calls between training sessions.

Bar as in test_gpu_sfma.py: events, lengths, C, T, I, model tables and counters bit-equal."""
import numpy as np
import pytest

import sfma_memory_common as mc
import test_gpu_sfma as ts
from conftest import SEED
from oracle.philox import STREAM_MEMORY, TapeRNG

pytestmark = pytest.mark.gpu

CASES = ('w55_dr_error_local', 'w67_sr_error_mod')


@pytest.fixture(scope='module')
def Z(golden):
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return golden('sfma_memory_traces')


def device_memory(D, S, n, base, flags=0, **switches):
    from cobel_amd.memory import SFMAMemory
    mem = SFMAMemory(D, S, 4)
    for k, v in switches.items():
        setattr(mem, k, v)
    mem.launch_flags = flags
    mem.bind(n, seed=SEED, instance_base=base)
    return mem


def oracle_memory(D, S, g, start=0, **switches):
    mem = mc.RefMemory(D, S, 4, TapeRNG(SEED, g, STREAM_MEMORY, start=start, double_sub=1),
                       dtype=np.float32)
    for k, v in switches.items():
        setattr(mem, k, v)
    return mem


def counter_of(mem, i):
    return int(mem.counter[i].item())


# ---------------------------------------------------------------------------------------------
# 1. the reference's recorded scripts through the host methods
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,pick', [(1, None), (3, 1)], ids=['single', 'instance_1_of_3'])
@pytest.mark.parametrize('name', CASES)
def test_recorded_scripts_through_the_host_methods(Z, name, n, pick):
    g = lambda k: Z['%s/%s' % (name, k)]          # noqa: E731
    inst, S = [int(x) for x in g('cfg')]
    mem = device_memory(g('D'), S, n, inst - (pick or 0))
    got = mc.run_script(mc.DictMemory(mem, pick, index=lambda m: counter_of(m, pick or 0)),
                        mc.loads(g('ops')))
    mc.assert_same_record(got, {k: g(k) for k in mc.RECORD_KEYS}, what=name)


# ---------------------------------------------------------------------------------------------
# 2. seeded store lists against the restatement, in every launch form
# ---------------------------------------------------------------------------------------------
def _metric(h, w):
    from cobel_amd.memory.utils import Euclidean
    return Euclidean(w, h).D


def _stores(S, n, count, seed):
    """[count][n] experiences: random (s, a), a successor near s, float32 rewards, given td."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, S, (count, n))
    s[1::7] = s[0]                                   # repeats of one (s, a)
    a = rng.integers(0, 4, (count, n))
    a[1::7] = a[0]
    ns = np.clip(s + rng.integers(-3, 4, (count, n)), 0, S - 1)
    r = rng.integers(-4, 9, (count, n)) / 8.0
    nt = (rng.random((count, n)) < 0.9).astype(np.int64)
    td = np.round(rng.normal(size=(count, n)), 3)
    return s, a, r, ns, nt, td


FORMS = [
    # id, h, w, launch flags, debug LDS room, expected (form, threads, streaming tier)
    ('s25_two_per_lane', 5, 5, 0, None, (0, 64, 0)),
    ('s42', 6, 7, 0, None, (0, 64, 0)),
    ('s225_four_waves', 15, 15, 0, None, (0, 256, 0)),
    ('s225_one_wave', 15, 15, 'NO_PREFETCH', None, (0, 64, 0)),
    ('s42_streaming', 6, 7, 'STREAM', None, (1, 256, 3)),
    ('s600_streaming_16_waves', 20, 30, 'STREAM', None, (1, 1024, 3)),
    ('s1505_rows_in_lds', 35, 43, 0, 48 * 1024, (1, 1024, 2)),
    ('s2006_rows_in_place', 34, 59, 0, 48 * 1024, (1, 1024, 0)),
]
SWITCHES = [
    dict(mode='default', decay_strength=0.95, error_mod_local=True),
    dict(mode='reverse', recency=True, reward_mod=True, reward_modulation=0.5),
    dict(mode='blend_forward', C_normalize=True, D_normalize=True, error_mod=True),
    dict(mode='interpolate', state_mod=True, reward_mod_local=True, decay_inhibition=0.8),
    dict(mode='sweeping', deterministic=True, R_normalize=False),
    dict(mode='forward', beta=5.0),
    dict(mode='blend_reverse', recency=True, decay_strength=0.97),
    dict(mode='sweeping', D_normalize=True, error_mod=True),
]


@pytest.mark.parametrize('form,sw', list(zip(FORMS, SWITCHES)), ids=[f[0] for f in FORMS])
def test_store_and_replay_vs_oracle_in_every_form(form, sw, monkeypatch):
    from cobel_amd import _lib
    _, h, w, flag, room, plan = form
    if room:
        monkeypatch.setenv('COBEL_DEBUG', '1')
        monkeypatch.setenv('COBEL_DEBUG_SFMA_STREAM_LDS', str(room))
    flags = {0: 0, 'NO_PREFETCH': _lib.F_NO_PREFETCH, 'STREAM': _lib.F_SFMA_STREAM}[flag]
    S, n, base, count = h * w, 2, 40, 90
    D = _metric(h, w)
    mem = device_memory(D, S, n, base, flags, **sw)
    p = mem.launch_plan()
    assert (p[0], p[2], p[3]) == plan
    refs = [oracle_memory(D, S, base + i, **sw) for i in range(n)]
    s, a, r, ns, nt, td = _stores(S, n, count, seed=S)
    L, seen = 12, []

    def compare(what):
        for i, ref in enumerate(refs):
            assert np.array_equal(mem.C[i], ref.C), (what, i)
            assert np.array_equal(mem.T[i], ref.T), (what, i)
            assert np.array_equal(mem.I[i], ref.I), (what, i)
            assert counter_of(mem, i) == ref.rng.index, (what, i)

    def replays(state, action):
        got = mem.replay(L, state, action)
        for i, ref in enumerate(refs):
            st = None if state is None else int(np.broadcast_to(state, (n,))[i])
            ac = None if action is None else int(np.broadcast_to(action, (n,))[i])
            want = ref.replay(L, st, ac)
            rows = mc.DictMemory._rows(got[i])
            assert rows == [[float(x) for x in e] for e in want], (state, action, i)
            seen.append(len(rows))
        compare((state, action))

    for k in range(count):
        mem.store({'state': s[k], 'action': a[k], 'reward': r[k], 'next_state': ns[k],
                   'terminal': nt[k], 'td': td[k]})
        for i, ref in enumerate(refs):
            ref.store(int(s[k, i]), int(a[k, i]), float(r[k, i]), int(ns[k, i]), int(nt[k, i]),
                      float(td[k, i]))
        if k == count // 2:
            replays(s[k], None)
    compare('stores')
    for i, ref in enumerate(refs):
        assert np.array_equal(mem.rewards[i], ref.rewards) and np.array_equal(mem.states[i], ref.states)
        assert np.array_equal(mem.terminals[i], ref.terminals)
    replays(int(s[0, 0]), None)
    replays(None, None)
    replays(s[3], a[3])
    replays(None, 2)
    assert sum(seen) > 5 * L and max(seen) == L


# ---------------------------------------------------------------------------------------------
# 3. memory calls between training sessions (one world with drawn successors)
# ---------------------------------------------------------------------------------------------
def _ref_agent(ow, D, g, opts):
    from oracle import sfma_loop
    from oracle.philox import STREAM_AGENT, STREAM_ENV, STREAM_POLICY
    env = sfma_loop.RefGridworld(ow, TapeRNG(SEED, g, STREAM_ENV, double_sub=1))
    mem = oracle_memory(D, env.n_states, g)
    pol = sfma_loop.RefEpsilonGreedy(0.1, TapeRNG(SEED, g, STREAM_POLICY))
    ag = sfma_loop.RefSFMA(env.n_states, 4, pol, mem, None, rng=TapeRNG(SEED, g, STREAM_AGENT),
                           dtype=np.float32)
    mem.mode = opts['mode']
    for k in ts.MEM_KEYS:
        if k in opts:
            setattr(mem, k, opts[k])
    return ag, env


@pytest.mark.parametrize('slip', [False, True], ids=['table_world', 'drawn_successors'])
def test_memory_calls_between_training_sessions(slip):
    from conftest import as_world
    from cobel_amd.memory.utils import DR
    h, w, n, base, steps, B = 7, 7, 4, 200, 40, 16
    walls = [(w + 1, w + 2), (w + 2, w + 1)]
    world = ts._field(h, w, w - 1, 1.0, walls)
    D = DR(w, h, world['next'], 0.9, world['invalid_transitions']).D
    tab = dict(world.compact(), height=h, width=w, coordinates=world['coordinates'])
    ow = ts._oracle_world(world)
    # (no recency here: train() ends with T.fill(0), after which a recency replay is empty)
    opts = {'mode': 'reverse', 'decay_strength': 0.97}
    if slip:
        sas = np.array(world['sas'])
        sas = 0.8 * sas + 0.1 * sas[:, [1, 2, 3, 0]] + 0.1 * sas[:, [3, 0, 1, 2]]
        made = as_world(tab)
        made['sas'] = sas
        made['deterministic'] = False
        env, agent = ts.build(made, D, opts, n, base, made=True)
        ow = dict(ow, sas=sas)
    else:
        env, agent = ts.build(tab, D, opts, n, base)
    e = {'state': 10, 'action': 2, 'reward': 0.5, 'next_state': 11, 'terminal': 1}
    agent.train(env, 4, steps, B)
    mid = agent.M.replay(16, 10)
    agent.M.store(e)
    drawn = agent.M.replay(16)
    agent.train(env, 4, steps, B)
    for i in (0, 3):
        ag, oenv = _ref_agent(ow, D, base + i, opts)
        ag.train(oenv, 4, steps, B)
        want_mid = ag.M.replay(16, 10)
        ag.M.store(10, 2, 0.5, 11, 1)
        want_drawn = ag.M.replay(16)
        ag.train(oenv, 4, steps, B)
        for got, want in ((mid[i], want_mid), (drawn[i], want_drawn)):
            assert len(want) > 0
            assert mc.DictMemory._rows(got) == [[float(x) for x in r] for r in want], i
        rp = np.array(ag.replayed, dtype=np.float64).reshape(-1, 8)
        ts.check_events(ts.events_of(agent, i), rp)
        assert np.array_equal(agent.Q[i].cpu().numpy(), ag.Q), i
        assert np.array_equal(agent.M.C[i], ag.M.C) and np.array_equal(agent.M.T[i], ag.M.T), i
        assert counter_of(agent.M, i) == ag.M.rng.index, i
        assert int(env.env_ctr[i].item()) == oenv.rng.index, i
    with pytest.raises(NotImplementedError, match='M.replay'):
        agent.replay(16, 10)


# ---------------------------------------------------------------------------------------------
# 4. replay_batch
# ---------------------------------------------------------------------------------------------
def test_replay_batch_vs_oracle_copies_on_their_strides():
    import copy
    import torch
    h, w, n, base, K, L = 6, 7, 3, 70, 5, 12
    S = h * w
    D = _metric(h, w)
    sw = dict(mode='blend_reverse', decay_strength=0.95)
    mem = device_memory(D, S, n, base, **sw)
    refs = [oracle_memory(D, S, base + i, **sw) for i in range(n)]
    s, a, r, ns, nt, td = _stores(S, n, 80, seed=5)
    for k in range(80):
        mem.store({'state': s[k], 'action': a[k], 'reward': r[k], 'next_state': ns[k],
                   'terminal': nt[k]})
        for i, ref in enumerate(refs):
            ref.store(int(s[k, i]), int(a[k, i]), float(r[k, i]), int(ns[k, i]), int(nt[k, i]))
    mem.replay(4)                                  # the stream does not start at 0
    for ref in refs:
        ref.replay(4)
    for state in (None, np.array([3, 17, 40])):
        before = [t.clone() for t in (mem.strength, mem.stamp, mem.table, mem.state)]
        c0 = [counter_of(mem, i) for i in range(n)]
        single = mem.counter.clone()
        out = mem.replay_batch(K, L, state)
        for x, y in zip(before, (mem.strength, mem.stamp, mem.table, mem.state)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert out['state'].shape == (n, K, L) and out['length'].shape == (n, K)
        for i, ref in enumerate(refs):
            assert counter_of(mem, i) == c0[i] + K * (L + 2) == c0[i] + 70
            for k in range(K):
                cp = copy.deepcopy(ref)
                cp.rng = TapeRNG(SEED, base + i, STREAM_MEMORY, start=c0[i] + k * (L + 2),
                                 double_sub=1)
                want = cp.replay(L, None if state is None else int(state[i]))
                m = int(out['length'][i, k])
                assert m == len(want) > 0
                got = [[float(out[key][i, k, j]) for key in
                        ('state', 'action', 'reward', 'next_state', 'terminal')] for j in range(m)]
                assert got == [[float(x) for x in e] for e in want], (i, k)
                assert (out['state'][i, k, m:] == -1).all()
                if k == 0:
                    assert np.array_equal(mem.I[i], cp.I)
            ref.rng.index = c0[i] + K * (L + 2)
        # replay 0 is a single replay() from the same state of memory and stream
        mem.counter.copy_(single)
        one = mem.replay(L, state)
        for i in range(n):
            m = int(out['length'][i, 0])
            assert [e['state'] for e in one[i]] == out['state'][i, 0, :m].tolist()
            assert [e['action'] for e in one[i]] == out['action'][i, 0, :m].tolist()
        mem.counter.copy_(torch.as_tensor([c + 70 for c in c0], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------
def test_early_end_empty_memory_and_ratings_below_threshold():
    D = _metric(5, 5)
    mem = device_memory(D, 25, 1, 3)
    assert np.array_equal(mem.I, np.zeros(25))
    with pytest.raises(ValueError):
        mem.replay(8)
    with pytest.raises(ValueError):
        mem.replay_batch(3, 8)
    assert mem.replay(8, 7) == [] and counter_of(mem, 0) == 1
    for a, ns in ((0, 6), (1, 2), (2, 8), (3, 12), (0, 6)):
        mem.store({'state': 7, 'action': a, 'reward': 0.0, 'next_state': ns, 'terminal': 1})
    for start in (7, None):
        out = mem.replay(8, start)
        assert len(out) == 1 and out[0]['state'] == 7
        assert mem.I[7] == 1.0 and np.count_nonzero(mem.I) == 1
    weak = device_memory(D, 25, 1, 0, C_step=1e-9)
    weak.store({'state': 3, 'action': 1, 'reward': 0.0, 'next_state': 4, 'terminal': 1})
    assert weak.replay(4, 3) == []
    with pytest.raises(IndexError):
        weak.store({'state': 25, 'action': 1, 'reward': 0.0, 'next_state': 4, 'terminal': 1})
    with pytest.raises(IndexError):
        weak.replay(4, 3, 4)
    werr = device_memory(D, 25, 1, 0, error_mod=True)
    with pytest.raises(KeyError):
        werr.store({'state': 3, 'action': 1, 'reward': 0.0, 'next_state': 4, 'terminal': 1})
