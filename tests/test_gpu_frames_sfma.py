"""``cobel_sfma_run`` in its kernel forms and the SFMA memory calls (``cobel_sfma_store``,
``cobel_sfma_replay``, ``cobel_sfma_random_batch``) with every array of the launch struct inside a
frame of sentinels (tests/frames_common.py): guards intact, the framed run bit-equal to the plain
run, the form told by ``cobel_sfma_plan`` / ``cobel_sfma_mem_plan``, and the edges reached — more
trials than ``trial_cap``, more replay events than ``trace_cap``, Q and the strengths changed in
the last instance and for the last state, replays done.

The launch struct is filled here as ``SFMA._launch`` fills it, from the agent's and the memory's
own attributes, because the agent sizes its replay trace itself and the cases need one that is
too small."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
from conftest import SEED

pytestmark = pytest.mark.gpu

N = 3
EVENT_BYTES = 24
SI_POISON = [0, 0, 0, 1, 0, 0, 0, fc.MARK]      # cobel_sfma_inst words: mode 'default', the last reserved


def _lib():
    from cobel_amd import _lib
    return _lib


def field(h, w):
    from cobel_amd.misc.gridworld_tools import make_gridworld
    S = h * w
    goal = S // 2
    return make_gridworld(h, w, terminals=[goal], goals=[goal], starting_states=[S - 1, 0],
                          rewards=np.array([[goal, 1.0], [S - 2, 0.25], [1, -0.5]]))


def build(h, w, opts, metric='Euclidean'):
    from cobel_amd.agent import SFMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.memory.utils import DR, Euclidean
    from cobel_amd.policy import EpsilonGreedy
    world = field(h, w)
    D = (DR(w, h, world['next'], 0.9, world['invalid_transitions']).D if metric == 'DR'
         else Euclidean(w, h).D)
    env = Gridworld(world, n_envs=N, seed=SEED, instance_base=40)
    mem = SFMAMemory(D, h * w, 4)
    agent = SFMA(env.observation_space, env.action_space, EpsilonGreedy(0.3), mem,
                 learning_rate=0.5, gamma=0.875)
    for k, v in opts.items():
        if k == 'mask':
            nxt = np.asarray(world['next'])
            m = nxt != np.arange(h * w)[:, None]
            m[~m.any(axis=1)] = True
            agent.mask_actions, agent.action_mask = True, m
        elif k == 'mode':
            mem.mode = v
        elif hasattr(mem, k) and k not in ('random',):
            setattr(mem, k, v)
        else:
            setattr(agent, k, v)
    return env, agent


def launch(ag, env, pol, flags, target, spt, budget, batch, trace, trace_len):
    """``SFMA._launch`` with the replay trace the test brings."""
    L = _lib()
    M = ag.M
    run = L.SFMARun()
    ag._fill_run(run, env, flags, target, spt, budget)
    run.q, run.model = L.ptr(ag._q), L.ptr(M.table)
    run.strength, run.stamp = L.ptr(M.strength), L.ptr(M.stamp)
    run.sfma_inst = L.ptr(M.state)
    run.metric = L.ptr(M._metric_on(ag.device, env.handle.n_worlds))
    run.sfma_flags = M._fill_params(run) | (L.SF_RANDOM if ag.random else 0) | \
        (L.SF_DYNAMIC if ag.dynamic else 0) | (L.SF_START_REPLAY if ag.start_replay else 0)
    if ag.random:
        run.random_cdf = L.ptr(ag._random_cdf())
    run.replays_done = L.ptr(ag.replays_done)
    if trace is not None:
        run.replay_trace, run.trace_len = L.ptr(trace), L.ptr(trace_len)
        run.trace_cap = trace.shape[1] // EVENT_BYTES
    run.flags = flags
    run.batch, run.nb_replays = batch, ag.nb_replays
    run.alpha, run.gamma, run.epsilon = ag.learning_rate, ag.gamma, pol.epsilon
    M._session(env.seed, env.instance_base, env.handle.n_worlds)
    M._sync_mode()
    ag._plan(flags)
    ag.inst[:, L.I_CTR_MEMORY] = M.counter
    L.check(L.lib().cobel_sfma_run(env.handle.ptr, C.byref(run), L.current_stream(ag.device)))
    M.counter.copy_(ag.inst[:, L.I_CTR_MEMORY])


class Holder:
    pass


def swap_memory(frames, M, dev, n_worlds):
    frames.swap(M, 'table', fc.MODEL_POISON)
    frames.swap(M, 'strength', fc.BIG)
    frames.swap(M, 'stamp', 0)                 # (a store clock: 0, never stored)
    frames.swap(M, 'state', SI_POISON)
    frames.swap(M, 'counter', fc.MARK)
    M._metric_on(dev, n_worlds)
    frames.swap(M, '_metric_dev', fc.BIG)
    if M.recency:
        tab = M._recency_table(dev)
        M._recency = (M._recency[0], frames.add('recency_tab', tab, fc.BIG))


def drive(h, w, opts, extra, framed, trial_cap, trace_cap, per_instance, batch=8, shift=0):
    L = _lib()
    env, ag = build(h, w, opts)
    ag.track_instances = per_instance
    ag.track_occupancy = per_instance
    ag.track_responses = True
    ag._bind(env)
    ag._env_in(env)
    pol = ag.policy
    flags = L.F_LEARN | extra | ag._policy_in(pol, env, False)
    if ag.mask_actions:
        flags |= L.F_MASK_ACTIONS
    ag.monitors.reserve(trial_cap, N, per_instance)
    assert ag.monitors.cap == trial_cap
    t = Holder()
    t.trace = t.trace_len = None
    if trace_cap:
        t.trace = torch.zeros((N, trace_cap * EVENT_BYTES), dtype=torch.uint8, device=ag.device)
        t.trace_len = torch.zeros(N, dtype=torch.int32, device=ag.device)
    if ag.random:
        ag._random_cdf()
    frames = None
    if framed:
        frames = fc.Frames(shift)
        fc.swap_fused(frames, ag)
        frames.swap(ag, '_q', fc.BIG)
        frames.swap(ag, 'replays_done', fc.MARK)
        swap_memory(frames, ag.M, ag.device, env.handle.n_worlds)
        frames.swap(ag, '_cdf', 1.0)            # (a CDF ends in ones)
        frames.swap(t, 'trace', 0x5A)
        frames.swap(t, 'trace_len', fc.MARK)
        if ag.mask_actions:
            fc.frame_mask(frames, ag)
    # six trials in two launches: a budget of 25 steps, then to the end
    launch(ag, env, pol, flags, 6, 12, 25, batch, t.trace, t.trace_len)
    launch(ag, env, pol, flags, 6, 12, 0, batch, t.trace, t.trace_len)
    torch.cuda.synchronize()
    M = ag.M
    out = {'q': ag._q, 'inst': ag.inst, 'last_exp': ag._last_exp, 'replays_done': ag.replays_done,
           'model': M.table, 'strength': M.strength, 'stamp': M.stamp, 'state': M.state,
           'counter': M.counter}
    if trace_cap:
        out.update(trace=t.trace, trace_len=t.trace_len)
    out.update(fc.monitor_arrays(ag.monitors))
    return {k: v.clone() for k, v in out.items()}, ag, frames


# What ``cobel_sfma_plan`` tells is the form (LDS / streaming) and the threads of an instance.
# WHICH kernel of the LDS form with one wave ran — the fast one, a specialised one or the general
# one — the library does not report: for the first five cases below the form is NOT verified on
# the device.  Each is held to the conditions by which ``cobel_sfma_run`` routes (csrc/sfma.hip),
# asserted on the launch's own arguments in ``_case``: no trace, no per-instance monitors, no
# occupancy and no ``last_exp`` for the fast kernel; a plain mode and at most 512 experiences for a
# specialised one; ``F_FORCE_WAVE`` or one of the recency / normalisation / deterministic switches
# for the general one.
CASES = {
    # name: (h, w, options, extra flags, trace, per-instance monitors, plan [form, threads])
    'fast_5x5': (5, 5, {}, 0, False, False, [0, 64]),
    'specialised_6x7_reverse_trace': (6, 7, {'mode': 'reverse'}, 0, True, True, [0, 64]),
    'specialised_5x5_blend_forward_mask': (5, 5, {'mode': 'blend_forward', 'mask': True}, 0, True,
                                           True, [0, 64]),
    'general_force_wave_sweeping_start': (6, 7, {'mode': 'sweeping', 'start_replay': True},
                                          'F_FORCE_WAVE', True, True, [0, 64]),
    'general_recency_6x7': (6, 7, {'mode': 'default', 'recency': True}, 0, True, True, [0, 64]),
    'four_waves_15x15_interpolate': (15, 15, {'mode': 'interpolate', 'nb_replays': 2}, 0, True,
                                     True, [0, 256]),
    'four_waves_15x15_random': (15, 15, {'random': True}, 0, True, True, [0, 256]),
    'stream_5x5_reverse': (5, 5, {'mode': 'reverse'}, 'F_SFMA_STREAM', True, True, [1, 256]),
    'stream_15x15_recency_mask': (15, 15, {'recency': True, 'mask': True}, 'F_SFMA_STREAM', True,
                                  True, [1, 256]),
    'stream_15x15_random_start': (15, 15, {'random': True, 'start_replay': True}, 'F_SFMA_STREAM',
                                  True, True, [1, 256]),
    'stream_36x36_beyond_lds': (36, 36, {'mode': 'blend_forward'}, 0, True, True, [1, 1024]),
}
TIERS = {
    'stream_tier_24B_1505': (35, 43, {'mode': 'sweeping'}, 0, True, True, [1, 1024]),
    'stream_tier_8B_2006': (34, 59, {'mode': 'interpolate', 'recency': True}, 0, True, True,
                            [1, 1024]),
}


def _routed(ag, extra, trace, experiences):
    """The one-wave kernel ``cobel_sfma_run`` gives this launch (csrc/sfma.hip), restated from the
    launch's own arguments — the library reports the form and the threads only."""
    L = _lib()
    M, mon = ag.M, ag.monitors
    special = M.recency or M.C_normalize or M.D_normalize or M.deterministic
    if special or (extra & L.F_FORCE_WAVE) or not M.R_normalize or experiences > 512:
        return 'general'
    slow = ag.random or ag.dynamic or ag.start_replay or M.reward_mod_local or M.reward_mod \
        or M.state_mod
    fast = (experiences <= 128 and not slow and ag.nb_replays == 1 and M.decay_strength == 1.0
            and 0.0 <= M.beta <= 700.0 and M.R_threshold >= 0.0 and not trace
            and mon.lat_trace is None and mon.occupancy is None)
    return 'fast' if fast else 'specialised'


def _case(h, w, opts, extra, trace, per_instance, plan, shift=0, kernel=None):
    L = _lib()
    extra = getattr(L, extra) if extra else 0
    how = dict(trial_cap=2, trace_cap=5 if trace else 0, per_instance=per_instance)
    plain, _, _ = drive(h, w, opts, extra, False, **how)
    framed, ag, frames = drive(h, w, opts, extra, True, shift=shift, **how)
    frames.check()
    fc.assert_same(plain, framed)
    got = list(ag.launch_plan)
    assert [got[0], got[2]] == plan, got
    if kernel is not None:
        assert plan == [0, 64] and _routed(ag, extra, trace, 4 * h * w) == kernel
    S = h * w
    assert (framed['inst'][:, L.I_TRIAL] == 6).all() and 6 > how['trial_cap']
    q, c = framed['q'].cpu().numpy(), framed['strength'].cpu().numpy().reshape(N, 4, S)
    assert q[-1].any() and q[:, -1].any(), 'Q unchanged in the last instance / for the last state'
    assert c[-1].any() and c[:, :, -1].any(), 'strengths unchanged there'
    assert int(framed['replays_done'].item()) > 0
    if trace:
        lens = framed['trace_len'].cpu().numpy()
        assert (lens > how['trace_cap']).all(), 'fewer replay events than trace_cap: %r' % lens
    return ag


@pytest.mark.parametrize('name', list(CASES))
def test_sfma_run(name):
    first = name.split('_')[0]
    ag = _case(*CASES[name], kernel=first if first in ('fast', 'specialised', 'general') else None)
    if 'random' in name:
        assert ag.random and ag._cdf is not None


@pytest.mark.parametrize('name', list(TIERS))
def test_sfma_run_narrow_streaming_tiers(name, monkeypatch):
    """The two narrower tiers of the streaming form on small worlds, with the LDS it may take
    lowered to 48 KiB: 24 bytes per state at 1 505 states, 8 at 2 006."""
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_SFMA_STREAM_LDS', str(48 * 1024))
    h, w = TIERS[name][:2]
    ag = _case(*TIERS[name])
    per_state = 24 if h * w == 1505 else 8
    assert list(ag.launch_plan)[1] == ((per_state * h * w + 15) & ~15) + 512 + 384 + 128


# -- the memory's own calls ----------------------------------------------------------------------------
def _memory(S_hw, stream, recency):
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.memory.utils import Euclidean
    h, w = S_hw
    mem = SFMAMemory(Euclidean(w, h).D, h * w, 4)
    mem.recency = recency
    mem.mode = 'reverse'
    mem.launch_flags = _lib().F_SFMA_STREAM if stream else 0
    mem.bind(N, torch.device('cuda', 0), seed=SEED, instance_base=9)
    return mem


@pytest.mark.parametrize('stream', [False, True])
@pytest.mark.parametrize('hw', [(5, 5), (6, 7)])
def test_sfma_memory_calls(hw, stream):
    """store, replay (one replay, and three side by side: strided), random batch — on the LDS form
    and the streaming form; ``events[N][R][L]``, ``lengths`` and ``inhibition`` framed."""
    L = _lib()
    lib = L.lib()
    h, w = hw
    S = h * w
    rng = np.random.default_rng(S)
    n_exp = 12
    exps = []
    for j in range(n_exp):
        s = rng.integers(0, S, N)
        s[-1] = S - 1 if j % 3 == 0 else s[-1]
        a = rng.integers(0, 4, N)
        exps.append({'state': s, 'action': a, 'next_state': rng.integers(0, S, N),
                     'terminal': rng.integers(0, 2, N),
                     'reward': rng.choice([1.0, -0.5, 0.25], N)})
    from cobel_amd.memory.sfma import EXPERIENCE
    from cobel_amd.memory import _device
    mask = np.ones(4 * S)
    mask[::5] = 0
    cdf = np.cumsum(mask / mask.sum())
    cdf /= cdf[-1]
    outs = []
    for framed in (False, True):
        mem = _memory(hw, stream, recency=True)
        dev = mem.table.device
        frames = fc.Frames()
        if framed:
            swap_memory(frames, mem, dev, 1)
        assert mem.launch_plan()[0] == int(stream)
        out = {}
        for e in exps:
            m, _ = mem._mem(0)
            rec = _device.records(e, N, EXPERIENCE, {'state': S, 'action': 4, 'next_state': S},
                                  skip=('td',))
            x = torch.as_tensor(rec.view(np.uint8), device=dev)
            if framed:
                x = frames.add('exps', x, 0)
            L.check(lib.cobel_sfma_store(C.byref(m), L.ptr(x), L.current_stream(dev)))
        for key, R, length, strided in (('one', 1, 6, False), ('three', 3, 6, True)):
            m, _ = mem._mem(L.SFM_STRIDED if strided else 0)
            ev = torch.zeros((N, R, length * EVENT_BYTES), dtype=torch.uint8, device=dev)
            ln = torch.zeros((N, R), dtype=torch.int32, device=dev)
            inh = torch.zeros((N, S), dtype=torch.float64, device=dev)
            st = torch.full((N,), S - 1, dtype=torch.int32, device=dev)
            ac = torch.zeros(N, dtype=torch.int32, device=dev)
            if framed:
                ev, ln = frames.add('events', ev, 0x5A), frames.add('lengths', ln, fc.MARK)
                inh = frames.add('inhibition', inh, fc.BIG)
                st, ac = frames.add('state', st, 0), frames.add('action', ac, 0)
            L.check(lib.cobel_sfma_replay(C.byref(m), R, length, L.ptr(st), L.ptr(ac), L.ptr(ev),
                                          L.ptr(ln), L.ptr(inh), L.current_stream(dev)))
            out.update({key + '_events': ev, key + '_lengths': ln, key + '_inhibition': inh})
        m, _ = mem._mem(0)
        k = 7
        cd = torch.as_tensor(cdf, device=dev)
        ev = torch.zeros((N, k * EVENT_BYTES), dtype=torch.uint8, device=dev)
        if framed:
            cd, ev = frames.add('random_cdf', cd, 1.0), frames.add('random_events', ev, 0x5A)
        L.check(lib.cobel_sfma_random_batch(C.byref(m), k, L.ptr(cd), L.ptr(ev),
                                            L.current_stream(dev)))
        torch.cuda.synchronize()
        if framed:
            frames.check()
        out.update(random_events=ev, model=mem.table, strength=mem.strength, stamp=mem.stamp,
                   state=mem.state, counter=mem.counter)
        outs.append({k_: v.clone() for k_, v in out.items()})
        assert int(out['one_lengths'].min().item()) >= 1 and int(out['three_lengths'].min().item()) >= 1
        assert bool(out['one_inhibition'][-1].any()) and bool(mem.strength[-1].any())
        assert bool(mem.strength.view(N, 4, S)[:, :, -1].any()), 'nothing stored for the last state'
        assert int(mem.counter.min().item()) > 0
    fc.assert_same(*outs)


@pytest.mark.parametrize('name', ['specialised_6x7_reverse_trace', 'four_waves_15x15_interpolate',
                                  'stream_15x15_recency_mask'])
def test_tables_sixteen_bytes_off_a_256_byte_boundary(name):
    """cobel_sfma_run checks ``q`` (and, for the streaming form, ``strength`` and ``stamp``) for 16
    bytes and the record tables for 8; its widest access is 16 bytes at a multiple of 16 from a
    table's base.  Every framed table starts 16 bytes behind a 256-byte boundary; same assertions."""
    ag = _case(*CASES[name], shift=16)
    assert ag._q.data_ptr() % 256 == 16 and ag.M.strength.data_ptr() % 256 == 16
