"""A plain restatement of one cobel_dqn_act_c2d call (csrc/dqn_act_c2d.hip) in NumPy and Python,
one instance after the other, composed of what the tests of its parts already hold: the selection
and the ring of tests/dqn_act_common.py (``select``, ``ring_store``), the arena of
tests/c2d_common.py (``step``, ``reset``, ``draw``) and the draws of oracle/philox.py — and seeded
cases whose conditions are asserted on the restatement alone (tests/test_host_dqn_c2d.py).

An arena is ``{'T', 'S', 'R', 'box', 'fallback', 'robot', 'params'}`` (edge table, spawn table,
reward rows, candidate box, fallback point, c2d_common.STEP / WHEEL, the scalars of c2d_common.step);
a state is a dict of arrays named as the fields of cobel_dqn_c2d_act_t ('state' and 'env_ctr' are
the arena's); the scalars are ``par``.  The restatement is exact for the step robot (the wheel
robot's targets go through cos / sin, which NumPy and the device round differently)."""
import numpy as np

import c2d_common as cc
import dqn_act_common as dac
from oracle import philox

M32 = 0xFFFFFFFF
ARRAYS = ('state', 'env_ctr', 'q', 'policy_ctr') + dac.RING + (
    'memory_ctr', 'trial', 'step', 'trial_reward', 'active', 'adam_steps', 'lat_sum', 'lat_cnt',
    'reward_sum', 'stepped', 'batch_slots', 'obs', 'reward_out', 'done_out', 'wall_out', 'fallbacks')
K_CALLS = 12


def reset(arena, seed, g, c):
    """c2d_common.reset in this arena.  Where the spawn rings lie wholly outside the candidate box
    ('no_spawn': no candidate can be inside them) and the robot is the step robot (orientation 0,
    whatever the draw), the 2 048 draws of the refused candidates decide nothing and are left out:
    the fallback point, the counter + 2052.  tests/test_host_dqn_c2d.py holds this against
    c2d_common.reset itself."""
    if arena.get('no_spawn') and arena['robot'] == cc.STEP:
        return (float(arena['fallback'][0]), float(arena['fallback'][1]), 0.0), (c + 2052) & M32, True, None
    return cc.reset(arena['T'], arena['S'], arena['box'], arena['fallback'], arena['robot'], seed, g, c)


def act_step(arena, par, st, log=None):
    """The state after one cobel_dqn_act_c2d call on ``st``: a new dict, the arguments left alone.
    ``log`` receives one (i, action, done, timed_out, restarted, candidates refused or None for the
    fallback, wall, ring_was_full) per instance that stepped."""
    out = {k: None if a is None else np.array(a, copy=True) for k, a in st.items()}
    T = np.float64 if par['is_float64'] else np.float32
    robot, seed, slots, batch = arena['robot'], par['seed'], par['slots'], par['batch']
    D = 2 if robot == cc.STEP else 3
    stripes = max(par['mon_stripes'], 1)
    for i in range(par['n']):
        if not st['active'][i]:                # finished all its trials: frozen, consumes nothing
            out['stepped'][i] = 0
            continue
        g = (par['instance_base'] + i) & M32
        # select
        q = np.asarray(st['q'][i], dtype=T)
        pc = int(st['policy_ctr'][i])
        u = float(philox.draw_double(seed, g, pc, 0, par['policy_stream']))
        out['policy_ctr'][i] = (pc + 1) & M32
        a, _ = dac.select(q, par['epsilon'], u)
        # Continuous2D.step
        before = tuple(float(v) for v in st['state'][i])
        after, reward, done, wall = cc.step(arena['T'], arena['R'], robot, before, int(a), arena['params'])
        out['reward_out'][i], out['done_out'][i], out['wall_out'][i] = reward, done, wall
        # store: the observation before the step and after it (before any reset)
        size, head = int(st['ring_size'][i]), int(st['ring_head'][i])
        full = size >= slots
        slot, size, head = dac.ring_store(size, head, slots)
        out['ring_states'][i, slot] = np.asarray(before[:D]).astype(T)
        out['ring_next_states'][i, slot] = np.asarray(after[:D]).astype(T)
        out['ring_actions'][i, slot] = a
        out['ring_rewards'][i, slot] = T(reward)
        out['ring_nonterminal'][i, slot] = T(0.0 if done else 1.0)
        out['ring_size'][i], out['ring_head'][i] = size, head
        # trial bookkeeping, monitors
        trial, step = int(st['trial'][i]), int(st['step'][i])
        trew = np.float64(st['trial_reward'][i]) + np.float64(reward)
        timed_out = step + 1 >= par['steps_per_trial']
        state, active, restarted, refused = after, True, False, 0
        if done or timed_out:
            if trial < par['trial_cap']:
                m = (i % stripes, trial)
                out['lat_sum'][m] += step
                out['lat_cnt'][m] += 1
                out['reward_sum'][m] += trew
            trial, trew, step = trial + 1, np.float64(0.0), 0
            active = trial < par['trials_target']
            if active:                          # auto-reset: cobel_c2d_reset for this instance
                state, ctr, fell, refused = reset(arena, seed, g, int(st['env_ctr'][i]))
                out['env_ctr'][i] = ctr
                out['fallbacks'][0] += int(fell)
                restarted = True
        else:
            step += 1
        out['state'][i] = state
        out['obs'][i] = state[:D]
        out['trial'][i], out['step'][i] = trial, step
        out['trial_reward'][i], out['active'][i] = trew, 1 if active else 0
        out['stepped'][i] = 1
        out['adam_steps'][i] += 1.0
        if log is not None:
            log.append((i, int(a), bool(done), (not done) and timed_out, restarted, refused, int(wall), full))
        # the batch: sub j of ONE counter of the memory stream
        mc = int(st['memory_ctr'][i])
        out['memory_ctr'][i] = (mc + 1) & M32
        if batch > 0:
            idx = philox.draw_bounded(seed, g, mc, np.arange(batch), dac.STREAM_MEMORY, size)
            out['batch_slots'][i] = (head + idx) % slots
    return out


# ---------------------------------------------------------------------------------------------
# arenas
def arenas():
    """name -> arena (step robot).  'open_field' and 'eight': spawn anywhere in the arena, so a
    reset refuses the candidates that fall into an obstacle or outside.  'wedge': the thin triangle
    c2d_common.WEDGE with a spawn ring that no candidate of its box can lie in — every reset takes
    the fallback point (0.5, 0) — walls 0.00875 above and below it (steps of 0.015 up and down end
    at them) and a reward three steps to its right."""
    out = {}
    for name in ('open_field', 'eight'):
        T, R = cc.geometries()[name]    # noqa: N806
        box = cc.bounds(T)
        out[name] = dict(T=T, S=T, R=R, box=box, fallback=cc.first_grid_point(T, T, box)[0],
                         robot=cc.STEP, params=dict(cc.DEFAULTS, punish_wall=1))
    T = cc.table(cc.WEDGE)    # noqa: N806
    far = cc.table([(5.0, 5.0), (6.0, 5.0), (6.0, 6.0), (5.0, 6.0)])
    out['wedge'] = dict(T=T, S=far, R=np.array([[0.64, 0.0, 3.0]]), box=cc.bounds(T),
                        fallback=(0.5, 0.0), robot=cc.STEP, params=dict(cc.DEFAULTS, punish_wall=1),
                        no_spawn=True)
    assert cc.bounds(far)[0] > out['wedge']['box'][2]      # the spawn ring: right of the whole box
    return out


BASE = dict(n=70, batch=3, slots=5, steps_per_trial=5, trials_target=3, trial_cap=4, mon_stripes=3,
            instance_base=10, epsilon=0.3, policy_stream=dac.STREAM_POLICY)
CONDITIONS = ('all_actions', 'by_done', 'by_limit', 'some_frozen', 'some_active', 'ring_wraps',
              'later_candidate', 'wall')
# what an arena's own geometry decides: every reset in the wedge is the fallback (and only there)
NEEDS = {'open_field': set(CONDITIONS), 'eight': set(CONDITIONS),
         'wedge': (set(CONDITIONS) - {'later_candidate'}) | {'fallback'}}


def draw_q(rng, n, k, T, mode='mixed'):
    """The Q table [n, 4] of call k: 'mixed' — 1 + (i + k) mod 4 maximal entries among a handful of
    values, as dqn_act_common.draw_q; 'ties' — all four equal."""
    if mode == 'ties':
        return np.full((n, 4), 0.5, dtype=T)
    return dac.draw_q(rng, n, 4, k, T)


def _start_near(arena, rng, i):
    """A clear start: every other one a step or two outside the reach of the first reward row (on
    one of the four axes through it, so that one action leads there), else near a wall."""
    T, R = arena['T'], arena['R']    # noqa: N806
    if len(R) and i % 2 == 0:
        for _ in range(64):
            ux, uy = cc.MOVES[int(rng.integers(4))]
            dist = 0.1 + rng.uniform(0.001, 0.028)
            x, y = float(R[0][0]) - ux * dist, float(R[0][1]) - uy * dist
            if cc.clear(T, x, y):
                return x, y
    return tuple(cc.planted_starts(T, 1, rng)[0])


def _draw_case(name, f64, seed, mode, changes):
    arena = arenas()[name]
    rng = np.random.default_rng([seed, 0xC2DA])
    par = dict(BASE, **changes)
    par.update(seed=0xC0BE1 + 7919 * seed, is_float64=int(f64))
    n, slots, batch, cap = par['n'], par['slots'], par['batch'], par['trial_cap']
    T = np.float64 if f64 else np.float32
    stripes = max(par['mon_stripes'], 1)
    ctr = (np.arange(n) % 3).astype(np.uint32)
    st = {k: None for k in ARRAYS}
    st['state'] = np.zeros((n, 3))
    for i in range(n):
        st['state'][i, :2] = _start_near(arena, rng, i)
    st['env_ctr'] = (2 * ctr).astype(np.uint32)            # (kept even, as cobel_c2d_reset keeps it)
    st['policy_ctr'], st['memory_ctr'] = ctr[::-1].copy(), (ctr + 1).astype(np.uint32)
    st['q'] = np.full((n, 4), np.nan, dtype=T)
    st['trial'], st['step'] = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    st['trial_reward'], st['active'] = np.zeros(n), np.ones(n, dtype=np.uint8)
    st['adam_steps'] = np.arange(n, dtype=np.float64)
    st['lat_sum'] = np.zeros((stripes, cap), dtype=np.int64)
    st['lat_cnt'] = np.zeros((stripes, cap), dtype=np.int64)
    st['reward_sum'] = np.zeros((stripes, cap))
    st['stepped'] = np.full(n, 0xA5, dtype=np.uint8)
    st['ring_states'] = np.full((n, slots, 2), -7.5, dtype=T)
    st['ring_next_states'] = np.full((n, slots, 2), -7.5, dtype=T)
    st['ring_actions'] = np.full((n, slots), 2 ** 40, dtype=np.int64)
    st['ring_rewards'] = np.full((n, slots), -7.5, dtype=T)
    st['ring_nonterminal'] = np.full((n, slots), -7.5, dtype=T)
    st['ring_size'], st['ring_head'] = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    st['batch_slots'] = np.full((n, batch), -7, dtype=np.int32)
    st['obs'] = np.full((n, 2), -7.5)
    st['reward_out'] = np.full(n, -7.5)
    st['done_out'], st['wall_out'] = np.full(n, 0xA5, dtype=np.uint8), np.full(n, 0xA5, dtype=np.uint8)
    st['fallbacks'] = np.zeros(1, dtype=np.int32)
    qs = [draw_q(rng, n, k, T, mode) for k in range(K_CALLS)]
    # (instance 1 is frozen from the start in every case of more than one instance, so that
    #  "nothing of its own is written" is held from the first call on)
    if n > 1:
        st['active'][1], st['trial'][1] = 0, par['trials_target']
    return {'name': name, 'arena': arena, 'par': par, 'state': st, 'qs': qs, 'seed': seed}


def simulate(case):
    """The K calls of a case through the restatement: (Q table handed in, state afterwards) per
    call — rows of instances that are frozen at that call hold NaN — and the log of every call."""
    st, steps, logs = case['state'], [], []
    for q in case['qs']:
        q = q.copy()
        q[st['active'] == 0] = np.nan
        log = []
        st = act_step(case['arena'], case['par'], dict(st, q=q), log)
        steps.append((q, st))
        logs.append(log)
    return steps, logs


def conditions(case, steps, logs):
    """Which of CONDITIONS (and 'fallback') the K calls of a case meet."""
    events = [e for log in logs for e in log]
    met = set()
    if {e[1] for e in events} == {0, 1, 2, 3}:
        met.add('all_actions')
    if any(e[2] for e in events):
        met.add('by_done')
    if any(e[3] for e in events):
        met.add('by_limit')
    went = {e[0] for e in events}
    if any((steps[-2][1]['active'][i] == 0) for i in went):   # stepped once, frozen before call K
        met.add('some_frozen')
    if len(logs[-1]) > 0:
        met.add('some_active')
    if any(e[7] for e in events):
        met.add('ring_wraps')
    if any(e[4] and e[5] is not None and e[5] > 0 for e in events):
        met.add('later_candidate')
    if any(e[4] and e[5] is None for e in events):
        met.add('fallback')
    if any(e[6] for e in events):
        met.add('wall')
    return met


_CASES: dict = {}


def make_case(name, f64, mode='mixed', tries=40, **changes):
    """The case of arena ``name`` from the first seed whose K calls meet every condition of
    NEEDS[name] (a case of one instance, or of ties only, is held to no condition), computed once
    per argument list.  Returns the case with its 'steps' and 'logs'."""
    key = (name, f64, mode, tuple(sorted(changes.items())))
    if key in _CASES:
        return _CASES[key]
    free = mode != 'mixed' or changes.get('n', BASE['n']) < 20 or 'epsilon' in changes
    first = 100 * (1 + sorted(NEEDS).index(name))
    for seed in range(first, first + tries):
        case = _draw_case(name, f64, seed, mode, changes)
        steps, logs = simulate(case)
        if free or NEEDS[name] <= conditions(case, steps, logs):
            case['steps'], case['logs'] = steps, logs
            _CASES[key] = case
            return case
    raise AssertionError('%s: no seed in %d .. %d meets %s' % (name, first, first + tries - 1,
                                                              sorted(NEEDS[name])))


def same(got, ref):
    """The names of the arrays that differ (bit for bit; NaN equals NaN)."""
    bad = []
    for k in ARRAYS:
        a, b = got[k], ref[k]
        if not (a.dtype == b.dtype and a.shape == b.shape and
                np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')):
            bad.append(k)
    return bad
