"""A plain restatement of one cobel_dqn_act call (csrc/dqn_act.hip: k_dqn_act + k_dqn_batch) in
NumPy and Python, one instance after the other, and what the tests around it share: seeded cases,
world builders through the C ABI, and the filler of ``_lib.DQNAct`` with every device array framed
by sentinels.

The restatement takes nothing from cobel_amd.  Its draws are oracle/philox.py's (draw_double /
draw_bounded) on the streams, counters and subs the kernel's header lists:
    policy stream (COBEL_STREAM_POLICY or .._TEST), counter policy_ctr[i], sub 0: one double
    COBEL_STREAM_ENV, counter env_ctr[i], sub 0: one integer below the start count, at a restart
    COBEL_STREAM_MEMORY, counter memory_ctr[i], sub j = 0 .. batch - 1: the batch
all of instance g = (instance_base + i) mod 2^32.  The selection is oracle/ref_loop.py's
RefEpsilonGreedy (policy/greedy.py as csrc/cobel_policy.h describes it: float64 probabilities, ties
by exact equality in the Q dtype, sequential cumulative sum, division by the last entry,
searchsorted(side='right')), pinned to the reference's golden rows by
tests/test_host_dqn_act_reference.py.

A world is ``{'next': uint16 [W, S, A], 'reward': float32 [W, S], 'terminal': uint8 [W, S],
'starts': [W lists]}``; a state is a dict of arrays named as the fields of cobel_dqn_act_t (None:
the pointer is NULL), the scalars are ``par``."""
import ctypes as C

import numpy as np

from mlp_gpu_common import DEV, PAD, Framed
from oracle import philox
from oracle.ref_loop import RefEpsilonGreedy

M32 = 0xFFFFFFFF
STREAM_ENV, STREAM_POLICY, STREAM_MEMORY, STREAM_POLICY_TEST = 0, 1, 2, 3
K_STEPS = 12
RING = ('ring_states', 'ring_next_states', 'ring_actions', 'ring_rewards', 'ring_nonterminal',
        'ring_size', 'ring_head')
MODEL = ('model_rewards', 'model_states', 'model_nonterminal', 'batch_state_index',
         'batch_next_index', 'batch_actions', 'batch_rewards', 'batch_nonterminal')
ARRAYS = ('state', 'env_ctr', 'obs_table', 'q', 'policy_ctr') + RING + (
    'memory_ctr', 'trial', 'step', 'trial_reward', 'active', 'adam_steps', 'lat_sum', 'lat_cnt',
    'reward_sum', 'stepped', 'batch_slots') + MODEL
SCALARS = ('n', 'n_obs', 'slots', 'batch', 'steps_per_trial', 'trials_target', 'trial_cap',
           'mon_stripes', 'instance_base', 'seed', 'epsilon', 'policy_stream', 'is_float64',
           'model_lr', 'n_states')


# ---------------------------------------------------------------------------------------------
# the restatement
class _One:
    """A generator that hands out one given double."""

    def __init__(self, u):
        self.u = u

    def random(self, size=None):
        return self.u


def select(q, epsilon, u, mask=None):
    """(action, probabilities) of policy/greedy.py on the values ``q`` (in their own dtype) with
    the double ``u`` as the draw of Generator.choice."""
    pol = RefEpsilonGreedy(epsilon, _One(u))
    return pol.select_action(q, mask), pol.get_action_probs(q, mask)


def ring_store(size, head, slots):
    """Where a FIFO ring of ``slots`` rows with ``size`` entries, the oldest in row ``head``, puts
    the next entry, and its size and head afterwards (memory/dqn.py:103-119)."""
    slot = (head + size) % slots
    if size >= slots:
        return slot, size, (head + 1) % slots
    return slot, size + 1, head


def act_step(world, par, st, log=None):
    """The state after one cobel_dqn_act call on ``st``: a new dict, every array of ``st`` copied
    and the arguments left alone.  ``log``: a list that receives one (i, action, ties, done,
    timed_out, restarted, ring_was_full) per instance that stepped."""
    out = {k: None if a is None else np.array(a, copy=True) for k, a in st.items()}
    T = np.float64 if par['is_float64'] else np.float32
    nxt, n_worlds, batch, slots = world['next'], world['next'].shape[0], par['batch'], par['slots']
    seed, dyna = par['seed'], st.get('model_rewards') is not None
    stripes = max(par['mon_stripes'], 1)
    draws_batch = dyna or st.get('batch_slots') is not None
    for i in range(par['n']):
        if not st['active'][i]:                # finished all its trials: frozen, consumes nothing
            out['stepped'][i] = 0
            continue
        g = (par['instance_base'] + i) & M32
        w = g % n_worlds
        # select
        q = np.asarray(st['q'][i], dtype=T)
        pc = int(st['policy_ctr'][i])
        u = float(philox.draw_double(seed, g, pc, 0, par['policy_stream']))
        out['policy_ctr'][i] = (pc + 1) & M32
        a, _ = select(q, par['epsilon'], u)
        # env.step: reward and end of the state ENTERED
        s = int(st['state'][i])
        ns = int(nxt[w, s, a])
        reward = np.float32(world['reward'][w, ns])
        done = bool(world['terminal'][w, ns])
        # store
        full = False
        if dyna:
            e = s * 4 + a
            old = np.float64(st['model_rewards'][i, e])
            out['model_rewards'][i, e] = old + np.float64(par['model_lr']) * (np.float64(reward) - old)
            out['model_states'][i, e] = ns
            out['model_nonterminal'][i, e] = 0.0 if done else 1.0
        else:
            size, head = int(st['ring_size'][i]), int(st['ring_head'][i])
            full = size >= slots
            slot, size, head = ring_store(size, head, slots)
            out['ring_states'][i, slot] = st['obs_table'][s].astype(T)
            out['ring_next_states'][i, slot] = st['obs_table'][ns].astype(T)
            out['ring_actions'][i, slot] = a
            out['ring_rewards'][i, slot] = T(reward)
            out['ring_nonterminal'][i, slot] = T(0.0 if done else 1.0)
            out['ring_size'][i], out['ring_head'][i] = size, head
        # trial bookkeeping, monitors, auto-reset
        trial, step = int(st['trial'][i]), int(st['step'][i])
        trew = np.float64(st['trial_reward'][i]) + np.float64(reward)
        timed_out = step + 1 >= par['steps_per_trial']
        state, active, restarted = ns, True, False
        if done or timed_out:
            if trial < par['trial_cap']:
                m = (i % stripes, trial)
                if st.get('lat_sum') is not None:
                    out['lat_sum'][m] += step
                if st.get('lat_cnt') is not None:
                    out['lat_cnt'][m] += 1
                if st.get('reward_sum') is not None:
                    out['reward_sum'][m] += trew
            trial, trew, step = trial + 1, np.float64(0.0), 0
            active = trial < par['trials_target']
            if active:
                starts = world['starts'][w]
                ec = int(st['env_ctr'][i])
                state = int(starts[int(philox.draw_bounded(seed, g, ec, 0, STREAM_ENV, len(starts)))])
                out['env_ctr'][i] = (ec + 1) & M32
                restarted = True
        else:
            step += 1
        out['state'][i], out['trial'][i], out['step'][i] = state, trial, step
        out['trial_reward'][i], out['active'][i] = trew, 1 if active else 0
        out['stepped'][i] = 1
        if st.get('adam_steps') is not None:
            out['adam_steps'][i] += 1.0
        if log is not None:
            log.append((i, a, int((q == q.max()).sum()), done, (not done) and timed_out, restarted, full))
        # the batch: sub j of ONE counter of the memory stream
        if not draws_batch:
            continue
        mc = int(st['memory_ctr'][i])
        out['memory_ctr'][i] = (mc + 1) & M32
        if batch <= 0:
            continue
        if dyna:
            pairs = par['n_states'] * 4
            idx = philox.draw_bounded(seed, g, mc, np.arange(batch), STREAM_MEMORY, pairs)
            out['batch_state_index'][i] = idx >> 2
            out['batch_next_index'][i] = out['model_states'][i, idx]
            out['batch_actions'][i] = idx & 3
            out['batch_rewards'][i] = out['model_rewards'][i, idx].astype(T)
            out['batch_nonterminal'][i] = out['model_nonterminal'][i, idx].astype(T)
        else:
            idx = philox.draw_bounded(seed, g, mc, np.arange(batch), STREAM_MEMORY, size)
            out['batch_slots'][i] = (head + idx) % slots
    return out


# ---------------------------------------------------------------------------------------------
# worlds
DYADIC = (1.0, -0.25, 0.5, 0.25)
NON_DYADIC = (0.1, -0.3, 0.7, 1.1)            # as float32: no partial sum of them is exact


def draw_world(rng, S, A, n_worlds, start_lens, rewards=DYADIC):
    """``n_worlds`` random worlds of S states and A actions: two terminal states per world with a
    reward on entering, one more rewarded state, start lists of the given lengths among the
    others."""
    assert len(start_lens) == n_worlds and S >= 6
    world = {'next': rng.integers(0, S, size=(n_worlds, S, A)).astype(np.uint16),
             'reward': np.zeros((n_worlds, S), dtype=np.float32),
             'terminal': np.zeros((n_worlds, S), dtype=np.uint8), 'starts': []}
    for w in range(n_worlds):
        order = rng.permutation(S)
        world['terminal'][w, order[:2]] = 1
        world['reward'][w, order[:3]] = np.asarray(rewards[:3], dtype=np.float32)
        world['reward'][w, order[3]] = np.float32(rewards[3]) * (w % 2)
        free = order[2:]
        world['starts'].append([int(s) for s in rng.choice(free, size=start_lens[w], replace=True)])
    return world


def create_world(world, device=0):
    """The world on the device through cobel_world_create (four actions: the record path) or
    cobel_world_create_n; returns the handle (cobel_world_destroy frees it)."""
    from cobel_amd import _lib
    n_worlds, S, A = world['next'].shape
    nxt = np.ascontiguousarray(world['next'], dtype=np.uint16)
    reward = np.ascontiguousarray(world['reward'], dtype=np.float32)
    terminal = np.ascontiguousarray(world['terminal'], dtype=np.uint8)
    starts = np.array([s for lst in world['starts'] for s in lst], dtype=np.uint16)
    off = np.concatenate([[0], np.cumsum([len(lst) for lst in world['starts']])]).astype(np.int32)
    handle = C.c_void_p()
    args = [_lib.ptr(nxt), _lib.ptr(reward), _lib.ptr(terminal), _lib.ptr(starts), _lib.ptr(off),
            S, n_worlds]
    if A == 4:
        rc = _lib.lib().cobel_world_create(*args, device, C.byref(handle))
    else:
        rc = _lib.lib().cobel_world_create_n(*args, A, device, C.byref(handle))
    _lib.check(rc)
    return handle


def set_one_hot_transitions(handle, world):
    """Distribution rows (cobel_world_set_transitions) that say what the table says: one successor
    of probability 1 per (state, action)."""
    from cobel_amd import _lib
    pairs = int(np.prod(world['next'].shape))
    off = np.arange(pairs + 1, dtype=np.uint32)
    succ = np.ascontiguousarray(world['next'].reshape(-1), dtype=np.uint16)
    cdf = np.ones(pairs, dtype=np.float64)
    _lib.check(_lib.lib().cobel_world_set_transitions(handle, _lib.ptr(off), _lib.ptr(succ),
                                                      _lib.ptr(cdf), pairs))


# ---------------------------------------------------------------------------------------------
# cases
BASE = dict(n=20, batch=3, slots=5, A=4, S=8, n_obs=6, f64=False, trials_target=3,
            steps_per_trial=7, trial_cap=8, mon_stripes=3, start_lens=(4,), instance_base=9,
            epsilon=0.3, policy_stream=STREAM_POLICY, ctr0=0, dyna=False, model_lr=0.9,
            rewards='dyadic', absent=(), K=K_STEPS, waive=())
CONDITIONS = ('all_actions', 'all_ties', 'by_done', 'by_limit', 'some_frozen', 'some_active',
              'ring_full5')
# Conditions a case's own parameters rule out (everything else is asserted for every case):
#   3 trials of at most 1 or 3 steps are over after 3 or 9 of the 12 calls: nobody is active at the
#   end, and a ring of 5 rows is never full for 5 steps;
#   one instance cannot be both frozen and active: n = 1 is drawn twice, once of each kind (the
#   frozen one takes fewer than 12 steps: its ring of 5 rows is not full for 5 of them).
SHORT = ('some_active', 'ring_full5')
CASES = {
    'base': {},
    'n1-freezes': dict(n=1, waive=('some_active', 'ring_full5')),
    'n1-active': dict(n=1, trials_target=40, waive=('some_frozen',)),
    'n63': dict(n=63), 'n64': dict(n=64), 'n65': dict(n=65), 'n130': dict(n=130),
    'batch0': dict(batch=0), 'batch1': dict(batch=1), 'batch32': dict(batch=32),
    'n65-batch4': dict(n=65, batch=4), 'n9-batch32': dict(n=9, batch=32),
    'spt1': dict(steps_per_trial=1, waive=SHORT), 'spt3': dict(steps_per_trial=3, waive=SHORT),
    # (3 trials of at most 3 steps once more, over 6 calls and with a ring of one row: nothing waived)
    'spt3-K6': dict(steps_per_trial=3, K=6, slots=1),
    'slots1': dict(slots=1), 'slots2': dict(slots=2), 'slots40': dict(slots=40),
    'no-batch_slots': dict(absent=('batch_slots',)),
    'no-batch_slots-no-memory_ctr': dict(absent=('batch_slots', 'memory_ctr')),
    'f64': dict(f64=True), 'n_obs1': dict(n_obs=1), 'n_obs7': dict(n_obs=7),
    'n_obs7-f64': dict(n_obs=7, f64=True),
    'cap0': dict(trial_cap=0), 'cap2': dict(trial_cap=2),
    'stripes0': dict(mon_stripes=0), 'stripes1': dict(mon_stripes=1), 'stripes-n': dict(mon_stripes=20),
    'stripes-n-non-dyadic': dict(mon_stripes=20, rewards='non-dyadic'),
    'no-lat_sum': dict(absent=('lat_sum',)), 'no-lat_cnt': dict(absent=('lat_cnt',)),
    'no-reward_sum': dict(absent=('reward_sum',)), 'no-adam_steps': dict(absent=('adam_steps',)),
    'A1': dict(A=1, S=6), 'A2': dict(A=2, S=7), 'A3': dict(A=3, S=9), 'A5': dict(A=5, S=10),
    'A6': dict(A=6, S=11, f64=True), 'A8': dict(A=8, S=12),
    'worlds3': dict(start_lens=(1, 4, 2)), 'worlds3-A6': dict(start_lens=(1, 4, 2), A=6, S=12),
    'base0-n130': dict(n=130, instance_base=0, start_lens=(1, 4, 2)),
    'base9-n130': dict(n=130, instance_base=9, start_lens=(1, 4, 2)),
    'base-wraps-n130': dict(n=130, instance_base=0xFFFFFFC0, start_lens=(1, 4, 2)),
    'eps0': dict(epsilon=0.0), 'eps1': dict(epsilon=1.0),
    'test-stream': dict(policy_stream=STREAM_POLICY_TEST),
    'ctr1': dict(ctr0=1), 'ctr5': dict(ctr0=5), 'ctr-wraps': dict(ctr0=0xFFFFFFFE),
}
for _lr in (0.1, 0.9, 1.0):
    for _batch in (1, 32):
        for _f64 in (False, True):
            # (non-dyadic rewards: reward_sum needs one writer per cell)
            CASES['model-lr%g-batch%d-%s' % (_lr, _batch, 'f64' if _f64 else 'f32')] = dict(
                dyna=True, S=6, model_lr=_lr, batch=_batch, f64=_f64, rewards='non-dyadic',
                mon_stripes=20)
CASES['model-batch0'] = dict(dyna=True, S=6, batch=0)


def spec_of(name):
    spec = dict(BASE, **CASES[name])
    spec['name'] = name
    return spec


def draw_q(rng, n, A, k, T):
    """The Q table of call k: instance i has 1 + (i + k) mod A maximal entries among values of a
    handful of numbers, the others below it (some -inf); now and then every entry is -inf."""
    q = np.empty((n, A), dtype=T)
    for i in range(n):
        ties = 1 + (i + k) % A
        top = rng.choice([0.0, 0.5, 1.0])
        low = [v for v in (-np.inf, -1.0, 0.0, 0.5) if v < top]
        if ties == A and rng.random() < 0.25:
            top = -np.inf
        row = rng.choice(low, size=A)
        row[rng.permutation(A)[:ties]] = top
        q[i] = row
    return q


def _draw_case(spec, seed):
    rng = np.random.default_rng([seed, 0xAC7])
    n, A, S, D, slots, batch = (spec[k] for k in ('n', 'A', 'S', 'n_obs', 'slots', 'batch'))
    T = np.float64 if spec['f64'] else np.float32
    world = draw_world(rng, S, A, len(spec['start_lens']), spec['start_lens'],
                       DYADIC if spec['rewards'] == 'dyadic' else NON_DYADIC)
    par = {k: spec[k] for k in ('n', 'n_obs', 'slots', 'batch', 'steps_per_trial', 'trials_target',
                                'trial_cap', 'mon_stripes', 'instance_base', 'epsilon',
                                'policy_stream', 'model_lr')}
    par.update(seed=0xC0BE1 + 7919 * seed, is_float64=int(spec['f64']), n_states=S if spec['dyna'] else 0)
    stripes, cap = max(spec['mon_stripes'], 1), spec['trial_cap']
    n_worlds = len(spec['start_lens'])
    ctr = ((spec['ctr0'] + np.arange(n) % 3) & M32).astype(np.uint32)
    st = {k: None for k in ARRAYS}
    st['state'] = np.array([world['starts'][((spec['instance_base'] + i) & M32) % n_worlds][0]
                            for i in range(n)], dtype=np.int32)
    st['env_ctr'], st['policy_ctr'], st['memory_ctr'] = ctr.copy(), ctr[::-1].copy(), (ctr + 1).astype(np.uint32)
    st['obs_table'] = rng.choice([0.1, 1.0 / 3.0, 0.5, -2.0, 1e-3, 7.0], size=(S, D))
    st['q'] = np.full((n, A), np.nan, dtype=T)
    st['trial'], st['step'] = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    st['trial_reward'], st['active'] = np.zeros(n), np.ones(n, dtype=np.uint8)
    st['adam_steps'] = np.arange(n, dtype=np.float64)
    st['lat_sum'] = np.zeros((stripes, cap), dtype=np.int64)
    st['lat_cnt'] = np.zeros((stripes, cap), dtype=np.int64)
    st['reward_sum'] = np.zeros((stripes, cap))
    st['stepped'] = np.full(n, 0xA5, dtype=np.uint8)
    if spec['dyna']:
        st['model_rewards'] = rng.choice([0.0, 0.1, -0.7], size=(n, S * 4))
        st['model_states'] = np.tile(np.repeat(np.arange(S, dtype=np.int64), 4), (n, 1))
        st['model_nonterminal'] = np.zeros((n, S * 4))
        st['batch_state_index'] = np.full((n, batch), -7, dtype=np.int32)
        st['batch_next_index'] = np.full((n, batch), -7, dtype=np.int32)
        st['batch_actions'] = np.full((n, batch), -7, dtype=np.int64)
        st['batch_rewards'] = np.full((n, batch), -7.5, dtype=T)
        st['batch_nonterminal'] = np.full((n, batch), -7.5, dtype=T)
    else:
        st['ring_states'] = np.full((n, slots, D), -7.5, dtype=T)
        st['ring_next_states'] = np.full((n, slots, D), -7.5, dtype=T)
        st['ring_actions'] = np.full((n, slots), 2 ** 40, dtype=np.int64)
        st['ring_rewards'] = np.full((n, slots), -7.5, dtype=T)
        st['ring_nonterminal'] = np.full((n, slots), -7.5, dtype=T)
        st['ring_size'], st['ring_head'] = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
        st['batch_slots'] = np.full((n, batch), -7, dtype=np.int32)
    for name in spec['absent']:
        st[name] = None
    qs = [draw_q(rng, n, A, k, T) for k in range(spec['K'])]
    return {'spec': spec, 'world': world, 'par': par, 'state': st, 'qs': qs, 'seed': seed}


def simulate(case):
    """The K calls of a case through the restatement: (Q table handed in, state afterwards) per
    call — rows of instances that are frozen at that call hold NaN — and the log of every call."""
    st, steps, logs = case['state'], [], []
    for q in case['qs']:
        q = q.copy()
        q[st['active'] == 0] = np.nan
        log = []
        st = act_step(case['world'], case['par'], dict(st, q=q), log)
        steps.append((q, st))
        logs.append(log)
    return steps, logs


def conditions(case, steps, logs):
    """Which of CONDITIONS the K calls of a case meet."""
    spec = case['spec']
    A, n = spec['A'], spec['n']
    events = [e for log in logs for e in log]
    met = set()
    if {e[1] for e in events} == set(range(A)):
        met.add('all_actions')
    if {e[2] for e in events} == set(range(1, A + 1)):
        met.add('all_ties')
    if any(e[3] for e in events):
        met.add('by_done')
    if any(e[4] for e in events):
        met.add('by_limit')
    if (steps[-2][1]['active'] == 0).any():             # frozen BEFORE call K: a later call skips it
        met.add('some_frozen')
    if len(logs[-1]) > 0:                               # still stepping AT call K
        met.add('some_active')
    full = np.zeros(n, dtype=int)
    for e in events:
        full[e[0]] += e[6]
    if spec['dyna'] or spec['slots'] > 5 or full.max() >= 5:
        met.add('ring_full5')
    return met


def make_case(name, tries=200):
    """The case ``name`` of CASES from the first of seed, seed + 1, ... whose K calls meet every
    condition its parameters do not rule out (CONDITIONS minus the case's 'waive'); raises if none
    of ``tries`` seeds will do.  Returns the case with its 'steps' and 'logs' (simulate)."""
    spec = spec_of(name)
    need = set(CONDITIONS) - set(spec['waive'])
    first = 1000 * (1 + sorted(CASES).index(name))
    for seed in range(first, first + tries):
        case = _draw_case(spec, seed)
        steps, logs = simulate(case)
        if need <= conditions(case, steps, logs):
            case['steps'], case['logs'] = steps, logs
            return case
    raise AssertionError('%s: no seed in %d .. %d meets %s' % (name, first, first + tries - 1,
                                                              sorted(need)))


# ---------------------------------------------------------------------------------------------
# the device side
def _torch_dtype(torch, a):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
            np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32}[a.dtype]


def _as_signed(a):
    """uint32 counters travel as the int32 of the same bits."""
    return a.view(np.int32) if a.dtype == np.uint32 else a


class DeviceCase:
    """The state of a case on the device, every array in a sentinel frame, and its world."""

    def __init__(self, torch, case):
        self.torch, self.case = torch, case
        self.host0 = case['state']
        self.framed = {}
        for k, a in case['state'].items():
            if a is None:
                continue
            dt = _torch_dtype(torch, a)
            fill = -777.25 if dt.is_floating_point else (0x5A if dt == torch.uint8 else -777)
            f = Framed(torch, a.shape, dt, fill=fill)
            f.view.copy_(torch.from_numpy(np.ascontiguousarray(_as_signed(a))).to(DEV))
            self.framed[k] = f
        self.world = create_world(case['world'])

    def close(self):
        from cobel_amd import _lib
        if self.world is not None:
            _lib.lib().cobel_world_destroy(self.world)
            self.world = None

    def set_q(self, q):
        self.framed['q'].view.copy_(self.torch.from_numpy(np.ascontiguousarray(q)).to(DEV))

    def fill(self, **changes):
        """``_lib.DQNAct`` of this case; ``changes``: scalars by name, or array names set to None
        (NULL)."""
        from cobel_amd import _lib
        run = _lib.DQNAct()
        for k in ARRAYS:
            f = self.framed.get(k)
            setattr(run, k, None if f is None or (k in changes and changes[k] is None)
                    else f.buf.data_ptr() + PAD * f.buf.element_size())   # (also of an empty view)
        for k in SCALARS:
            setattr(run, k, changes.get(k, self.case['par'][k]))
        return run

    def launch(self, run, world=None):
        """The return code of cobel_dqn_act, after the device has finished."""
        from cobel_amd import _lib
        rc = _lib.lib().cobel_dqn_act(self.world if world is None else world, C.byref(run), None)
        self.torch.cuda.synchronize()
        return rc

    def read(self):
        """Every array as the host dict holds it."""
        out = {k: None for k in ARRAYS}
        for k, f in self.framed.items():
            a = f.view.detach().cpu().numpy()
            out[k] = a.view(np.uint32) if self.host0[k].dtype == np.uint32 else a
        return out

    def buffers(self):
        """Every framed buffer whole, frame included."""
        return {k: f.buf.detach().cpu().numpy().copy() for k, f in self.framed.items()}

    def intact(self):
        return [k for k, f in self.framed.items() if not f.intact()]


def same(got, ref):
    """The names of the arrays that differ (bit for bit where NaN is held: NaN equals NaN)."""
    bad = []
    for k in ARRAYS:
        a, b = got[k], ref[k]
        if (a is None) != (b is None):
            bad.append(k)
        elif a is not None and not (a.dtype == b.dtype and a.shape == b.shape and
                                    np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')):
            bad.append(k)
    return bad
