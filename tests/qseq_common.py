"""TEST INFRASTRUCTURE: QAgent on a Sequence with a Softmax or an EpsilonGreedy policy (agent/q.py,
interface/sequence.py, policy/softmax.py, policy/greedy.py of the reference) restated in plain NumPy,
the cases of tests/golden/qseq_traces.npz, and the helpers that run the same cases on the device.
Reads only oracle/philox.py.

Deliberate differences from the reference, both in the last bits of a probability only: the softmax
sum is the device's (csrc/qseq.hip), ``((e_0 + e_1) + e_2) + ...`` in action order where NumPy adds
eight values pairwise; and the device's ``exp`` is not NumPy's (the restatement uses ``np.exp``).  A
draw at least 1e-9 away from every edge of the normalised CDF selects the same action either way, and
then every action, reward, td, log entry and Q value is the reference's bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle.philox import STREAM_MEMORY, STREAM_POLICY, TapeRNG

STREAM_POLICY_TEST = 3
SEED = 0xC0BE1
MARGIN = 1e-9


# -- the policies -----------------------------------------------------------------------------------
def softmax_probs(v, beta, mask=None) -> np.ndarray:
    """policy/softmax.py:77-86 with the sum in action order."""
    v = np.asarray(v, dtype=np.float64)
    on = np.ones(len(v), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    e = np.zeros(len(v))
    e[on] = np.exp((v[on] - np.amax(v[on])) * beta)
    total = 0.0
    for x in e:
        total = total + x
    return np.where(on, e / total, 0.0)


def eps_greedy_probs(v, epsilon, mask=None) -> np.ndarray:
    """policy/greedy.py:77-86."""
    v = np.asarray(v, dtype=np.float64)
    on = np.ones(len(v), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    p = np.zeros(len(v))
    p[on] = epsilon / on.sum()
    ties = np.amax(v[on]) == v[on]
    p[on] += (1.0 - epsilon) * ties / np.sum(ties)
    return p


def cdf_of(p) -> np.ndarray:
    """cumsum(p) / cumsum(p)[-1], the cumulative sum in order (Generator.choice)."""
    run, cum = 0.0, []
    for a, x in enumerate(p):
        run = float(x) if a == 0 else run + float(x)
        cum.append(run)
    return np.array(cum) / cum[-1]


def choose(p, u) -> int:
    return int(np.searchsorted(cdf_of(p), u, side='right'))


class RefPolicy:
    def __init__(self, kind, par, rng):
        self.kind, self.par, self.rng = kind, float(par), rng
        self.margin = float('inf')

    def probs(self, v, mask=None):
        return (softmax_probs if self.kind == 'softmax' else eps_greedy_probs)(v, self.par, mask)

    def select_action(self, v):
        cdf = cdf_of(self.probs(v))
        u = self.rng.random()
        if len(cdf) > 1:
            self.margin = min(self.margin, float(np.abs(cdf[:-1] - u).min()))
        return int(np.searchsorted(cdf, u, side='right'))


# Known-answer rows of the stand-alone policy: name -> (values, mask or None, beta).  The fixture
# holds the reference's get_action_probs for each (tests/golden/gen_qseq.py).
KAT_ROWS = {
    'plain8': ([0.1, -0.3, 0.7, 0.0, 0.25, 0.7, -1.5, 0.4], None, 1.0),
    'equal8': ([0.5] * 8, None, 1.0),
    'equal3': ([-2.0] * 3, None, 5.0),
    'single': ([0.3], None, 1.0),
    'cold': ([0.1, -0.3, 0.7, 0.0, 0.25], None, 1e-3),
    'hot': ([0.1, -0.3, 0.7, 0.0, 0.25, 0.6999], None, 1e4),
    'hot_tie': ([0.7, -0.3, 0.7, 0.0], None, 1e4),
    'masked': ([0.1, 2.0, 0.7, 0.0, 0.25, 0.7, -1.5, 0.4], [1, 0, 1, 1, 0, 1, 1, 0], 5.0),
    'masked_one': ([0.1, 2.0, 0.7], [0, 0, 1], 1.0),
    'large': ([1e6, 1e6 - 1.0, -1e6, 0.0, 5e5, 1e6, 3.0], None, 0.25),
    'seven': ([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], None, 10.0),
}


# -- interface/sequence.py --------------------------------------------------------------------------
def keys_of(observations: dict) -> tuple:
    """(key of every observation name, the observation tuples in key order): observations of equal
    values share a key, the zero observation a trial ends in is key 0."""
    first = np.asarray(next(iter(observations.values())), dtype=np.float64)
    seen = {tuple([0.0] * first.size): 0}
    key = {}
    for name, o in observations.items():
        key[name] = seen.setdefault(tuple(np.asarray(o, dtype=np.float64).reshape(-1).tolist()),
                                    len(seen))
    return key, list(seen)


class RefSequence:
    def __init__(self, trials, observations, nb_actions, overwrite):
        self.trials, self.overwrite, self.nb_actions = trials, overwrite, nb_actions
        self.key, self.tuples = keys_of(observations)
        self.current_trial = self.current_step = 0

    def reset(self) -> int:
        self.current_step = 0
        return self.key[self.trials[self.current_trial][0]['observation']]

    def step(self, action):
        st = self.trials[self.current_trial][self.current_step]
        if type(st['reward']) is float:
            reward = st['reward']
        else:
            reward = float(st['reward'][st['action'] if self.overwrite else action])
        self.current_step += 1
        end = len(self.trials[self.current_trial]) == self.current_step
        ns = 0 if end else self.key[self.trials[self.current_trial][self.current_step]['observation']]
        self.current_trial += end
        return ns, reward, end


# -- agent/q.py -------------------------------------------------------------------------------------
def new_record() -> dict:
    return {'action': [], 'reward': [], 'end': [], 'td': [], 'Q': [], 'steps': [], 'trial_reward': []}


class RefQ:
    def __init__(self, n_keys, nb_actions, policy, policy_test, lr, gamma, rng):
        self.Q = np.zeros((n_keys, nb_actions))
        self.created, self.M = [], []
        self.policy, self.policy_test = policy, policy if policy_test is None else policy_test
        self.lr, self.gamma, self.rng = float(lr), float(gamma), rng

    def _meet(self, key) -> None:
        if key not in self.created:
            self.created.append(key)

    def update_q(self, e) -> float:
        td = e[2]
        td += self.gamma * e[4] * np.amax(self.Q[e[3]])
        td -= self.Q[e[0]][e[1]]
        self.Q[e[0]][e[1]] += self.lr * td
        return float(td)

    def run(self, env, trials, steps, learn, batch, rec) -> None:
        pol = self.policy if learn else self.policy_test
        for _ in range(trials):
            state, trial_reward = env.reset(), 0.0
            for step in range(steps):
                self._meet(state)
                action = pol.select_action(self.Q[state])
                ns, reward, end = env.step(action)
                td = 0.0
                if learn:
                    self._meet(ns)
                    e = (state, action, reward, ns, 1 - int(end))
                    self.M.append(e)
                    td = self.update_q(e)
                    for k in self.rng.integers(0, len(self.M), batch):
                        again = self.update_q(self.M[int(k)])
                        # (update_q writes 'td' into the experience it is given, and the step's
                        #  logs take the experience after the replay, agent/q.py:214-219: a replay
                        #  of the step's own experience leaves ITS td in the logs)
                        if int(k) == len(self.M) - 1:
                            td = again
                state = ns
                trial_reward += reward
                rec['action'].append(action)
                rec['reward'].append(reward)
                rec['end'].append(bool(end))
                rec['td'].append(td)
                if end:
                    break
            rec['Q'].append(self.Q.copy())
            rec['steps'].append(step)
            rec['trial_reward'].append(trial_reward)


def pack(rec: dict, n_keys: int, nb_actions: int) -> dict:
    return {'action': np.array(rec['action'], dtype=np.int64),
            'reward': np.array(rec['reward'], dtype=np.float64),
            'end': np.array(rec['end'], dtype=bool), 'td': np.array(rec['td'], dtype=np.float64),
            'Q': np.array(rec['Q'], dtype=np.float64).reshape(-1, n_keys, nb_actions),
            'steps': np.array(rec['steps'], dtype=np.int64),
            'trial_reward': np.array(rec['trial_reward'], dtype=np.float64)}


def restate(schedule, observations, nb_actions, overwrite, policy, policy_test, lr, gamma, sessions,
            inst, seed=SEED) -> dict:
    """One instance.  ``policy`` / ``policy_test``: (kind, parameter) or None; ``sessions``:
    [('train' | 'test', trials, steps, batch), ...]."""
    env = RefSequence(schedule, observations, nb_actions, overwrite)
    rngs = [TapeRNG(seed, inst, STREAM_POLICY), TapeRNG(seed, inst, STREAM_POLICY_TEST),
            TapeRNG(seed, inst, STREAM_MEMORY)]
    pol = RefPolicy(policy[0], policy[1], rngs[0])
    pol_t = None if policy_test is None else RefPolicy(policy_test[0], policy_test[1], rngs[1])
    ag = RefQ(len(env.tuples), nb_actions, pol, pol_t, lr, gamma, rngs[2])
    rec = new_record()
    for kind, trials, steps, batch in sessions:
        ag.run(env, trials, steps, kind == 'train', batch, rec)
    out = pack(rec, len(env.tuples), nb_actions)
    out['index'] = np.array([r.index for r in rngs], dtype=np.int64)
    out['len_M'] = np.int64(len(ag.M))
    out['created'] = np.array(ag.created, dtype=np.int64)
    out['M'] = np.array([[e[0], e[1], e[3], e[4]] for e in ag.M], dtype=np.int64).reshape(-1, 4)
    out['M_reward'] = np.array([e[2] for e in ag.M], dtype=np.float64)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['margin'] = np.float64(min(p.margin for p in (pol, pol_t) if p is not None))
    return out


EXACT = ('action', 'reward', 'end', 'td', 'Q', 'steps', 'trial_reward', 'index', 'len_M', 'created',
         'M', 'M_reward', 'position')


def assert_same_record(out, ref, prefix='', what='', keys=EXACT) -> None:
    for k in keys:
        if k not in out or (prefix + k) not in ref:
            continue
        a, b = np.asarray(out[k]), np.asarray(ref[prefix + k])
        assert a.shape == b.shape, '%s %s: shapes %s and %s' % (what, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[0]
            raise AssertionError('%s %s differs first at %s: %r != %r' % (
                what, k, bad.tolist(), a[tuple(bad)], b[tuple(bad)]))


# -- the recorded cases -----------------------------------------------------------------------------
def _step(obs, reward, action=None):
    return {'observation': obs, 'reward': reward, 'action': action}


def demo_design(reps, nb_actions=8):
    """The grid-search demo: four one-hot stimuli, one of the arms 0, 2, 4, 6 pays."""
    seq = []
    for _ in range(reps):
        for k, name in enumerate('ABCD'):
            seq.append([_step(name, np.eye(nb_actions)[(2 * k) % nb_actions])])
    return seq, {n: np.eye(4)[i] for i, n in enumerate('ABCD')}


def _demo12():
    return demo_design(12)


def _demo3():
    return demo_design(8, 3)


def _multistep():
    obs = {n: np.eye(3)[i] for i, n in enumerate('ABC')}
    two = [_step('A', 0.0), _step('B', np.array([1.0, 0.0, 0.5]))]
    three = [_step('A', np.array([0.0, 0.25, 0.0])), _step('B', 0.5), _step('C', np.array([0.0, 1.0, 1.0]))]
    one = [_step('C', 1.0)]
    return [two, one, three, two, three, one, one, three] * 3, obs


def _overwrite():
    obs = {n: np.eye(2)[i] for i, n in enumerate('AB')}
    seq = []
    for _ in range(10):
        seq += [[_step('A', np.array([0.0, 1.0]), 1)], [_step('B', np.array([0.25, 1.0]), 0)],
                [_step('A', 0.5, None), _step('B', np.array([1.0, 0.0]), 0)]]
    return seq, obs


def _one_action():
    obs = {n: np.eye(2)[i] for i, n in enumerate('AB')}
    return [[_step('A', np.array([1.0]))], [_step('B', 0.5), _step('A', np.array([0.25]))]] * 6, obs


def _ties():
    """Rewards that repeat inside a row: with Q = 0 at the start and a learning rate of 1 the
    values of several actions are exactly equal, at the maximum of their row too."""
    obs = {n: np.eye(2)[i] for i, n in enumerate('AB')}
    seq = []
    for _ in range(15):
        seq += [[_step('A', np.array([1.0, 1.0, 0.0, 1.0]))],
                [_step('B', np.array([0.5, 0.0, 0.5, 0.5])), _step('A', np.array([0.0, 1.0, 1.0, 0.0]))]]
    return seq, obs


def _shared_keys():
    """'A' and 'A2' hold the same values, 'Z' is all zeros — the key of a trial's end."""
    obs = {'A': np.array([1.0, 0.0, 0.5]), 'B': np.array([0.0, 1.0, 0.0]),
           'A2': np.array([1.0, 0.0, 0.5]), 'Z': np.zeros(3)}
    seq = []
    for _ in range(8):
        seq += [[_step('A', np.array([1.0, 0.0, 0.0])), _step('Z', 0.25)],
                [_step('A2', np.array([0.0, 0.0, 1.0]))],
                [_step('Z', np.array([0.0, 0.5, 0.0])), _step('B', 0.0), _step('A2', 1.0)]]
    return seq, obs


def _case(design, nb_actions, sessions, inst, policy=('softmax', 1.0), policy_test=None, lr=0.9,
          gamma=0.8, overwrite=False):
    return dict(design=design, nb_actions=nb_actions, sessions=sessions, inst=inst, policy=policy,
                policy_test=policy_test, lr=lr, gamma=gamma, overwrite=overwrite)


# (instance numbers: those for which the real reference keeps every draw 1e-9 away from every edge
#  of its CDF — tests/golden/gen_qseq.py asserts it)
CASES = {
    'demo12': _case(_demo12, 8, [('train', 48, 100, 32)], 0),
    'multistep_cut': _case(_multistep, 3, [('train', 8, 2, 4), ('train', 10, 5, 9)], 1,
                           policy=('softmax', 5.0), lr=0.4),
    'overwrite': _case(_overwrite, 2, [('train', 30, 10, 7)], 2, policy=('softmax', 0.25),
                       overwrite=True, lr=0.5),
    'one_action': _case(_one_action, 1, [('train', 12, 5, 3)], 3),
    'three_actions': _case(_demo3, 3, [('train', 32, 100, 8)], 4, policy=('softmax', 10.0)),
    'b0_then_b5': _case(_demo3, 3, [('train', 10, 10, 0), ('train', 14, 10, 5)], 5,
                        policy=('softmax', 1.0), lr=0.3),
    'eps_ties': _case(_ties, 4, [('train', 30, 10, 6)], 6, policy=('eps', 0.3), lr=1.0, gamma=0.5),
    'shared_keys': _case(_shared_keys, 3, [('train', 12, 2, 5), ('train', 12, 3, 5)], 7,
                         policy=('softmax', 5.0)),
    'train_test': _case(_multistep, 3, [('train', 10, 5, 8), ('test', 6, 5, 0), ('train', 8, 2, 8)],
                        8, policy=('softmax', 1.0), policy_test=('softmax', 5.0), lr=0.7),
}


def restate_case(name: str, **over) -> dict:
    c = dict(CASES[name])
    c.update(over)
    schedule, obs = c['design']()
    return restate(schedule, obs, c['nb_actions'], c['overwrite'], c['policy'], c['policy_test'],
                   c['lr'], c['gamma'], c['sessions'], c['inst'])


# -- the launch structs, for calls that must be refused before any launch ---------------------------
def fake_structs(n=2, n_actions=3, n_keys=4, learn=True):
    """A cobel_seq_t and a cobel_qseq_run_t that pass every check; the pointers are aligned numbers
    nothing dereferences on the host."""
    from cobel_amd import _lib
    seq, run = _lib.Seq(), _lib.QSeqRun()
    for k, (name, _) in enumerate(_lib.Seq._fields_[:9]):
        setattr(seq, name, 0x10000 + 0x100 * k)
    seq.n, seq.dim, seq.n_obs, seq.n_actions = n, 4, n_keys, n_actions
    seq.n_schedules, seq.n_trials, seq.n_steps, seq.overwrite = 1, 3, 5, 0
    for k, (name, _) in enumerate(_lib.QSeqRun._fields_[:17]):
        setattr(run, name, 0x20000 + 0x100 * k)
    run.n, run.n_keys, run.n_actions, run.log_cap = n, n_keys, n_actions, 16
    run.trial_cap, run.trace_cap, run.par_rows, run.policy = 8, 4, 1, _lib.QSEQ_POLICY_SOFTMAX
    run.batch_size, run.flags = 4, _lib.F_LEARN if learn else 0
    run.pol_stream, run.trial_first, run.trials = STREAM_POLICY, 0, 0
    run.steps_per_trial, run.step_budget, run.seed = 5, 0, SEED
    return seq, run


def run_rc(seq, run) -> int:
    from cobel_amd import _lib
    return _lib.lib().cobel_qseq_run(C.byref(seq), C.byref(run), None)


# -- the same on the device -------------------------------------------------------------------------
def device_policy(spec, value=None):
    from cobel_amd.policy import EpsilonGreedy, Softmax
    if spec is None:
        return None
    par = spec[1] if value is None else value
    return Softmax(par) if spec[0] == 'softmax' else EpsilonGreedy(par)


def device_run(schedules, observations, nb_actions, overwrite, policy, policy_test, lr, gamma,
               sessions, n_envs=1, instance_ids=None, instance_base=0, schedule_of=None,
               callbacks=None, record=4096, seed=SEED, policy_value=None):
    """Build Sequence and agent, run the sessions; returns (agent, interface)."""
    from cobel_amd.agent import QAgent
    from cobel_amd.interface import Sequence
    from cobel_amd.spaces import Box
    shape = np.asarray(next(iter(observations.values()))).shape
    env = Sequence(schedules, observations, Box(0.0, 1.0, shape), nb_actions, overwrite,
                   n_envs=n_envs, seed=seed, schedule_of=schedule_of, instance_base=instance_base,
                   instance_ids=instance_ids)
    ag = QAgent(env.observation_space, env.action_space, device_policy(policy, policy_value),
                device_policy(policy_test), lr, gamma, callbacks)
    ag.record_steps = record
    for kind, trials, steps, batch in sessions:
        if kind == 'train':
            ag.train(env, trials, steps, batch)
        else:
            ag.test(env, trials, steps)
    return ag, env


def device_case(name: str, callbacks=None, **kw):
    c = CASES[name]
    schedule, obs = c['design']()
    return device_run(schedule, obs, c['nb_actions'], c['overwrite'], c['policy'], c['policy_test'],
                      c['lr'], c['gamma'], c['sessions'], callbacks=callbacks,
                      instance_base=c['inst'], **kw)


def device_record(ag, env, i: int = 0) -> dict:
    """What ``restate`` returns, read back from instance i (Q after every trial excepted)."""
    h = ag._seq
    rows = ag.recorded_steps(i)
    T = ag.current_trial
    out = {'action': rows[:, 1].astype(np.int64), 'reward': rows[:, 2].copy(),
           'end': rows[:, 4] == 0, 'td': rows[:, 5].copy(),
           'steps': ag.trial_steps_trace[i, :T].cpu().numpy().astype(np.int64),
           'trial_reward': ag.trial_reward_trace[i, :T].cpu().numpy()}
    test_ctr = 0 if ag.policy_test is ag.policy or ag.policy_test.counter is None \
        else int(ag.policy_test.counter[i].item())
    out['index'] = np.array([int(ag.policy.counter[i].item()), test_ctr,
                             int(h._mem_ctr[i].item())], dtype=np.int64)
    n = int(h._log_len[i].item())
    out['len_M'] = np.int64(n)
    if h._log is not None:
        raw = h._log[i, :n].cpu().numpy()
        m = raw[:, 1]
        out['M'] = np.stack([m & 0xFF, (m >> 16) & 0xFF, (m >> 8) & 0xFF, (m >> 24) & 1],
                            axis=1).astype(np.int64).reshape(-1, 4)
        out['M_reward'] = raw[:, 0].copy().view(np.float64)
    out['position'] = np.array([int(env._trial[i].item()), int(env._step[i].item())], dtype=np.int64)
    assert out['position'][0] == env._h_trial[i] and out['position'][1] == env._h_step[i], \
        'the host mirror of the position left the device'
    out['Q_final'] = h._q[i].cpu().numpy()
    return out


def random_design(rng, n_schedules, n_trials, max_len, nb_actions, n_obs):
    """Schedules of the same number of trials and differing trial lengths over shared one-hot
    observations, float rewards mixed with array rewards."""
    obs = {'o%d' % k: np.eye(n_obs)[k] for k in range(n_obs)}
    schedules = []
    for _ in range(n_schedules):
        sched = []
        for _ in range(n_trials):
            trial = []
            for _ in range(int(rng.integers(1, max_len + 1))):
                name = 'o%d' % int(rng.integers(n_obs))
                if rng.random() < 0.6:
                    trial.append(_step(name, np.round(rng.random(nb_actions) * 4) / 4))
                else:
                    trial.append(_step(name, float(np.round(rng.random() * 4) / 4)))
            sched.append(trial)
        schedules.append(sched)
    return schedules, obs


def compare_instances(ag, env, schedules, obs, nb_actions, policy, lr, gamma, sessions, ids,
                      policy_value=None, what='') -> None:
    """Every instance of a device run against its own restatement with np.array_equal; instances
    whose restatement comes within MARGIN of a CDF edge would be no evidence either way, so the
    caller's seeds are chosen to have none (asserted)."""
    N = env.n_envs
    lr, gamma = np.broadcast_to(lr, (N,)), np.broadcast_to(gamma, (N,))
    par = np.broadcast_to(policy[1] if policy_value is None else policy_value, (N,))
    for i in range(N):
        ref = restate(schedules[int(env.schedule_of[i])], obs, nb_actions, False,
                      (policy[0], float(par[i])), None, float(lr[i]), float(gamma[i]), sessions,
                      int(ids[i]), seed=env.seed)
        assert ref['margin'] > MARGIN, '%s instance %d: margin %g' % (what, i, ref['margin'])
        out = device_record(ag, env, i)
        assert_same_record(out, ref, what='%s instance %d' % (what, i))
        assert np.array_equal(out['Q_final'], ref['Q'][-1]), '%s instance %d: Q' % (what, i)
