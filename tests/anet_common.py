"""TEST INFRASTRUCTURE: the AssociativeNetwork agent of the reference (agent/anet.py) and its
EpsilonGreedy policy (policy/greedy.py) restated in plain Python floats, on the ``RefSequence`` of
tests/rw_common.py; the cases of tests/golden/anet_traces.npz; and the helpers that run the same
cases on the device.

One deliberate difference from the reference: ``state @ W[:, a]`` is not BLAS's sum but the device's
(csrc/anet.hip, ``tree_dot`` of rw_common.py).  All cases but the dense one have observations of at
most two non-zero components, each a power of two: the products are exact, every summation order
gives the same sum, and those cases reproduce the reference exactly.

The agent's generator is a tape on STREAM_AGENT whose vector draw ``random(k)`` takes k consecutive
indices (``NoiseTape``); the policy's is the usual tape on STREAM_POLICY.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rw_common import SEED, STREAM_POLICY_TEST, RefSequence, _step, tree_dot  # noqa: E402,F401

from oracle.philox import STREAM_AGENT, STREAM_POLICY, TapeRNG, draw_double  # noqa: E402

KEYS = ('excitatory', 'inhibitory')


class NoiseTape(TapeRNG):
    """``random(k)``: the k doubles at the indices index .. index + k - 1, as the kernels draw the
    noise of the k outputs."""

    def random(self, size=None):
        if size is None:
            return super().random()
        k = int(size)
        u = draw_double(self.seed, self.instance, self.index + np.arange(k), self.double_sub,
                        self.stream)
        self.index += k
        self.log.append(u.copy())
        return u


# -- policy/greedy.py -------------------------------------------------------------------------------
class RefEpsilonGreedy:
    """greedy.py:40-88 with the Generator.choice draw written out; ``margin`` is the smallest
    distance of a draw from a threshold of the normalised cumulative probabilities."""

    def __init__(self, epsilon, rng):
        self.epsilon, self.rng = float(epsilon), rng
        self.margin = float('inf')

    def select_action(self, q) -> int:
        n, m = len(q), max(q)
        ties = [1.0 if v == m else 0.0 for v in q]
        nt = sum(ties)
        cdf, run = [], 0.0
        for k, t in enumerate(ties):
            p = self.epsilon / n + ((1.0 - self.epsilon) * t) / nt
            run = p if k == 0 else run + p
            cdf.append(run)
        u = self.rng.random()
        thresholds = [c / cdf[-1] for c in cdf[:-1]]
        self.margin = min([self.margin] + [abs(u - c) for c in thresholds])
        return sum(1 for c in thresholds if c <= u)


# -- agent/anet.py ----------------------------------------------------------------------------------
def new_record() -> dict:
    return {'q': [], 'action': [], 'reward': [], 'end': [], 'We': [], 'Wi': [], 'steps': [],
            'trial_reward': [], 'mid_predict': []}


def _matrix(value, dim, na) -> list:
    v = np.broadcast_to(np.asarray(value, dtype=np.float64), (dim, na))
    return [[float(x) for x in row] for row in v]


class RefANet:
    def __init__(self, dim, n_actions, policy, policy_test=None, saturation=20.0, learning_rate=0.01,
                 noise=1.0, linear_update=False, rng=None, rec=None):
        self.dim, self.na = dim, n_actions - 1
        self.policy = policy
        self.policy_test = policy if policy_test is None else policy_test
        self.rng = rng
        self.weights = {k: _matrix(0.0, dim, self.na) for k in KEYS}
        self.saturation = {k: _matrix(saturation[k] if type(saturation) is dict else saturation,
                                      dim, self.na) for k in KEYS}
        self.learning_rate = {k: _matrix(learning_rate[k] if type(learning_rate) is dict
                                         else learning_rate, dim, self.na) for k in KEYS}
        self.linear_update, self.noise_amplitude = linear_update, float(noise)
        self.alpha, self.d_alpha = 1.0, 0.0
        self.current_trial = 0
        self.rec = new_record() if rec is None else rec
        self.gap = float('inf')      # smallest difference of the two largest outputs of a step

    def retrieve_q(self, x) -> list:
        u = self.rng.random(self.na)
        q = []
        for a in range(self.na):
            e = tree_dot([row[a] for row in self.weights['excitatory']], x)
            h = tree_dot([row[a] for row in self.weights['inhibitory']], x)
            q.append((e - h) + self.noise_amplitude * float(u[a]))
        return q

    def update_q(self, experience: dict) -> None:
        a = int(experience['action'])
        if not 0 <= a < self.na:
            return
        k = 'excitatory' if experience['reward'] > 0 else 'inhibitory'
        W, sat, lr = self.weights[k], self.saturation[k], self.learning_rate[k]
        for j, s in enumerate(experience['state']):
            if s != 0:
                delta = 1.0 if self.linear_update else self.alpha * (sat[j][a] - W[j][a])
                W[j][a] = W[j][a] + lr[j][a] * delta

    def rescale_weights(self, factor: dict) -> None:
        for k in KEYS:
            self.weights[k] = [[w * factor[k] for w in row] for row in self.weights[k]]

    def predict_on_batch(self, batch):
        return np.array([self.retrieve_q([float(v) for v in row]) for row in np.asarray(batch)])

    def _run(self, env, trials, steps, learn):
        rec, pol = self.rec, self.policy      # (agent/anet.py:272: test() selects with `policy` too)
        for _ in range(trials):
            trial_reward = 0.0
            state, _ = env.reset()
            for step in range(steps):
                q = self.retrieve_q(state)
                if len(q) > 1:
                    top = sorted(q)[-2:]
                    self.gap = min(self.gap, top[1] - top[0])
                action = pol.select_action(q)
                ns, reward, end, _, _ = env.step(action)
                if learn:
                    self.update_q({'state': state, 'action': action, 'reward': reward})
                rec['q'].append(q)
                rec['action'].append(action)
                rec['reward'].append(reward)
                rec['end'].append(bool(end))
                state = ns
                trial_reward += reward
                if end:
                    break
            self.current_trial += 1
            rec['We'].append([list(r) for r in self.weights['excitatory']])
            rec['Wi'].append([list(r) for r in self.weights['inhibitory']])
            rec['steps'].append(step)
            rec['trial_reward'].append(trial_reward)

    def train(self, env, trials, steps=32):
        self._run(env, trials, steps, True)

    def test(self, env, trials, steps=32):
        self._run(env, trials, steps, False)


def run_sessions(ag, env, sessions, rec) -> None:
    """The same for the restatement, the reference and the device.  A session is ('train' | 'test',
    trials, steps), ('rescale', factors), ('alpha', value) or ('predict', batch)."""
    for s in sessions:
        if s[0] in ('train', 'test'):
            getattr(ag, s[0])(env, s[1], s[2])
        elif s[0] == 'rescale':
            ag.rescale_weights(s[1])
        elif s[0] == 'alpha':
            ag.alpha = s[1]
        else:
            assert s[0] == 'predict'
            p = ag.predict_on_batch(np.asarray(s[1], dtype=np.float64))
            rec['mid_predict'].append(np.asarray(p.cpu() if hasattr(p, 'cpu') else p))


def pack(rec: dict, dim: int, na: int) -> dict:
    return {'q': np.array(rec['q'], dtype=np.float64).reshape(-1, na),
            'action': np.array(rec['action'], dtype=np.int64),
            'reward': np.array(rec['reward'], dtype=np.float64),
            'end': np.array(rec['end'], dtype=bool),
            'We': np.array(rec['We'], dtype=np.float64).reshape(-1, dim, na),
            'Wi': np.array(rec['Wi'], dtype=np.float64).reshape(-1, dim, na),
            'steps': np.array(rec['steps'], dtype=np.int64),
            'trial_reward': np.array(rec['trial_reward'], dtype=np.float64),
            'mid_predict': np.array(rec['mid_predict'], dtype=np.float64).reshape(-1, dim, na)}


def probe_of(dim: int) -> np.ndarray:
    return np.eye(dim)


def restate(schedule, observations, seq_actions, overwrite, n_actions, eps, eps_test, agent_kw,
            sessions, inst, seed=SEED, probe=None) -> dict:
    """One instance.  ``agent_kw``: saturation, learning_rate, noise, linear_update."""
    env = RefSequence(schedule, observations, seq_actions, overwrite)
    # (the third generator is policy_test's: it must never be drawn from, agent/anet.py:272)
    rngs = [NoiseTape(seed, inst, STREAM_AGENT), TapeRNG(seed, inst, STREAM_POLICY),
            TapeRNG(seed, inst, STREAM_POLICY_TEST)]
    pol = RefEpsilonGreedy(eps, rngs[1])
    pol_t = None if eps_test is None else RefEpsilonGreedy(eps_test, rngs[2])
    ag = RefANet(env.dim, n_actions, pol, pol_t, rng=rngs[0], **agent_kw)
    run_sessions(ag, env, sessions, ag.rec)
    out = pack(ag.rec, env.dim, n_actions - 1)
    out['index'] = np.array([r.index for r in rngs], dtype=np.int64)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    if probe is not None:
        out['predict'] = ag.predict_on_batch(probe)
    out['margin'] = np.float64(pol.margin)
    out['gap'] = np.float64(ag.gap)
    return out


EXACT = ('q', 'action', 'reward', 'end', 'We', 'Wi', 'steps', 'trial_reward', 'mid_predict', 'index',
         'position', 'predict')
DISCRETE = ('action', 'reward', 'end', 'steps', 'trial_reward', 'index', 'position')


def assert_same_record(out, ref, prefix='', what='', keys=EXACT) -> None:
    """np.array_equal on every key both sides hold (-0.0 equals +0.0: the sign of a zero does depend
    on the summation order)."""
    for k in keys:
        if k not in out or (prefix + k) not in ref:
            continue
        a, b = np.asarray(out[k]), np.asarray(ref[prefix + k])
        assert a.shape == b.shape, '%s %s: shapes %s and %s' % (what, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[0]
            raise AssertionError('%s %s differs first at %s: %r != %r' % (
                what, k, bad.tolist(), a[tuple(bad)], b[tuple(bad)]))


# -- the recorded cases ---------------------------------------------------------------------------
def _unit():
    """unit_tests/test_anet.py: alternating A/B trials, the reward an array indexed by the action
    (one entry per action of the Sequence, which has three)."""
    seq = []
    for _ in range(10):
        seq.append([_step('A', np.array([1.0, 0.0, 0.0]))])
        seq.append([_step('B', np.array([0.0, 1.0, 0.0]))])
    return seq, {'A': np.array([1.0, 0.0]), 'B': np.array([0.0, 1.0])}, 3


def _single_output():
    obs = {n: np.eye(3)[i] for i, n in enumerate('ABC')}
    seq = []
    for _ in range(8):
        seq += [[_step('A', 1.0)], [_step('B', -0.5)], [_step('C', 0.0)]]
    return seq, obs, 1


def _eight_outputs():
    obs = {n: np.eye(5)[i] for i, n in enumerate('ABCDE')}
    obs['AC'] = np.array([1.0, 0.0, 0.5, 0.0, 0.0])
    seq = []
    for r in range(5):
        for k, name in enumerate(('A', 'B', 'C', 'D', 'E', 'AC')):
            reward = np.zeros(8)
            reward[(3 * k + 1) % 8] = 1.0
            reward[(3 * k + 2) % 8] = -1.0
            seq.append([_step(name, reward)])
    return seq, obs, 8


def _edge(dim):
    def design():
        obs = {}
        for k, (i, j) in enumerate(((0, dim - 1), (1, dim // 2), (dim - 2, dim - 1), (dim // 2, 2))):
            o = np.zeros(dim)
            o[i], o[j] = 1.0, 0.25
            obs['o%d' % k] = o
        seq = []
        for r in range(6):
            for k in range(4):
                reward = np.zeros(3)
                reward[k % 3] = 1.0
                seq.append([_step('o%d' % k, reward)])
        return seq, obs, 3
    return design


def _multistep():
    """Trials of one to three steps; float rewards that are zero, negative and positive, and array
    rewards under overwrite=True with the step's own action."""
    obs = {n: np.eye(3)[i] for i, n in enumerate('ABC')}
    two = [_step('A', 0.0), _step('B', np.array([1.0, -1.0]), 1)]
    three = [_step('A', -0.5), _step('B', 0.5), _step('C', np.array([0.25, 1.0]), 0)]
    one = [_step('C', 1.0)]
    return [two, one, three, two, three, one, one, three] * 3, obs, 2


def _ties():
    """noise = 0 and zero weights: all outputs tie on the first steps; an output that was punished
    leaves the other two tied."""
    obs = {'A': np.array([1.0, 0.0]), 'B': np.array([0.0, 1.0])}
    seq = []
    for _ in range(12):
        seq += [[_step('A', np.array([0.0, 0.0, 1.0]))], [_step('B', np.array([0.0, 1.0, 0.0]))]]
    return seq, obs, 3


def _mask():
    obs = {'A': np.array([0.5, 0.0, 2.0, 0.0]), 'B': np.array([0.0, 2.0, 0.0, 0.5]),
           'C': np.array([0.0, 0.0, 0.0, 2.0])}
    seq = []
    for _ in range(8):
        seq += [[_step('A', np.array([1.0, 0.0]))], [_step('B', np.array([0.0, 1.0]))],
                [_step('C', np.array([-1.0, 1.0]))]]
    return seq, obs, 2


def _dense():
    rng = np.random.default_rng(21)
    obs = {'o%d' % k: rng.random(6) for k in range(5)}
    order = rng.integers(0, 5, 60)
    return [[_step('o%d' % k, rng.random(3) - 0.4)] for k in order], obs, 3


def _case(design, n_actions, sessions, inst, eps=0.1, eps_test=None, overwrite=False, dense=False,
          **agent_kw):
    return dict(design=design, n_actions=n_actions, sessions=sessions, inst=inst, eps=eps,
                eps_test=eps_test, overwrite=overwrite, dense=dense, agent_kw=agent_kw)


_UNIT = [('train', 10, 10), ('test', 10, 10)]
# (every entry distinct, so that a transposed or swapped index shows)
_DISTINCT = {'excitatory': np.array([[20.0, 12.0], [6.0, 30.0]]),
             'inhibitory': np.array([[9.0, 17.0], [25.0, 4.0]])}
_RATES = {'excitatory': np.array([[0.01, 0.04], [0.07, 0.02]]),
          'inhibitory': np.array([[0.05, 0.03], [0.015, 0.06]])}

CASES = {
    'unit': _case(_unit, 3, _UNIT, 0, eps_test=0.0),
    'unit_linear': _case(_unit, 3, _UNIT, 1, eps_test=0.0, linear_update=True),
    'unit_saturation': _case(_unit, 3, _UNIT, 2, eps_test=0.0, saturation=_DISTINCT),
    'unit_rates': _case(_unit, 3, _UNIT, 3, eps_test=0.0, learning_rate=_RATES),
    'single_output': _case(_single_output, 2, [('train', 18, 10), ('test', 6, 10)], 4, eps=0.2,
                           learning_rate=0.1),
    'eight_outputs': _case(_eight_outputs, 9, [('train', 24, 10), ('test', 6, 10)], 5, eps=0.3,
                           learning_rate=0.05, noise=0.5),
    'edge33': _case(_edge(33), 4, [('train', 18, 10), ('test', 6, 10)], 6, learning_rate=0.05),
    'edge64': _case(_edge(64), 4, [('train', 18, 10), ('test', 6, 10)], 7, learning_rate=0.05),
    'multistep_cut': _case(_multistep, 3, [('train', 6, 2), ('train', 12, 5), ('test', 3, 2),
                                           ('train', 6, 3)], 8, eps=0.2, overwrite=True,
                           learning_rate=0.1),
    'ties': _case(_ties, 4, [('train', 18, 10), ('test', 6, 10)], 9, noise=0.0, learning_rate=0.1),
    'mask_nonzero': _case(_mask, 3, [('train', 18, 10), ('test', 6, 10)], 10, learning_rate=0.1,
                          saturation=5.0),
    'between_sessions': _case(_unit, 3, [('train', 6, 10),
                                         ('rescale', {'excitatory': 0.5, 'inhibitory': 1.5}),
                                         ('alpha', 0.5), ('predict', np.array([[0.0, 1.0], [1.0, 0.0]])),
                                         ('train', 8, 10), ('test', 6, 10)], 11, learning_rate=0.1),
    'dense6': _case(_dense, 4, [('train', 40, 10), ('test', 20, 10)], 12, dense=True,
                    learning_rate=0.05, noise=0.5),
}
# The dense case against the reference's BLAS sums: the largest absolute differences the generator
# measured (tests/golden/gen_anet.py prints them), restatement against reference, and the bounds —
# the next power of two above each.  Only the outputs handed to the policy see the sums: an update
# reads the action, the reward and the weight itself, and the rows of np.eye(D) have one non-zero
# component, so as long as the actions agree the weights and the final predictions are the
# reference's exactly (measured 0, bound 0).
DENSE_MEASURED = {'W': 0.0, 'q': 1.0658141036401503e-14, 'predict': 0.0}
DENSE_BOUND = {'W': 0.0, 'q': 2.0 ** -46, 'predict': 0.0}


def restate_case(name: str) -> dict:
    c = CASES[name]
    schedule, obs, seq_actions = c['design']()
    dim = np.asarray(next(iter(obs.values()))).size
    return restate(schedule, obs, seq_actions, c['overwrite'], c['n_actions'], c['eps'],
                   c['eps_test'], c['agent_kw'], c['sessions'], c['inst'], probe=probe_of(dim))


_RESTATED = {}


def restated(name: str) -> dict:
    """``restate_case`` computed once and shared; not to be written to."""
    if name not in _RESTATED:
        _RESTATED[name] = restate_case(name)
    return _RESTATED[name]


# -- the same on the device -------------------------------------------------------------------------
def device_run(schedules, observations, seq_actions, overwrite, n_actions, eps, eps_test, agent_kw,
               sessions, n_envs=1, instance_ids=None, instance_base=0, schedule_of=None,
               callbacks=None, record=4096, seed=SEED, rec=None):
    """Build Sequence and agent, run the sessions; returns (agent, interface)."""
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.interface import Sequence
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    shape = np.asarray(next(iter(observations.values()))).shape
    env = Sequence(schedules, observations, Box(0.0, 1.0, shape), seq_actions, overwrite,
                   n_envs=n_envs, seed=seed, schedule_of=schedule_of, instance_base=instance_base,
                   instance_ids=instance_ids)
    ag = AssociativeNetwork(env.observation_space, Discrete(n_actions), EpsilonGreedy(eps),
                            None if eps_test is None else EpsilonGreedy(eps_test),
                            custom_callbacks=callbacks, **agent_kw)
    ag.record_steps = record
    run_sessions(ag, env, sessions, new_record() if rec is None else rec)
    return ag, env


def device_case(name, **kw):
    c = CASES[name]
    schedule, obs, seq_actions = c['design']()
    return device_run(schedule, obs, seq_actions, c['overwrite'], c['n_actions'], c['eps'],
                      c['eps_test'], c['agent_kw'], c['sessions'], **kw)


def device_record(ag, env, i: int = 0, probe=None) -> dict:
    """What ``restate`` returns, read back from instance i (the matrices after every trial and the
    predictions between sessions excepted)."""
    rows = ag.recorded_steps(i)
    T = ag.current_trial
    out = {'q': rows[:, 3:].copy(), 'action': rows[:, 0].astype(np.int64),
           'reward': rows[:, 1].copy(), 'end': rows[:, 2] != 0,
           'steps': ag.trial_steps_trace[i, :T].cpu().numpy().astype(np.int64),
           'trial_reward': ag.trial_reward_trace[i, :T].cpu().numpy()}
    # (policy_test is stored only — agent/anet.py:272 — so its stream is never drawn from)
    assert ag.policy_test is ag.policy or ag.policy_test.counter is None
    out['index'] = np.array([int(ag._agent_ctr[i].item()), int(ag.policy.counter[i].item()), 0],
                            dtype=np.int64)
    out['position'] = np.array([int(env._trial[i].item()), int(env._step[i].item())], dtype=np.int64)
    assert out['position'][0] == env._h_trial[i] and out['position'][1] == env._h_step[i], \
        'the host mirror of the position left the device: %s vs (%d, %d)' % (
            out['position'], env._h_trial[i], env._h_step[i])
    out['We_final'] = ag.weights['excitatory'][i].cpu().numpy()
    out['Wi_final'] = ag.weights['inhibitory'][i].cpu().numpy()
    if probe is not None:
        p = ag.predict_on_batch(np.asarray(probe, dtype=np.float64))
        out['predict'] = p if ag.n_envs == 1 else p[i].cpu().numpy()
    return out
