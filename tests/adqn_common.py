"""TEST INFRASTRUCTURE: the ADQN agent of the reference (agent/adqn.py) and its memory
(memory/adqn.py) restated in NumPy, on the ``RefSequence`` of tests/rw_common.py and the float64
network of tests/mlp_common.py; the cases of tests/golden/adqn_traces.npz; and the helpers that run
the same cases on the device.

Two memories.  ``PlainMemory`` says memory/adqn.py in NumPy's own words: ``np.append``, ``*=``,
``np.sum`` and ``Generator.choice`` through a tape.  ``RefMemory`` is the device's
(csrc/adqn.hip): the same store, and a draw whose cumulative distribution is formed in the
device's summation order (``device_cdf``), bit for bit — 64 consecutive chunks of
ceil(count / 64) entries, sequential sums inside a chunk, the balanced tree over the chunk sums
for ``prob_sum``, a Hillis-Steele scan over the chunk totals of the probabilities, and the index
as the number of entries whose normalised cdf the draw has passed.  The two agree on the drawn
indices as long as no draw lies close to a cdf boundary (``margin``).

The memory's generator is a tape on STREAM_ADQN_MEMORY: ``choice(n, p=probs, size=B)`` is ONE call,
B doubles at sub = 0 .. B - 1 of one draw index.
"""
from __future__ import annotations

import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402
from rw_common import SEED, RefSequence, _step  # noqa: E402,F401

from oracle.philox import TapeRNG  # noqa: E402

STREAM_ADQN_MEMORY = 7
HYPER = {'lr': 1e-3, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-8, 'weight_decay': 0.0, 'tau': 0.0}
# Values, final weights and final predictions of the float64 restatement against the reference's
# torch run, largest absolute difference over all golden cases as tests/golden/gen_adqn.py printed
# it, and the bound: 16 times that (Adam's division by sqrt(v) + eps amplifies last-bit differences
# in the first steps; BLAS and torch contract differently).
VALUE_MEASURED = 2.2204460492503131e-16
VALUE_BOUND = 16 * VALUE_MEASURED


class ChoiceTape(TapeRNG):
    """The tape with Generator.choice's ``replace`` keyword; ``margin`` is the smallest distance of
    a draw from a cdf boundary it was compared with (the last one, 1.0, excepted)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.margin = float('inf')
        self.drawn = []

    def choice(self, a, size=None, p=None, replace=True):
        assert replace and p is not None
        at = self.index
        out = super().choice(a, size, p)
        cdf = np.cumsum(np.asarray(p, dtype=np.float64))
        cdf /= cdf[-1]
        u = np.atleast_1d(self.log[-1])
        assert self.index == at + 1
        if len(cdf) > 1:
            self.margin = min(self.margin, float(np.abs(cdf[:-1, None] - u[None, :]).min()))
        self.drawn.append(np.array(out, dtype=np.int64))
        return out


# -- memory/adqn.py -------------------------------------------------------------------------------
class PlainMemory:
    """memory/adqn.py:77-164 for Box observations, statement by statement."""

    def __init__(self, dim, decay=1.0, rpe=True, rng=None):
        self.rng = rng
        self.states = np.zeros((0, dim))
        self.reinforcements = np.array([], dtype=float)
        self.errors = np.array([], dtype=float)
        self.priorities = np.array([], dtype=float)
        self.decay, self.rpe = decay, rpe

    def store(self, state, action, reward):
        self.states = np.append(self.states, np.asarray(state, dtype=np.float64)[np.newaxis], axis=0)
        self.reinforcements = np.append(self.reinforcements, reward)
        self.errors = np.append(self.errors, action - reward)
        self.priorities *= self.decay
        self.priorities = np.append(self.priorities, abs(self.errors[-1]) ** int(self.rpe))

    def sample(self, batch_size):
        n = self.priorities.shape[0]
        probs = np.ones(n) / n
        prob_sum = np.sum(self.priorities)
        if prob_sum != 0:
            probs = self.priorities / prob_sum
        return self.rng.choice(n, p=probs, size=batch_size, replace=True)


def device_cdf(priorities) -> np.ndarray:
    """The normalised cumulative distribution of a draw in the order of csrc/adqn.hip."""
    pr = np.asarray(priorities, dtype=np.float64)
    n = len(pr)
    assert n >= 1
    c = (n + 63) // 64
    lanes = np.arange(64)
    held = (lanes[:, None] * c + np.arange(c)[None, :]) < n          # [64, c]
    chunk = np.zeros(64 * c)
    chunk[:n] = pr
    chunk = chunk.reshape(64, c)
    s = np.zeros(64)
    for k in range(c):
        s = np.where(held[:, k], s + chunk[:, k], s)
    for o in (1, 2, 4, 8, 16, 32):
        s = s + s[lanes ^ o]
    prob_sum = s[0]
    assert (s == prob_sum).all() or np.isnan(prob_sum)
    with np.errstate(all='ignore'):
        p = np.full((64, c), 1.0 / n) if prob_sum == 0 else chunk / prob_sum
    t = np.zeros(64)
    run = np.zeros((64, c))
    for k in range(c):
        t = np.where(held[:, k], t + p[:, k], t)
        run[:, k] = t
    inc = t.copy()
    for o in (1, 2, 4, 8, 16, 32):
        up = np.concatenate([np.zeros(o), inc[:-o]])
        inc = np.where(lanes >= o, inc + up, inc)
    excl = np.concatenate([[0.0], inc[:-1]])
    last_lane = (n - 1) // c
    last = excl[last_lane] + t[last_lane]
    return ((excl[:, None] + run) / last).reshape(-1)[:n]


def device_indices(cdf, u) -> np.ndarray:
    n = len(cdf)
    k = (np.asarray(cdf)[:, None] <= np.asarray(u)[None, :]).sum(axis=0)
    return np.minimum(k, n - 1).astype(np.int64)


class RefMemory(PlainMemory):
    """The device's memory: PlainMemory's store, the draw in the device's summation order."""

    def __init__(self, dim, decay=1.0, rpe=True, rng=None):
        super().__init__(dim, decay, rpe, rng)
        self.margin = float('inf')

    def store(self, state, action, reward):
        err = np.float64(action) - np.float64(reward)
        self.states = np.append(self.states, np.asarray(state, dtype=np.float64)[np.newaxis], axis=0)
        self.reinforcements = np.append(self.reinforcements, np.float64(reward))
        self.errors = np.append(self.errors, err)
        self.priorities = np.append(self.priorities * np.float64(self.decay),
                                    np.abs(err) if self.rpe else 1.0)

    def sample(self, batch_size):
        cdf = device_cdf(self.priorities)
        u = np.atleast_1d(self.rng.random(int(batch_size)))
        if len(cdf) > 1:
            self.margin = min(self.margin, float(np.abs(cdf[:-1, None] - u[None, :]).min()))
        return device_indices(cdf, u)


# -- agent/adqn.py ----------------------------------------------------------------------------------
def new_record() -> dict:
    return {'value': [], 'reward': [], 'end': [], 'idx': [], 'count': [], 'prio': [], 'steps': [],
            'trial_reward': []}


def new_net(params: dict) -> dict:
    p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    zero = {k: np.zeros_like(v) for k, v in p.items()}
    return {'p': p, 'm': zero, 'v': {k: v.copy() for k, v in zero.items()}, 'steps': 0.0}


class RefADQN:
    def __init__(self, params, memory, rec=None, batch=32):
        self.net = new_net(params)
        self.memory = memory
        self.current_trial = 0
        self.rec = new_record() if rec is None else rec
        self.batch = batch

    def retrieve_v(self, state) -> float:
        return float(mc.forward(self.net['p'], np.asarray(state, dtype=np.float64)[None])[2][0, 0])

    def predict_on_batch(self, batch):
        return mc.forward(self.net['p'], np.asarray(batch, dtype=np.float64))[2]

    def replay(self, batch_size, nb_replays):
        idx = self.memory.sample(batch_size)
        x, y = self.memory.states[idx], self.memory.reinforcements[idx][:, None]
        for _ in range(nb_replays):
            self.net = mc.fit_step(self.net, x, y, None, True, HYPER)
        return idx

    def _run(self, env, trials, steps, batch_size, nb_replays, learn):
        rec, mem = self.rec, self.memory
        for _ in range(trials):
            trial_reward = 0.0
            state, _ = env.reset()
            for step in range(steps):
                value = self.retrieve_v(state)
                ns, reward, end, _, _ = env.step(value)
                if learn:
                    mem.store(state, value, float(reward))
                    idx = self.replay(batch_size, nb_replays)
                else:
                    idx = np.full(self.batch, -1, dtype=np.int64)
                rec['value'].append(value)
                rec['reward'].append(float(reward))
                rec['end'].append(bool(end))
                rec['idx'].append(np.array(idx, dtype=np.int64))
                rec['count'].append(len(mem.priorities))
                rec['prio'].append(mem.priorities.copy())
                state = ns
                trial_reward += reward
                if end:
                    break
            self.current_trial += 1
            rec['steps'].append(step)
            rec['trial_reward'].append(trial_reward)

    def train(self, env, trials, steps, batch_size=32, nb_replays=1):
        self._run(env, trials, steps, batch_size, nb_replays, True)

    def test(self, env, trials, steps):
        self._run(env, trials, steps, 0, 0, False)


def run_sessions(ag, env, sessions) -> None:
    """The same for the restatement, the reference and the device.  A session is ('train', trials,
    steps, batch_size, nb_replays) or ('test', trials, steps)."""
    for s in sessions:
        getattr(ag, s[0])(env, *s[1:])


def weights_of(params: dict) -> np.ndarray:
    return np.concatenate([np.asarray(params[k], dtype=np.float64).reshape(-1) for k in mc.KEYS])


def pack(rec: dict, batch: int) -> dict:
    return {'value': np.array(rec['value'], dtype=np.float64),
            'reward': np.array(rec['reward'], dtype=np.float64),
            'end': np.array(rec['end'], dtype=bool),
            'idx': np.array(rec['idx'], dtype=np.int64).reshape(-1, batch),
            'count': np.array(rec['count'], dtype=np.int64),
            'prio': np.concatenate([np.zeros(0)] + [np.asarray(p, dtype=np.float64)
                                                    for p in rec['prio']]),
            'steps': np.array(rec['steps'], dtype=np.int64),
            'trial_reward': np.array(rec['trial_reward'], dtype=np.float64)}


def memory_arrays(mem) -> dict:
    return {'states': np.array(mem.states, dtype=np.float64),
            'reinforcements': np.array(mem.reinforcements, dtype=np.float64),
            'errors': np.array(mem.errors, dtype=np.float64),
            'priorities': np.array(mem.priorities, dtype=np.float64)}


def probe_of(dim: int) -> np.ndarray:
    return np.concatenate([np.eye(dim), np.full((1, dim), 0.5)])


def restate(schedule, observations, overwrite, seq_actions, params, decay, rpe, sessions, inst,
            batch, seed=SEED) -> dict:
    env = RefSequence(schedule, observations, seq_actions, overwrite)
    tape = TapeRNG(seed, inst, STREAM_ADQN_MEMORY)
    mem = RefMemory(env.dim, decay, rpe, tape)
    ag = RefADQN(params, mem, batch=batch)
    run_sessions(ag, env, sessions)
    out = pack(ag.rec, batch)
    out.update(memory_arrays(mem))
    out['weights'] = weights_of(ag.net['p'])
    out['predict'] = ag.predict_on_batch(probe_of(env.dim))
    out['draws'] = np.int64(tape.index)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['margin'] = np.float64(mem.margin)
    out['adam_steps'] = np.float64(ag.net['steps'])
    return out


EXACT = ('reward', 'end', 'idx', 'count', 'steps', 'trial_reward', 'states', 'reinforcements',
         'draws', 'position')
CLOSE = ('value', 'prio', 'errors', 'priorities', 'weights', 'predict')


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


def largest_difference(out, ref, prefix='', keys=CLOSE) -> float:
    return max(float(np.abs(np.asarray(out[k]) - np.asarray(ref[prefix + k])).max())
               for k in keys if np.asarray(out[k]).size)


# -- the recorded cases -----------------------------------------------------------------------------
def _unit():
    """unit_tests/test_adqn.py: alternating A/B trials, rewarded and punished."""
    seq = []
    for _ in range(10):
        seq.append([_step('A', 1.0)])
        seq.append([_step('B', -1.0)])
    return seq, {'A': np.array([1.0, 0.0]), 'B': np.array([0.0, 1.0])}, 1


def _multistep():
    """Trials of one to three steps, some cut by the cap; float rewards of every sign and array
    rewards under overwrite=True with the step's own action; observations that are not one-hot."""
    obs = {'A': np.array([1.0, 0.0, 0.0]), 'B': np.array([0.0, 1.0, 0.5]),
           'C': np.array([0.25, 0.0, 1.0])}
    two = [_step('A', 0.0), _step('B', np.array([1.0, -1.0]), 1)]
    three = [_step('A', -0.5), _step('B', 0.5), _step('C', np.array([0.25, 1.0]), 0)]
    one = [_step('C', 1.0)]
    return [two, one, three, two, three, one, one, three] * 3, obs, 2


def _case(design, sessions, inst, net_seed, decay=1.0, rpe=True, overwrite=False, dtype=np.float64):
    return dict(design=design, sessions=sessions, inst=inst, net_seed=net_seed, decay=decay,
                rpe=rpe, overwrite=overwrite, dtype=dtype)


CASES = {
    'unit': _case(_unit, [('train', 10, 10, 32, 1), ('test', 10, 10)], 0, 100),
    'unit_decay': _case(_unit, [('train', 10, 10, 32, 1), ('test', 10, 10)], 1, 101, decay=0.9),
    'unit_no_rpe': _case(_unit, [('train', 10, 10, 32, 1), ('test', 10, 10)], 2, 102, decay=0.9,
                         rpe=False),
    'unit_replays2': _case(_unit, [('train', 20, 10, 32, 2)], 3, 103),
    'two_sessions': _case(_unit, [('train', 10, 10, 32, 1), ('train', 10, 10, 32, 1)], 4, 104,
                          decay=0.9),
    'multistep_cut': _case(_multistep, [('train', 6, 2, 32, 1), ('train', 12, 5, 32, 1),
                                        ('test', 3, 2), ('train', 3, 3, 32, 2)], 5, 105,
                           decay=0.9, overwrite=True),
}
BATCH = 32


def case_params(name: str) -> dict:
    """The initial network of a case, D -> 64 -> 64 -> 1, as one float64 parameter dict."""
    c = CASES[name]
    obs = c['design']()[1]
    dim = np.asarray(next(iter(obs.values()))).size
    stack = mc.draw_networks(np.random.default_rng(c['net_seed']), 1, dim, 1, c['dtype'])
    return mc.one(stack, 0)


def restate_case(name: str) -> dict:
    c = CASES[name]
    schedule, obs, seq_actions = c['design']()
    return restate(schedule, obs, c['overwrite'], seq_actions, case_params(name), c['decay'],
                   c['rpe'], c['sessions'], c['inst'], BATCH)


_RESTATED = {}


def restated(name: str) -> dict:
    """``restate_case`` computed once and shared; not to be written to."""
    if name not in _RESTATED:
        _RESTATED[name] = restate_case(name)
    return _RESTATED[name]


def replay_memory(values, rewards, states, learned, decay, rpe, inst, batch, seed=SEED):
    """The device's memory fed with recorded (state, value, reward) of the steps marked in
    ``learned``: the priorities after every such step and the indices drawn there."""
    tape = TapeRNG(seed, inst, STREAM_ADQN_MEMORY)
    mem = RefMemory(states.shape[1], decay, rpe, tape)
    prio, idx = [], []
    for k in np.flatnonzero(learned):
        mem.store(states[k], values[k], rewards[k])
        idx.append(mem.sample(batch))
        prio.append(mem.priorities.copy())
    return mem, prio, idx


# -- torch models -----------------------------------------------------------------------------------
def torch_model(params: dict, dtype=np.float64):
    """Linear(D, 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, O) holding ``params``."""
    import torch
    from torch import nn
    D, O = params['w1'].shape[1], params['w3'].shape[0]
    model = nn.Sequential(OrderedDict([('l1', nn.Linear(D, mc.H)), ('r1', nn.ReLU()),
                                       ('l2', nn.Linear(mc.H, mc.H)), ('r2', nn.ReLU()),
                                       ('l3', nn.Linear(mc.H, O))]))
    model = model.double() if np.dtype(dtype) == np.float64 else model.float()
    with torch.no_grad():
        for k, layer in (('1', model.l1), ('2', model.l2), ('3', model.l3)):
            layer.weight.copy_(torch.from_numpy(np.asarray(params['w' + k], dtype=dtype)))
            layer.bias.copy_(torch.from_numpy(np.asarray(params['b' + k], dtype=dtype)))
    return model


# -- launch structs ---------------------------------------------------------------------------------
def fill_mem(lib, t, n, dim, cap, count_min, count_max, decay, rpe, seed=SEED, instance_base=0):
    """``t``: tensors by the struct's field names."""
    m = lib.ADQNMem()
    for name in ('states', 'reinforcements', 'errors', 'priorities', 'count', 'draw_ctr',
                 'instance_ids', 'scratch'):
        setattr(m, name, lib.ptr(t.get(name)))
    m.n, m.dim, m.cap, m.count_min, m.count_max = n, dim, cap, count_min, count_max
    m.instance_base, m.flags = instance_base, lib.ADQN_RPE if rpe else 0
    m.decay, m.seed = decay, seed
    return m


# -- the same on the device -------------------------------------------------------------------------
def device_run(schedules, observations, overwrite, seq_actions, params, decay, rpe, sessions,
               n_envs=1, instance_ids=None, instance_base=0, schedule_of=None, callbacks=None,
               record=4096, seed=SEED, dtype=np.float64, fused=None, model=None):
    """Build Sequence, memory, network and agent, run the sessions; returns (agent, interface)."""
    from cobel_amd.agent import ADQN
    from cobel_amd.interface import Sequence
    from cobel_amd.memory import ADQNMemory
    from cobel_amd.network import TorchNetwork
    from cobel_amd.spaces import Box
    shape = np.asarray(next(iter(observations.values()))).shape
    env = Sequence(schedules, observations, Box(0.0, 1.0, shape), seq_actions, overwrite,
                   n_envs=n_envs, seed=seed, schedule_of=schedule_of, instance_base=instance_base,
                   instance_ids=instance_ids)
    mem = ADQNMemory(env.observation_space, decay, rpe)
    net = TorchNetwork(torch_model(params, dtype) if model is None else model)
    ag = ADQN(env.observation_space, net, mem, custom_callbacks=callbacks)
    ag.record_steps, ag.fused_loop = record, fused
    run_sessions(ag, env, sessions)
    return ag, env


def device_case(name, **kw):
    c = CASES[name]
    schedule, obs, seq_actions = c['design']()
    return device_run(schedule, obs, c['overwrite'], seq_actions, case_params(name), c['decay'],
                      c['rpe'], c['sessions'], **kw)


def device_record(ag, env, i: int = 0) -> dict:
    """What ``restate`` returns, read back from instance i (the priorities after every step
    excepted)."""
    rows, mem, T = ag.recorded_steps(i), ag.memory, ag.current_trial
    n = int(mem._h_count[i])
    out = {'value': rows[:, 0].copy(), 'reward': rows[:, 1].copy(), 'end': rows[:, 2] != 0,
           'idx': ag.recorded_indices(i).astype(np.int64),
           'steps': ag.trial_steps_trace[i, :T].cpu().numpy().astype(np.int64),
           'trial_reward': ag.trial_reward_trace[i, :T].cpu().numpy()}
    assert int(mem._count[i].item()) == n, 'the host mirror of the count left the device'
    for k in ('states', 'reinforcements', 'errors', 'priorities'):
        out[k] = mem._arrays[k][i, :n].cpu().numpy()
    names = ag._net._mlp3_names()
    got = {}
    for j, name in enumerate(names):
        got['w%d' % (j + 1)] = ag._net.params[name + '.weight'][i].detach().cpu().numpy()
        got['b%d' % (j + 1)] = ag._net.params[name + '.bias'][i].detach().cpu().numpy()
    out['weights'] = weights_of(got)
    p = ag.predict_on_batch(probe_of(ag.dim))
    out['predict'] = np.asarray(p if ag.n_envs == 1 else p[i].cpu().numpy(), dtype=np.float64)
    out['draws'] = np.int64(mem._draw_ctr[i].item())
    out['position'] = np.array([int(env._trial[i].item()), int(env._step[i].item())], dtype=np.int64)
    assert out['position'][0] == env._h_trial[i] and out['position'][1] == env._h_step[i], \
        'the host mirror of the position left the device'
    out['adam_steps'] = np.float64(ag._net._steps[i].item()) if hasattr(ag._net, '_steps') \
        else np.float64(0)
    return out
