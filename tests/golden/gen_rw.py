"""Golden traces of the Rescorla-Wagner agents (agent/rw.py) on a Sequence environment
(interface/sequence.py) with the scalar policies (policy/scalar.py), recorded from the real
reference in float64.

The cases are those of tests/rw_common.py (``CASES``): the two demos shortened to 40 repetitions, a
blocking design, per-component learning rates, multi-step trials cut by the step cap,
``overwrite=True`` with array rewards, each policy with ``code_reverse`` both ways (``Threshold``
with a window, so that its draws are conditional) and one case of dense observations.  The
policies draw from the tape generators.  Recorded per step: value, action (``log['action']`` of
``Sequence.step``), reward and end flag; per trial ``W``, ``logs['steps']`` and the trial reward; at
the end the generator indices, the position and ``predict_on_batch(np.eye(D))``.

Asserted here: no recorded double draw lies within 1e-12 of the probability it is compared with
(the device's exp is not libm's); the restatement equals the reference exactly in every case but
the dense one.  Printed: the largest differences of the dense case in ``W``, in the values and in
the final predictions, restatement against reference (``DENSE_MEASURED`` / ``DENSE_BOUND`` of
rw_common.py).

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_rw.py

Reuses the shim and the tape generators of gen_golden.py.  Writes rw_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import rw_common as rc  # noqa: E402


def reference_case(c: dict) -> dict:
    import gymnasium
    from cobel.agent import BinaryRescorlaWagner, RescorlaWagner
    from cobel.interface import Sequence
    from cobel.policy import Proportional, Sigmoid, Threshold
    classes = {'proportional': Proportional, 'threshold': Threshold, 'sigmoid': Sigmoid}
    schedule, obs = c['design']()
    dim = np.asarray(next(iter(obs.values()))).size
    env = Sequence(schedule, obs, gymnasium.spaces.Box(0.0, 1.0, (dim,)), c['nb_actions'],
                   c['overwrite'])
    rngs = [TapeRNG(SEED, c['inst'], rc.STREAM_POLICY), TapeRNG(SEED, c['inst'], rc.STREAM_POLICY_TEST)]
    rec = rc.new_record()
    last = {}

    def on_trial_end(logs):
        rec['W'].append(np.array(logs['agent'].W, dtype=np.float64))
        rec['steps'].append(logs['steps'])
        rec['trial_reward'].append(logs['trial_reward'])
        rec['last_action'].append(last['action'])

    cbs = {'on_trial_end': [on_trial_end]}
    lr = c['lr']
    if c['policy'] is None:
        ag = RescorlaWagner(env.observation_space, lr, cbs)
        pols = []
    else:
        pol = classes[c['policy'][0]](rng=rngs[0], **c['policy'][1])
        pol_t = None if c['policy_test'] is None else \
            classes[c['policy_test'][0]](rng=rngs[1], **c['policy_test'][1])
        ag = BinaryRescorlaWagner(env.observation_space, pol, pol_t, lr, cbs)
        pols = [p for p in (pol, pol_t) if p is not None]
    if c['w0'] is not None:
        ag.W.fill(c['w0'])
    orig_predict, orig_step = ag.predict_on_batch, env.step

    def predict(batch):
        out = orig_predict(batch)
        last['v'] = float(out[0])
        return out

    def step(action):
        out = orig_step(action)
        rec['value'].append(last['v'])
        rec['action'].append(int(out[4]['action']))
        rec['reward'].append(float(out[1]))
        rec['end'].append(bool(out[2]))
        last['action'] = int(out[4]['action'])
        return out

    ag.predict_on_batch, env.step = predict, step
    # the margin between every double draw and the probability it is compared with
    margin = [float('inf')]
    for p in pols:
        if isinstance(p, Threshold):
            continue
        real = p.rng.random

        def random(p=p, real=real):
            u = real()
            v = last['v'] / p.value_max
            prob = v if isinstance(p, Proportional) else \
                1 / (1 + np.exp(-(v - p.threshold) * p.scale))
            margin[0] = min(margin[0], abs(u - prob))
            return u

        p.rng.random = random
    for kind, trials, steps in c['sessions']:
        (ag.train if kind == 'train' else ag.test)(env, trials, steps)
    ag.predict_on_batch = orig_predict
    out = rc.pack(rec, dim)
    out['index'] = np.array([rngs[0].index, rngs[1].index], dtype=np.int64)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['predict'] = np.array(ag.predict_on_batch(rc.probe_of(dim)), dtype=np.float64)
    out['margin'] = np.float64(margin[0])
    return out


def policy_probabilities() -> dict:
    """get_action_probs of the three policies on a grid of values (tests/test_host_rw.py)."""
    from cobel.policy import Proportional, Sigmoid, Threshold
    values = np.array([-0.25, 0.0, 0.1, 0.39, 0.4, 0.45, 0.5, 0.55, 0.61, 0.9, 1.0, 1.4])
    out = {'probs/values': values}
    for name, make in (('proportional', lambda cr: Proportional(1.5, cr)),
                       ('threshold', lambda cr: Threshold(0.5, 0.2, 1.25, cr)),
                       ('sigmoid', lambda cr: Sigmoid(0.4, 3.0, 1.25, cr))):
        for cr in (True, False):
            pol = make(cr)
            out['probs/%s_%d' % (name, cr)] = np.array(
                [pol.get_action_probs(np.float64(v)) for v in values], dtype=np.float64)
    return out


def main() -> None:
    out = {}
    for name, c in rc.CASES.items():
        d = reference_case(c)
        r = rc.restate_case(name)
        assert d['margin'] > 1e-12, '%s: a draw within 1e-12 of its probability (%g): take another ' \
                                    'instance number' % (name, d['margin'])
        if c['dense']:
            for k in ('action', 'end', 'steps', 'index', 'position'):
                assert np.array_equal(d[k], r[k]), (name, k)
            for k in ('W', 'value', 'predict'):
                diff = float(np.abs(d[k] - r[k]).max())
                bound = 2.0 ** np.ceil(np.log2(diff)) if diff > 0 else 0.0
                if bound == diff:
                    bound *= 2
                print('%-22s largest |%s(restatement) - %s(reference)| = %.17g -> bound %.17g '
                      '(2^%d)' % (name, k, k, diff, bound, int(np.log2(bound)) if bound else 0))
        else:
            rc.assert_same_record(r, d, what=name + ' (restatement vs reference)')
        nz = max(int((np.asarray(o) != 0).sum()) for o in c['design']()[1].values())
        assert c['dense'] or nz <= 2, name
        print('%-22s steps %4d trials %3d draws %s margin %.3g' % (
            name, len(d['value']), len(d['steps']), d['index'].tolist(), d['margin']))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    out.update(policy_probabilities())
    path = G._out('rw_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
