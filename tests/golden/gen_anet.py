"""Golden traces of the AssociativeNetwork agent (agent/anet.py) on a Sequence environment
(interface/sequence.py) with the EpsilonGreedy policy (policy/greedy.py), recorded from the real
reference in float64.

The cases are those of tests/anet_common.py (``CASES``): the reference's unit-test design in four
variants (plain, ``linear_update``, dict ``saturation``, dict ``learning_rate``), one output and
eight outputs, observations of 33 and 64 components, multi-step trials cut by the step cap with
float, zero and negative rewards and overwritten array rewards, exact ties (``noise=0.0``),
observation components that are neither zero nor one, ``rescale_weights`` / ``alpha`` /
``predict_on_batch`` between sessions, and one case of dense observations.  The agent's ``rng`` is
a tape on STREAM_AGENT (a vector draw takes consecutive indices), the policy's a tape on
STREAM_POLICY, ``policy_test``'s one on STREAM_POLICY_TEST.  Recorded per step: q, action, reward and
end flag; per trial both weight matrices, ``logs['steps']`` and the trial reward; the predictions
made between sessions; at the end the three generator indices, the position and
``predict_on_batch(np.eye(D))``.

Asserted here: no policy draw lies within 1e-12 of a threshold of the cumulative probabilities; in
the dense case the two largest outputs of every step differ by more than 1e-9 (a difference in the
last bits cannot flip the argmax); all other cases have observations of at most two non-zero
components, each a power of two, and there the restatement equals the reference exactly in every
recorded array.  Printed: the largest differences of the dense case in the weights, the outputs and
the final predictions, restatement against reference (``DENSE_MEASURED`` / ``DENSE_BOUND`` of
anet_common.py).

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_anet.py

Reuses the shim and the tape generators of gen_golden.py.  Writes anet_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import anet_common as ac  # noqa: E402


def reference_case(c: dict) -> dict:
    import gymnasium
    from cobel.agent import AssociativeNetwork
    from cobel.interface import Sequence
    from cobel.policy import EpsilonGreedy
    schedule, obs, seq_actions = c['design']()
    dim = np.asarray(next(iter(obs.values()))).size
    na = c['n_actions'] - 1
    env = Sequence(schedule, obs, gymnasium.spaces.Box(0.0, 1.0, (dim,)), seq_actions,
                   c['overwrite'])
    rngs = [ac.NoiseTape(SEED, c['inst'], ac.STREAM_AGENT), TapeRNG(SEED, c['inst'], ac.STREAM_POLICY),
            TapeRNG(SEED, c['inst'], ac.STREAM_POLICY_TEST)]
    rec = ac.new_record()

    def on_trial_end(logs):
        rec['We'].append(np.array(logs['agent'].weights['excitatory'], dtype=np.float64))
        rec['Wi'].append(np.array(logs['agent'].weights['inhibitory'], dtype=np.float64))
        rec['steps'].append(logs['steps'])
        rec['trial_reward'].append(logs['trial_reward'])

    pol = EpsilonGreedy(c['eps'], rngs[1])
    pol_t = None if c['eps_test'] is None else EpsilonGreedy(c['eps_test'], rngs[2])
    ag = AssociativeNetwork(env.observation_space, gymnasium.spaces.Discrete(c['n_actions']), pol,
                            pol_t, custom_callbacks={'on_trial_end': [on_trial_end]}, rng=rngs[0],
                            **c['agent_kw'])
    orig_q, orig_step = ag.retrieve_q, env.step
    last, margin, gap = {}, [float('inf')], [float('inf')]

    def retrieve_q(observation):
        q = orig_q(observation)
        last['q'] = np.array(q, dtype=np.float64)
        return q

    def step(action):
        out = orig_step(action)
        rec['q'].append(last['q'])
        rec['action'].append(int(action))
        rec['reward'].append(float(out[1]))
        rec['end'].append(bool(out[2]))
        if na > 1:
            top = np.sort(last['q'])[-2:]
            gap[0] = min(gap[0], float(top[1] - top[0]))
        return out

    # the margin between every policy draw and the thresholds it is compared with
    real = pol.rng.random

    def random(size=None):
        u = real(size)
        cdf = np.cumsum(pol.get_action_probs(last['q']))
        cdf /= cdf[-1]
        margin[0] = min([margin[0]] + [abs(u - t) for t in cdf[:-1]])
        return u

    pol.rng.random = random
    ag.retrieve_q, env.step = retrieve_q, step
    # (predict_on_batch calls retrieve_q through the instance: the wrapper only remembers q)
    ac.run_sessions(ag, env, c['sessions'], rec)
    ag.retrieve_q = orig_q
    out = ac.pack(rec, dim, na)
    out['index'] = np.array([r.index for r in rngs], dtype=np.int64)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['predict'] = np.array(ag.predict_on_batch(ac.probe_of(dim)), dtype=np.float64)
    out['margin'] = np.float64(margin[0])
    out['gap'] = np.float64(gap[0])
    return out


def main() -> None:
    out = {}
    for name, c in ac.CASES.items():
        d = reference_case(c)
        r = ac.restate_case(name)
        assert d['margin'] > 1e-12, '%s: a policy draw within 1e-12 of a threshold (%g): take ' \
                                    'another instance number' % (name, d['margin'])
        observations = c['design']()[1]
        if c['dense']:
            assert d['gap'] > 1e-9 and r['gap'] > 1e-9, \
                '%s: the two largest outputs of a step within 1e-9 (%g): take another instance ' \
                'number' % (name, min(d['gap'], r['gap']))
            assert max(int(((np.asarray(o) != 0) & (np.frexp(np.asarray(o))[0] != 0.5)).sum())
                       for o in observations.values()) >= 3, name
            ac.assert_same_record(r, d, what=name + ' (restatement vs reference)', keys=ac.DISCRETE)
            for key, pair in (('W', ('We', 'Wi')), ('q', ('q',)), ('predict', ('predict',))):
                diff = max(float(np.abs(d[k] - r[k]).max()) for k in pair)
                bound = 2.0 ** np.ceil(np.log2(diff)) if diff > 0 else 0.0
                if bound == diff:
                    bound *= 2
                print('%-18s largest |%s(restatement) - %s(reference)| = %.17g -> bound %.17g '
                      '(2^%d)' % (name, key, key, diff, bound, int(np.log2(bound)) if bound else 0))
        else:
            for o in observations.values():
                nz = np.asarray(o)[np.asarray(o) != 0]
                assert len(nz) <= 2 and all(np.frexp(v)[0] == 0.5 for v in nz), name
            ac.assert_same_record(r, d, what=name + ' (restatement vs reference)')
        print('%-18s steps %4d trials %3d draws %s margin %.3g gap %.3g' % (
            name, len(d['action']), len(d['steps']), d['index'].tolist(), d['margin'], d['gap']))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    path = G._out('anet_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
