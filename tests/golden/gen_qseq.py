"""Golden traces of QAgent (agent/q.py) on a Sequence environment (interface/sequence.py) with the
Softmax and EpsilonGreedy policies, recorded from the real reference in float64.

The cases are those of tests/qseq_common.py (``CASES``): the grid-search demo shortened to 12
repetitions (8 actions, batches of 32), multi-step trials cut by the step cap with float rewards
mixed with array rewards, ``overwrite=True``, one action and three, a session without replay followed
by one with batches of 5, epsilon-greedy with exact ties, observations that share their values (and
one of all zeros), and ``train`` / ``test`` with a distinct ``policy_test``.  The policies and the
agent draw from the tape generators: ``policy`` from STREAM_POLICY, ``policy_test`` from its own
stream, the agent's replay from STREAM_MEMORY.  Recorded per step: action, reward, end flag and td
(0 in ``test``); per trial ``Q`` as an array in key order (tests/qseq_common.keys_of), ``logs['steps']``
and the trial reward; at the end the generator indices, ``len(M)``, ``M`` itself, the keys of ``Q`` in
the order the dict holds them, the position and the margin.

Asserted here: every recorded draw lies at least 1e-9 away from every edge of the normalised CDF it
is compared with (the device's exp is not NumPy's, and its softmax sum runs in action order), and
the restatement equals the reference exactly in every case.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_qseq.py

Reuses the shim and the tape generators of gen_golden.py.  Writes qseq_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import qseq_common as qc  # noqa: E402


def reference_case(c: dict) -> dict:
    import gymnasium
    from cobel.agent import QAgent
    from cobel.interface import Sequence
    from cobel.policy import EpsilonGreedy, Softmax
    schedule, obs = c['design']()
    shape = np.asarray(next(iter(obs.values()))).shape
    A = c['nb_actions']
    env = Sequence(schedule, obs, gymnasium.spaces.Box(0.0, 1.0, shape), A, c['overwrite'])
    key, tuples = qc.keys_of(obs)
    rngs = [TapeRNG(SEED, c['inst'], qc.STREAM_POLICY), TapeRNG(SEED, c['inst'], qc.STREAM_POLICY_TEST),
            TapeRNG(SEED, c['inst'], qc.STREAM_MEMORY)]

    def make(spec, rng):
        return (Softmax if spec[0] == 'softmax' else EpsilonGreedy)(spec[1], rng)

    pol = make(c['policy'], rngs[0])
    pol_t = None if c['policy_test'] is None else make(c['policy_test'], rngs[1])
    rec = qc.new_record()
    margin = [float('inf')]

    def on_step_end(logs):
        rec['action'].append(int(logs['action']))
        rec['reward'].append(float(logs['reward']))
        rec['end'].append(logs['terminal'] == 0)
        rec['td'].append(float(logs['td']) if 'td' in logs else 0.0)

    def on_trial_end(logs):
        q = np.zeros((len(tuples), A))
        for t, row in logs['agent'].Q.items():
            q[tuples.index(t)] = row
        rec['Q'].append(q)
        rec['steps'].append(logs['steps'])
        rec['trial_reward'].append(logs['trial_reward'])

    ag = QAgent(env.observation_space, gymnasium.spaces.Discrete(A), pol, pol_t, c['lr'], c['gamma'],
                {'on_step_end': [on_step_end], 'on_trial_end': [on_trial_end]}, rngs[2])
    # the margin between every draw and the edges of the CDF it is compared with
    for p in [q for q in (pol, pol_t) if q is not None]:
        real = p.select_action

        def select(v, mask=None, p=p, real=real):
            cdf = np.cumsum(p.get_action_probs(v, mask))
            cdf /= cdf[-1]
            a = real(v, mask)
            if len(cdf) > 1:
                margin[0] = min(margin[0], float(np.abs(cdf[:-1] - p.rng.log[-1]).min()))
            return a

        p.select_action = select
    for kind, trials, steps, batch in c['sessions']:
        if kind == 'train':
            ag.train(env, trials, steps, batch)
        else:
            ag.test(env, trials, steps)
    out = qc.pack(rec, len(tuples), A)
    out['index'] = np.array([r.index for r in rngs], dtype=np.int64)
    out['len_M'] = np.int64(len(ag.M))
    out['created'] = np.array([tuples.index(t) for t in ag.Q], dtype=np.int64)
    out['M'] = np.array([[tuples.index(e['state']), e['action'], tuples.index(e['next_state']),
                          e['terminal']] for e in ag.M], dtype=np.int64).reshape(-1, 4)
    out['M_reward'] = np.array([e['reward'] for e in ag.M], dtype=np.float64)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['margin'] = np.float64(margin[0])
    return out


def softmax_probabilities() -> dict:
    """get_action_probs of the reference's Softmax on the known-answer rows (tests/test_gpu_qseq.py)."""
    from cobel.policy import Softmax
    out = {}
    for name, (v, mask, beta) in qc.KAT_ROWS.items():
        out['probs/' + name] = Softmax(beta).get_action_probs(
            np.array(v, dtype=np.float64), None if mask is None else np.array(mask, dtype=bool))
    return out


def main() -> None:
    out = {}
    for name, c in qc.CASES.items():
        d = reference_case(c)
        r = qc.restate_case(name)
        assert d['margin'] > qc.MARGIN, '%s: a draw within 1e-9 of an edge of its CDF (%g): take ' \
                                        'another instance number' % (name, d['margin'])
        qc.assert_same_record(r, d, what=name + ' (restatement vs reference)')
        print('%-16s steps %4d trials %3d draws %s len(M) %4d margin %.3g' % (
            name, len(d['action']), len(d['steps']), d['index'].tolist(), int(d['len_M']),
            d['margin']))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    out.update(softmax_probabilities())
    path = G._out('qseq_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
