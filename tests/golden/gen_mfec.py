"""Golden traces of the MFEC agent (agent/mfec.py), recorded from the real reference in float64
with scikit-learn's own ``KDTree``.

``MFEC.train`` (one case followed by ``test``) on a ``Topology`` with an ``OfflineSimulator`` and an
``EpsilonGreedy`` policy, as demo/topology/demo_mfec.py sets it up, ``projection_size`` 16 and
``rng=np.random.default_rng(instance)``.  Every buffer stays at or below 80 entries (asserted), so
that each tree is a single leaf and the reference is deterministic.  Recorded per case: the compact
tables of the graph, the feature table (``process_observation`` of every node's observation), node,
action, reward and terminal flag of every step, the Q estimates handed to the policy, after every
trial each buffer's node ids, values and times, the generator indices and a final
``predict_on_batch`` over all nodes.  ``cobel.agent.mfec.time`` is patched with a counter that
advances by one per call (tests/mfec_common.py: the one deliberate difference).

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_mfec.py

Reuses the shim and the tape generators of gen_golden.py.  Writes mfec_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, STREAM_ENV, STREAM_POLICY, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import mfec_common as mc  # noqa: E402

PROJECTION = 16
# name: (graph, observations, instance, trials, steps, capacity, k, test trials, epsilon)
CASES = {
    'track_k3_c12': ('track', 'onehot', 0, 30, 150, 12, 3, 0, 0.1),
    'grid5_k10_c80': ('grid5', 'onehot', 1, 40, 40, 80, 10, 0, 0.1),
    'hex4_k2_c10': ('hex4', 'onehot', 2, 40, 30, 10, 2, 0, 0.1),
    'grid5_timeouts': ('grid5', 'onehot', 3, 40, 6, 20, 3, 0, 0.1),
    'track_c2_k3': ('track', 'onehot', 4, 20, 150, 2, 3, 0, 0.1),
    'track_dict': ('track', 'dict', 5, 25, 100, 12, 3, 0, 0.1),
    'track_traintest': ('track', 'onehot', 6, 25, 150, 12, 3, 8, 0.1),
}


class Clock:
    def __init__(self):
        self.t = 0

    def time(self):
        self.t += 1
        return float(self.t)


def graph(name):
    from cobel.misc import topology_tools as tt
    if name == 'track':
        return tt.linear_track(10, 2, 1.0, 20, 'right')
    if name == 'grid5':
        return tt.grid(5, (0.0, 1.0))
    return tt.hexagonal(4, (0.0, 1.0))


def case(gname, okind, inst, trials, steps, capacity, k, test_trials, eps) -> dict:
    import gymnasium
    import cobel.agent.mfec as M
    from cobel.interface import OfflineSimulator, Topology
    from cobel.policy import EpsilonGreedy
    nodes, starts = graph(gname)
    ids = list(nodes)
    S = len(ids)
    index = {n: i for i, n in enumerate(ids)}
    if okind == 'dict':
        obs = {nodes[n]['pose']: {'1': np.array(nodes[n]['pose']), '2': np.array(nodes[n]['pose'])}
               for n in ids}
        space = gymnasium.spaces.Dict({'1': gymnasium.spaces.Box(0., 1., (6,)),
                                       '2': gymnasium.spaces.Box(0., 1., (6,))})
    else:
        obs = {nodes[n]['pose']: o for n, o in zip(ids, np.eye(S))}
        space = gymnasium.spaces.Box(low=0.0, high=1.0, shape=(S,))
    env = Topology(nodes, starts, OfflineSimulator(obs, space), rng=TapeRNG(SEED, inst, STREAM_ENV))
    pol = EpsilonGreedy(eps, rng=TapeRNG(SEED, inst, STREAM_POLICY))
    M.time = Clock()
    tr = mc.new_trace()
    last = {}

    def on_trial_end(logs):
        tr['steps'].append(logs['steps'])
        tr['ended'].append(bool(last['end']))
        mc.snapshot(tr, logs['agent'].Q.buffers, lambda b: [node_of[x.tobytes()] for x in b.states])

    ag = M.MFEC(env.observation_space, env.action_space, pol, capacity=capacity, k=k,
                projection_size=PROJECTION, rng=np.random.default_rng(inst),
                custom_callbacks={'on_trial_end': [on_trial_end]})
    F = np.array([ag.process_observation(obs[nodes[n]['pose']]) for n in ids])
    node_of = {F[i].tobytes(): i for i in range(S)}
    assert len(node_of) == S
    A = ag.nb_actions
    orig_q, orig_sel, orig_step = ag.retrieve_q, pol.select_action, env.step

    def retrieve_q(state):
        q = orig_q(state)
        last['s'], last['q'] = node_of[np.asarray(state).tobytes()], np.array(q, dtype=np.float64)
        return q

    def select_action(v, mask=None):
        last['a'] = int(orig_sel(v, mask))
        return last['a']

    def step(action):
        out = orig_step(action)
        last['end'] = bool(out[2])
        tr['sar'].append((last['s'], last['a'], float(out[1]), float(out[2])))
        tr['q'].append(last['q'])
        return out

    ag.retrieve_q, pol.select_action, env.step = retrieve_q, select_action, step
    ag.train(env, trials, steps)
    if test_trials:
        ag.test(env, test_trials, steps)
    assert max(max(r) for r in tr['buf_len']) <= 80, 'a tree of more than one leaf'
    d = mc.pack(tr, A)
    d['index'] = np.array([env.rng.index, pol.rng.index], dtype=np.int64)
    d['predict'] = np.array(ag.predict_on_batch([obs[nodes[n]['pose']] for n in ids]),
                            dtype=np.float64)
    d['F'] = F
    d['projection'] = np.array(ag.projection)
    d['cfg'] = np.array([inst, trials, steps, capacity, k, test_trials, round(eps * 1e6)],
                        dtype=np.int64)
    d['gamma'] = np.float64(ag.gamma)
    d['tab_next'] = np.array([[index[m] for m in nodes[n]['neighbors']] for n in ids], dtype=np.uint16)
    d['tab_reward'] = np.array([nodes[n]['reward'] for n in ids], dtype=np.float64)
    d['tab_terminal'] = np.array([bool(nodes[n]['terminal']) for n in ids]).astype(np.uint8)
    d['tab_starts'] = np.array([index[n] for n in starts], dtype=np.uint16)
    d['graph'], d['observations'] = np.array(gname), np.array(okind)
    return d


def main() -> None:
    out = {}
    for name, args in CASES.items():
        d = case(*args)
        ended = d['ended'][:args[3]]
        if name == 'grid5_timeouts':
            assert ended.any() and not ended.all(), 'some trials must time out, some must not'
        print('%-18s steps %5d ended %3d/%3d  buffers %s non-zero estimates %d' % (
            name, len(d['state']), int(d['ended'].sum()), len(d['ended']), d['buf_len'][-1].tolist(),
            int((d['q'] != 0).sum())))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    path = G._out('mfec_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
