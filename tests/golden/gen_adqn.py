"""Golden traces of the ADQN agent (agent/adqn.py) with its ADQNMemory (memory/adqn.py) and a
TorchNetwork (network/network_torch.py) D -> 64 -> 64 -> 1 in float64 on a Sequence environment
(interface/sequence.py), recorded from the real reference.

The cases are those of tests/adqn_common.py (``CASES``): the reference's unit-test design (A
rewarded, B punished) with ``decay`` 1 and 0.9, with ``rpe`` off, with two replays per step and as
two training sessions back to back, a ``test()`` session behind the training, and multi-step trials
cut by the step cap with overwritten array rewards.  The memory's ``rng`` is a tape on
STREAM_ADQN_MEMORY: ``choice(n, p=probs, size=32)`` is one call, 32 doubles of one draw index.
Recorded per step: value, reward, end flag, the drawn indices (-1 in ``test()``), the count and
the priorities; per trial ``logs['steps']`` and the trial reward; at the end the memory's arrays,
the weights, ``predict_on_batch`` of a probe, the tape's index and the position.

Asserted here, for every case: no draw lies within 1e-9 of a cdf boundary, neither in the
reference's cdf nor in the restatement's; the largest difference between restatement and reference
in any value is at most a hundredth of that margin divided by the largest count; the drawn
indices, rewards, end flags, counts, states and reinforcements are equal.  Printed: the largest
absolute difference, restatement against reference, in values, priorities, errors, weights and
predictions (``VALUE_MEASURED`` of adqn_common.py; ``VALUE_BOUND`` is 16 times it).

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_adqn.py

Reuses the shim and the tape generators of gen_golden.py.  Writes adqn_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import adqn_common as ac  # noqa: E402

MARGIN = 1e-9


def reference_case(name: str) -> dict:
    import gymnasium
    import torch
    from cobel.agent import ADQN
    from cobel.interface import Sequence
    from cobel.memory import ADQNMemory
    from cobel.network import TorchNetwork
    torch.set_num_threads(1)
    c = ac.CASES[name]
    schedule, obs, seq_actions = c['design']()
    dim = np.asarray(next(iter(obs.values()))).size
    env = Sequence(schedule, obs, gymnasium.spaces.Box(0.0, 1.0, (dim,)), seq_actions,
                   c['overwrite'])
    tape = ac.ChoiceTape(SEED, c['inst'], ac.STREAM_ADQN_MEMORY)
    mem = ADQNMemory(env.observation_space, c['decay'], c['rpe'], tape)
    net = TorchNetwork(ac.torch_model(ac.case_params(name)))
    rec = ac.new_record()
    replayed = [False]

    def on_step_end(logs):
        rec['value'].append(float(logs['action']))
        rec['reward'].append(float(logs['reward']))
        rec['end'].append(logs['terminal'] == 0)
        rec['idx'].append(tape.drawn[-1] if replayed[0] else np.full(ac.BATCH, -1, dtype=np.int64))
        rec['count'].append(len(mem.priorities))
        rec['prio'].append(np.array(mem.priorities, dtype=np.float64))
        replayed[0] = False

    def on_trial_end(logs):
        rec['steps'].append(logs['steps'])
        rec['trial_reward'].append(logs['trial_reward'])

    ag = ADQN(env.observation_space, net, mem,
              custom_callbacks={'on_step_end': [on_step_end], 'on_trial_end': [on_trial_end]})
    orig = ag.replay

    def replay(batch_size=32, nb_replays=1):
        orig(batch_size, nb_replays)
        replayed[0] = True

    ag.replay = replay
    ac.run_sessions(ag, env, c['sessions'])
    out = ac.pack(rec, ac.BATCH)
    out.update(ac.memory_arrays(mem))
    out['weights'] = ac.weights_of(dict(zip(('w1', 'b1', 'w2', 'b2', 'w3', 'b3'),
                                            net.get_weights())))
    out['predict'] = np.array(ag.predict_on_batch(ac.probe_of(dim)), dtype=np.float64)
    out['draws'] = np.int64(tape.index)
    out['position'] = np.array([env.current_trial, env.current_step], dtype=np.int64)
    out['margin'] = np.float64(tape.margin)
    return out


def main() -> None:
    out, worst = {}, 0.0
    for name in ac.CASES:
        d = reference_case(name)
        r = ac.restate_case(name)
        margin = min(float(d['margin']), float(r['margin']))
        assert margin > MARGIN, '%s: a draw within %g of a cdf boundary (%g): take another ' \
                                'instance number' % (name, MARGIN, margin)
        ac.assert_same_record(r, d, what=name + ' (restatement vs reference)')
        diff = ac.largest_difference(r, d)
        value = float(np.abs(r['value'] - d['value']).max())
        allowed = margin / 100.0 / max(int(d['count'].max()), 1)
        assert value <= allowed, '%s: values differ by %g, more than margin / 100 / count = %g' % (
            name, value, allowed)
        worst = max(worst, diff)
        print('%-14s steps %3d count %3d draws %3d margin %.3g largest |restatement - reference| '
              '%.17g (values %.3g)' % (name, len(d['value']), int(d['count'].max()),
                                       int(d['draws']), margin, diff, value))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    print('VALUE_MEASURED = %.17g -> VALUE_BOUND = %.17g' % (worst, 16 * worst))
    path = G._out('adqn_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
