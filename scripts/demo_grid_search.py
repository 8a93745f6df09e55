"""The grid-search demo on the device: fit the learning rate and the inverse temperature of a
Q-learning agent with a softmax policy on a bandit-like task.

Four one-hot stimuli are shown in turn; under each, one of eight arms pays.  Synthetic behaviour is
made with a learning rate of 0.9 and an inverse temperature of 1 (100 runs); a 9 x 3 grid of
(learning_rate, beta) with 100 runs per combination is then simulated — 2 700 agents on 2 700
environment instances, laid out with ``spread_over_instances`` and run by ONE launch — and the
combination whose mean trial-by-trial reward lies closest to the data is printed.

    python scripts/demo_grid_search.py [--runs 100] [--repetitions 100] [--seed 1]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cobel-rl_amd')]

from cobel_amd.agent import QAgent  # noqa: E402
from cobel_amd.interface import Sequence  # noqa: E402
from cobel_amd.optimizer import GridSearchOptimizer  # noqa: E402
from cobel_amd.optimizer.grid_search import spread_over_instances  # noqa: E402
from cobel_amd.policy import Softmax  # noqa: E402
from cobel_amd.spaces import Box, Discrete  # noqa: E402

ARMS = 8
TRUTH = {'learning_rate': 0.9, 'beta': 1}
GRID = {'learning_rate': [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], 'beta': [1, 5, 10]}


def make_task(repetitions: int) -> dict:
    """Stimulus k of A, B, C, D pays on arm 2 k; every trial is one step."""
    names = 'ABCD'
    trials = [[{'observation': name, 'reward': np.eye(ARMS)[2 * k], 'action': None}]
              for _ in range(repetitions) for k, name in enumerate(names)]
    return {'sequence': trials, 'observations': {n: np.eye(4)[k] for k, n in enumerate(names)},
            'observation_space': Box(0.0, 1.0, (4,)), 'action_space': Discrete(ARMS)}


def simulate(task: dict, learning_rate, beta, n: int, seed: int, first_instance: int) -> np.ndarray:
    """``n`` agents, each on its own instance of the task, in one launch: the reward of every trial,
    ``[n, trials]``.  ``learning_rate`` and ``beta`` are scalars or one value per instance."""
    env = Sequence(task['sequence'], task['observations'], task['observation_space'],
                   int(task['action_space'].n), n_envs=n, seed=seed, instance_base=first_instance)
    agent = QAgent(task['observation_space'], task['action_space'], Softmax(beta),
                   learning_rate=learning_rate)
    agent.train(env, len(task['sequence']), 100)       # (batches of 32 replayed experiences per step)
    return agent.trial_reward_trace.cpu().numpy()


def loss(simulation_data: dict, behavioral_data: dict) -> float:
    return float(np.sum(np.sqrt((np.mean(simulation_data['demo'], axis=0)
                                 - np.mean(behavioral_data['demo'], axis=0)) ** 2)))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--runs', type=int, default=100)
    ap.add_argument('--repetitions', type=int, default=100, help='of the four stimuli (400 trials)')
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    task = make_task(args.repetitions)
    data = {'demo': list(simulate(task, TRUTH['learning_rate'], float(TRUTH['beta']), args.runs,
                                  args.seed, 0))}
    launches = []

    def simulation_batch(task, combinations, nb_runs):
        par, which = spread_over_instances(combinations, nb_runs)
        launches.append(len(which))
        # (instance numbers after those of the data: no run shares its random streams with another)
        rows = simulate(task, par['learning_rate'].astype(np.float64), par['beta'].astype(np.float64),
                        len(which), args.seed, args.runs)
        return [list(rows[which == k]) for k in range(len(combinations))]

    with tempfile.TemporaryDirectory() as folder:
        optimizer = GridSearchOptimizer(folder + '/', GRID, args.runs, 'nested')
        fit = optimizer.fit_vectorised(simulation_batch, {'demo': task}, data, loss)
    keys, losses = list(fit), np.array(list(fit.values()))
    best = keys[int(np.argmin(losses))]
    truth = (TRUTH['learning_rate'], TRUTH['beta'])
    print('%d combinations x %d runs = %d instances of %d trials in %d launch(es)'
          % (len(keys), args.runs, sum(launches), len(task['sequence']), len(launches)))
    print('Best fit is: ', best, ' loss %.4f' % losses.min())
    print('Ground Truth:', truth, ' loss %.4f' % fit[truth])
    li = GRID['learning_rate'].index(best[0]) - GRID['learning_rate'].index(truth[0])
    bi = GRID['beta'].index(best[1]) - GRID['beta'].index(truth[1])
    if (li, bi) == (0, 0):
        print('The grid search recovers the ground truth.')
    elif max(abs(li), abs(bi)) <= 1:
        print('The grid search lands on a neighbour of the ground truth on the grid '
              '(%+d step(s) in learning_rate, %+d in beta).' % (li, bi))
    else:
        print('The grid search does NOT recover the ground truth or a neighbour of it.')
        sys.exit(1)


if __name__ == '__main__':
    main()
