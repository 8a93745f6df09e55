"""A fixed slice of the randomised parity sweep (scripts/fuzz_vs_oracle.py): random worlds (sizes
1 x 2 to 44 x 44, terminals, rewards of either sign, walls, blocked transitions, wind, start
lists), hyper-parameters, batch sizes 0..130, 1..257 instances, masks, episodic replay, second
sessions, forced general kernel / row-streaming SR kernel — every table, counter and per-trial
monitor of DynaQ / QAgent / SR bit for bit against the C oracle.  The sweep found, in its first
300 cases: QAgent sessions with batch_size 0 did not log their experiences (the reference does,
q.py:213), and SR's transition table was not initialised for worlds of fewer than four states.
Below it: slices of the sweeps for SFMA, topologies, stochastic worlds, the network agents and their
kernels.  The sweeps for PMA, AssociativeNetwork, Continuous2D and MFEC have their slices in
tests/test_gpu_fuzz_agents.py (what those contain: tests/test_host_fuzz_agents.py); several hundred
seeds of each beyond the slice found no mismatch (docs/MEASUREMENTS.md section 20), so there is no
regression case of theirs next to test_sweep_regressions.  The tabular policy kernel (Softmax,
ExclusiveEpsilonGreedy and RandomDiscrete for QAgent and DynaQ, csrc/tabular_policy.hip), which none
of the sweeps above reaches — they all build EpsilonGreedy agents —, has scripts/fuzz_tabpol.py:
its slices are tests/test_gpu_fuzz_tabpol.py (what they contain: tests/test_host_fuzz_tabpol.py),
its first thousand seeds found no mismatch (docs/MEASUREMENTS.md section 35)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('first', [0, 60, 120, 180])
def test_random_cases_match_the_oracle(first):
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import fuzz_vs_oracle as fz
    failed = []
    for seed in range(first, first + 60):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


@pytest.mark.parametrize('first', [0, 50])
def test_random_sfma_cases_match_the_restatement(first):
    """scripts/fuzz_sfma.py: random worlds, metrics (DR / SR / Euclidean), the seven replay modes
    and every memory / agent switch; three instances per case re-run by oracle/sfma_loop.py —
    latencies, every reactivation with its TD error, Q, model tables, strengths, recency."""
    import fuzz_sfma as fz
    failed = []
    for seed in range(first, first + 50):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


def test_random_topologies_match_the_restatement():
    """scripts/fuzz_topology.py: QAgent on random graphs with 1..8 and 9..32 actions (four: wavefront
    kernels, up to eight: k_tab_wqn / the general kernel, beyond: its wide instantiations), replay
    batches 0..70, against oracle/ref_loop.py."""
    import fuzz_topology as fz
    failed = []
    for seed in list(range(0, 120)) + list(range(1_000_000, 1_000_040)):   # (from 10^6: 9..32 actions)
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


def test_random_stochastic_worlds_match_the_restatement():
    """scripts/fuzz_stochastic.py: gridworlds whose sas rows are edited into random distributions,
    Dyna-Q / Q-learning through the general kernel against oracle/ref_loop.py drawing successors
    the way the reference does."""
    import fuzz_stochastic as fz
    failed = []
    for seed in range(0, 100):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


def test_random_network_agent_runs_fused_equal_torch_loops():
    """scripts/fuzz_network_agents.py: DQN on random tracks, Dyna-DQN and Dyna-DSR on random
    gridworlds — the fused HIP loops against the PyTorch-ROCm loops of the same classes: rings /
    model tables, counters and monitors exactly, every network to float64 round-off."""
    import fuzz_network_agents as fz
    failed = []
    for seed in range(0, 40):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


def test_network_kernels_over_input_and_output_widths():
    """A slice of scripts/fuzz_networks.py: cobel_dqn_replay at input widths the fixed tests do not
    visit, cobel_mlp_forward / cobel_mlp_fit at random (inputs, outputs) pairs."""
    import torch
    import test_gpu_mlp
    import test_gpu_parity
    for n_in, dtype_name, ddqn in ((2, 'f64', True), (13, 'f64', False), (17, 'f32', True),
                                   (31, 'f64', True), (32, 'f64', False), (12, 'f32', True)):
        for kernel in (None, 'stream'):
            test_gpu_parity.test_fused_dqn_replay_equals_torch_path(torch, dtype_name, n_in, ddqn,
                                                                    kernel, f32_atol=1e-4)
    for D, O, dtype_name in ((1, 1, 'f64'), (1, 32, 'f64'), (32, 1, 'f64'), (7, 29, 'f64'),
                             (31, 18, 'f32'), (19, 5, 'f64'), (30, 31, 'f64')):
        test_gpu_mlp.test_mlp_forward_and_fit_match_pytorch(torch, D, O, dtype_name, f32_atol=1e-4)


def test_sweep_regressions():
    """The two cases the sweep caught, spelled out."""
    import numpy as np
    import torch
    from cobel_amd.agent import SR, QAgent
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_gridworld
    from cobel_amd.policy import EpsilonGreedy
    # SR on a three-state corridor: T starts as the identity for every (state, action)
    world = make_gridworld(1, 3, terminals=[0], rewards=np.array([[0, 1.0]]), goals=[0])
    env = Gridworld(world, n_envs=5, seed=1)
    sr = SR(env.observation_space, env.action_space, EpsilonGreedy(1.0))
    sr.train(env, 1, 1)
    T = sr._T.cpu().numpy()
    untouched = T[:, 0, :]                    # the terminal state is never left
    assert (untouched == 0).all() and set(np.unique(T[:, 2, :])) <= {1, 2}
    assert (T[:, 1, :] <= 2).all() and (T[:, 1, 1] == 1).all() and (T[:, 1, 3] == 1).all()
    # QAgent without replay still fills its memory, and a later session replays from all of it
    world = make_gridworld(3, 3, terminals=[8], rewards=np.array([[8, 1.0]]), goals=[8])
    for n in (1, 70):                         # wave-per-instance and lane-per-instance kernels
        env = Gridworld(world, n_envs=n, seed=3)
        ag = QAgent(env.observation_space, env.action_space, EpsilonGreedy(0.3))
        ag.track_instances = True
        ag.train(env, 4, 12, 0)
        torch.cuda.synchronize()
        steps = ag.monitors.lat_trace[:, :4].cpu().numpy() + 1
        assert np.array_equal(ag.inst[:, 6].cpu().numpy(), steps.sum(axis=1))
        assert len(ag.M) == int(steps[0].sum())
        first = ag.M[0]
        assert set(first) == {'state', 'action', 'reward', 'next_state', 'terminal'}
        ag.log_experiences = False            # opt out: the log stops growing at batch_size 0
        ag.train(env, 2, 12, 0)
        assert len(ag.M) == int(steps[0].sum())


def test_memory_facade_interleaved_with_training():
    """DynaQMemory.store / retrieve / retrieve_batch as host calls, interleaved at random with
    train() sessions (memory/dyna_q.py:77-157 next to agent/dyna_q.py:140-330), against
    oracle/ref_loop.py on the same streams: drawn batches, model tables, Q, latencies.  A
    rewarding experience stored BY HAND into the model of an agent that has not been rewarded
    yet must show up in planning at once (the kernel derives at launch whether there is anything
    to plan from the tables as it finds them)."""
    import numpy as np
    import torch
    from conftest import SEED
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_gridworld
    from cobel_amd.policy import EpsilonGreedy
    from oracle import ref_loop
    from oracle.philox import STREAM_ENV, STREAM_MEMORY, STREAM_POLICY, TapeRNG
    propagated = 0
    for seed in range(24):
        r = np.random.default_rng(seed)
        h, w = int(r.integers(2, 6)), int(r.integers(2, 6))
        S = h * w
        goal = int(r.integers(0, S))
        world = make_gridworld(h, w, terminals=[goal], rewards=np.array([[goal, 0.0]]), goals=[goal])
        inst = int(r.integers(0, 50))        # (no reward anywhere in the world: only hand-stored ones)
        env = Gridworld(world, seed=SEED, instance_base=inst)
        ag = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(0.2))
        ag.track_instances = True
        tab = dict(next=world['next'], reward=world['rewards'], terminal=world['terminals'],
                   starts=world['starting_states'])
        renv = ref_loop.RefGridworld(tab, TapeRNG(SEED, inst, STREAM_ENV))
        pol = ref_loop.RefEpsilonGreedy(0.2, TapeRNG(SEED, inst, STREAM_POLICY))
        ref = ref_loop.RefDynaQ(S, 4, pol, TapeRNG(SEED, inst, STREAM_MEMORY), dtype=np.float32)
        ag.train(env, 1, 3, 4)               # binds the tables
        ref.train(renv, 1, 3, 4)
        trials = 1
        for _ in range(int(r.integers(3, 9))):
            op = r.choice(['store', 'store', 'train', 'batch', 'retrieve'])
            if op == 'store':
                s, a, ns = int(r.integers(0, S)), int(r.integers(0, 4)), int(r.integers(0, S))
                rew, nt = float(r.choice([1.0, -0.5, 0.0, 2.0])), int(r.integers(0, 2))
                ag.M.store({'state': s, 'action': a, 'reward': rew, 'next_state': ns, 'terminal': nt})
                ref.M.store(s, a, np.float32(rew), ns, nt)
            elif op == 'train':
                t, st, B = int(r.integers(1, 4)), int(r.integers(2, 15)), int(r.choice([1, 8, 32, 70]))
                ag.train(env, t, st, B)
                ref.train(renv, t, st, B)
                trials += t
            elif op == 'batch':
                B = int(r.integers(1, 40))
                got = ag.M.retrieve_batch(B)
                want, _ = ref.M.sample(B)
                assert [(e['state'], e['action'], float(e['reward']), e['next_state'], e['terminal'])
                        for e in got] == [(int(a0), int(a1), float(a2), int(a3), int(a4))
                                          for a0, a1, a2, a3, a4 in want], seed
            else:
                s, a = int(r.integers(0, S)), int(r.integers(0, 4))
                e = ag.M.retrieve(s, a)
                assert (float(e['reward']), e['next_state'], e['terminal']) == \
                    (float(ref.M.rewards[s, a]), int(ref.M.states[s, a]), int(ref.M.terminals[s, a]))
        torch.cuda.synchronize()
        assert np.array_equal(ag._q[0].cpu().numpy(), ref.Q), seed
        assert np.array_equal(np.asarray(ag.M.states), ref.M.states), seed
        assert np.array_equal(np.asarray(ag.M.terminals), ref.M.terminals), seed
        assert np.array_equal(np.asarray(ag.M.rewards, dtype=np.float32), ref.M.rewards), seed
        propagated += int(ref.Q.any())
    assert propagated >= 5       # hand-stored rewards did reach Q through planning
