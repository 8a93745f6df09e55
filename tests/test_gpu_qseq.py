"""GPU tests of QAgent on a Sequence (csrc/qseq.hip, agent/q_seq.py, policy/softmax.py): the device
against the traces recorded from the real reference, against the restatement of tests/qseq_common.py
at the seams of the packing, the stand-alone Softmax policy, and the grid search on top."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qseq_common as qc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qseq_traces.npz')

# The largest relative difference |p(device) - p(restatement)| / p(restatement) over the known-answer
# set — the rows of qseq_common.KAT_ROWS (1.24e-16) and the seeded random rows of
# test_softmax_batches_select_as_the_restatement (3.31e-16) — measured on an MI355X
# (docs/MEASUREMENTS.md section 24), and the bound: the next power of two above it.  The
# restatement's exp is np.exp, the reference's own; everything else in a probability is rounded
# alike on both sides, so a bound above 2^-48 would be a defect, not a tolerance.
PROB_MEASURED = 3.3071745509667795e-16
PROB_BOUND = 2.0 ** -51


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def q_array(ag, tuples, A) -> np.ndarray:
    q = np.zeros((len(tuples), A))
    for t, row in ag.Q_dict.items():
        q[tuples.index(t)] = row
    return q


STEP_KEYS = {'trial_reward', 'trial', 'trial_session', 'step', 'state', 'action', 'reward',
             'next_state', 'terminal', 'agent'}


# -- against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['none', 'trial', 'step'])
@pytest.mark.parametrize('name', sorted(qc.CASES))
def test_fixture_cases_one_instance(Z, name, mode):
    """n_envs = 1: one launch per session, per trial (trial callbacks) or per step (step callbacks);
    every recorded quantity equals the reference's bit for bit."""
    from cobel_amd.monitor import RewardMonitor
    c = qc.CASES[name]
    _, obs = c['design']()
    _, tuples = qc.keys_of(obs)
    A = c['nb_actions']
    g = lambda k: Z[name + '/' + k]      # noqa: E731
    steps_seen, trials_seen = [], []
    monitor = RewardMonitor(len(g('steps')))

    def on_step_end(logs):
        steps_seen.append(dict(logs))

    def on_trial_end(logs):
        trials_seen.append((dict(logs), q_array(logs['agent'], tuples, A)))

    cbs = {'none': None, 'trial': {'on_trial_end': [on_trial_end]},
           'step': {'on_step_end': [on_step_end, monitor.update], 'on_trial_end': [on_trial_end]}}[mode]
    ag, env = qc.device_case(name, callbacks=cbs)
    out = qc.device_record(ag, env, 0)
    qc.assert_same_record(out, Z, name + '/', what='%s (%s)' % (name, mode))
    assert np.array_equal(out['Q_final'], g('Q')[-1])
    # Q_dict: exactly the keys the reference's dict holds, in its order, and its values
    assert [tuples.index(t) for t in ag.Q_dict] == g('created').tolist()
    assert np.array_equal(q_array(ag, tuples, A), g('Q')[-1])
    assert all(v.dtype == np.float64 and v.shape == (A,) for v in ag.Q_dict.values())
    assert list(ag.Q) == list(ag.Q_dict)      # (one instance: `Q` is the reference's dict)
    # M in the reference's form
    M = ag.M
    assert len(M) == int(g('len_M'))
    assert [[tuples.index(e['state']), e['action'], tuples.index(e['next_state']), e['terminal']]
            for e in M] == g('M').tolist()
    assert np.array_equal([e['reward'] for e in M], g('M_reward'))
    assert ag.current_trial == len(g('steps'))
    seen = np.array([tuples[k] for k in g('created')])
    assert np.array_equal(ag.predict_on_batch(seen), g('Q')[-1][g('created')])
    with pytest.raises(KeyError):
        ag.predict_on_batch(np.full((1, seen.shape[1]), 0.123))
    last = np.cumsum(g('steps') + 1) - 1       # index of every trial's last step
    if mode == 'none':
        return
    # per trial: Q as the reference's dict held it, logs['steps'], the trial reward, the last step
    assert len(trials_seen) == len(g('steps'))
    learn = np.concatenate([[kind == 'train'] * trials for kind, trials, _, _ in c['sessions']])
    for t, (logs, q) in enumerate(trials_seen):
        assert np.array_equal(q, g('Q')[t]), 'Q after trial %d' % t
        assert logs['steps'] == g('steps')[t] and logs['trial'] == t
        assert logs['trial_reward'] == g('trial_reward')[t]
        assert logs['action'] == g('action')[last[t]] and logs['reward'] == g('reward')[last[t]]
        assert logs['terminal'] == 1 - int(g('end')[last[t]])
        assert ('td' in logs) == bool(learn[t])
        if learn[t]:
            assert logs['td'] == g('td')[last[t]]
    if mode == 'trial':
        return
    # per step: the reference's log keys and values
    assert len(steps_seen) == len(g('action'))
    trial_of = np.repeat(np.arange(len(last)), g('steps') + 1)
    for k, logs in enumerate(steps_seen):
        assert set(logs) == STEP_KEYS | ({'td'} if learn[trial_of[k]] else set()), k
        assert logs['action'] == g('action')[k] and logs['reward'] == g('reward')[k]
        assert logs['terminal'] == 1 - int(g('end')[k]) and logs['trial'] == trial_of[k]
        assert type(logs['state']) is tuple and type(logs['next_state']) is tuple
        if learn[trial_of[k]]:
            assert logs['td'] == g('td')[k]
    trained = [k for k in range(len(steps_seen)) if learn[trial_of[k]]]
    assert [[tuples.index(steps_seen[k]['state']), tuples.index(steps_seen[k]['next_state'])]
            for k in trained] == g('M')[:, [0, 2]].tolist()
    # the demo's monitor, registered under on_step_end: its trace is the trial rewards
    assert np.array_equal(monitor.get_trace(), g('trial_reward'))


# -- against the restatement, at the seams of the packing -------------------------------------------
# (n instances, actions, keys, batch size, seed): the group (1), the wavefront (8 instances) and the
# workgroup (32 instances) with one fewer and one more; one, three and eight actions; two keys and
# sixty-four; batches around the eight lanes of a group and around the 32 records gathered at a time
SWEEP = [(1, 8, 5, 32, 11), (7, 3, 5, 7, 12), (8, 1, 2, 8, 13), (9, 8, 64, 9, 14), (33, 3, 5, 1, 15),
         (33, 8, 5, 40, 16), (9, 3, 64, 0, 17), (8, 8, 2, 33, 18)]


def sweep_setup(n, A, keys, B, seed):
    rng = np.random.default_rng(seed)
    schedules, obs = qc.random_design(rng, 3, 6, 3, A, keys - 1)
    ids = rng.choice(5000, n, replace=False)
    par = dict(lr=np.round(rng.uniform(0.1, 1.0, n), 3), gamma=np.round(rng.uniform(0.0, 0.95, n), 3),
               beta=rng.choice([0.25, 1.0, 5.0, 10.0], n))
    sessions = [('train', 3, 2, B), ('train', 3, 3, B)]
    return schedules, obs, ids, par, sessions


@pytest.mark.parametrize('n,A,keys,B,seed', SWEEP)
def test_batches_against_the_restatement(n, A, keys, B, seed):
    """Several schedules of different trial lengths in one launch, arbitrary instance numbers,
    per-instance learning rate, gamma and beta, a session cut into two train calls across a growth
    of the log: every instance equals its own restatement with np.array_equal."""
    schedules, obs, ids, par, sessions = sweep_setup(n, A, keys, B, seed)
    ag, env = qc.device_run(schedules, obs, A, False, ('softmax', 1.0), None, par['lr'], par['gamma'],
                            sessions, n_envs=n, instance_ids=ids, policy_value=par['beta'])
    assert len(ag._seq.key_obs) == keys and ag.trial_reward_trace.shape == (n, 6)
    assert n == 1 or tuple(ag.Q.shape) == (n, keys, A)
    assert ag._seq._log_cap >= int(ag._seq._log_len.max().item())
    qc.compare_instances(ag, env, schedules, obs, A, ('softmax', 1.0), par['lr'], par['gamma'],
                         sessions, ids, policy_value=par['beta'], what=str((n, A, keys, B)))
    assert ag.env_steps() == int(ag._seq._log_len.sum().item())


def test_eps_greedy_batch_against_the_restatement():
    n, A = 9, 4
    rng = np.random.default_rng(21)
    schedules, obs = qc.random_design(rng, 2, 8, 2, A, 3)
    ids = np.arange(100, 100 + n)
    eps = np.round(rng.uniform(0.0, 1.0, n), 2)
    sessions = [('train', 8, 2, 5)]
    ag, env = qc.device_run(schedules, obs, A, False, ('eps', 0.1), None, 1.0, 0.5, sessions, n_envs=n,
                            instance_ids=ids, policy_value=eps)
    qc.compare_instances(ag, env, schedules, obs, A, ('eps', 0.1), 1.0, 0.5, sessions, ids,
                         policy_value=eps, what='eps-greedy')


def test_an_instance_of_a_batch_equals_the_same_instance_alone_and_step_launches_one_launch():
    n, A, keys, B, seed = 9, 8, 5, 9, 31
    schedules, obs, ids, par, sessions = sweep_setup(n, A, keys, B, seed)
    ag, env = qc.device_run(schedules, obs, A, False, ('softmax', 1.0), None, par['lr'], par['gamma'],
                            sessions, n_envs=n, instance_ids=ids, policy_value=par['beta'])
    for i in range(n):
        for cbs in (None, {'on_step_begin': [lambda logs: None]}):    # one launch / one per step
            one, e1 = qc.device_run(schedules[int(env.schedule_of[i])], obs, A, False,
                                    ('softmax', float(par['beta'][i])), None, float(par['lr'][i]),
                                    float(par['gamma'][i]), sessions, instance_base=int(ids[i]),
                                    callbacks=cbs)
            a, b = qc.device_record(ag, env, i), qc.device_record(one, e1, 0)
            for k in a:
                assert np.array_equal(a[k], b[k]), (i, k)


def test_sentinel_frames_around_q_log_and_traces():
    """Q, the log and the per-trial traces sit inside larger buffers filled with a sentinel: the
    kernel writes nothing outside its own."""
    import torch
    n, A, keys, B, seed = 33, 3, 5, 9, 41
    schedules, obs, ids, par, sessions = sweep_setup(n, A, keys, B, seed)
    ag, env = qc.device_run(schedules, obs, A, False, ('softmax', 1.0), None, par['lr'], par['gamma'],
                            [('train', 0, 2, B)], n_envs=n, instance_ids=ids,
                            policy_value=par['beta'], record=0)
    h = ag._seq
    h.reserve_replay(3 * 2 + 3 * 3)      # (the steps the two sessions can take at the most)
    h._reserve(6)
    frames = {}

    def framed(t, fill):
        big = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
        big[1:-1] = t
        return big

    for name, fill in (('_q', 777.0), ('_log', 0x5A5A5A5A5A5A5A5A), ('trial_reward_trace', 777.0),
                       ('trial_steps_trace', 0x5A5A5A5A), ('_last', 777.0), ('_trew', 777.0)):
        frames[name] = (framed(getattr(h, name), fill), fill)
        setattr(h, name, frames[name][0][1:-1])
    for kind, trials, steps_cap, batch in sessions:
        ag.train(env, trials, steps_cap, batch)
    for name, (big, fill) in frames.items():
        assert getattr(h, name).data_ptr() == big[1:-1].data_ptr(), name + ' was reallocated'
        assert bool((big[0] == fill).all()) and bool((big[-1] == fill).all()), name
    # the log beyond every instance's length is untouched as well
    lens = h._log_len.cpu().numpy()
    log = h._log.cpu().numpy()
    assert all((log[i, lens[i]:] == 0).all() for i in range(n))
    ag.record_steps = 0
    refs = [qc.restate(schedules[int(env.schedule_of[i])], obs, A, False,
                       ('softmax', float(par['beta'][i])), None, float(par['lr'][i]),
                       float(par['gamma'][i]), sessions, int(ids[i])) for i in range(n)]
    q = h._q.cpu().numpy()
    for i, ref in enumerate(refs):
        assert ref['margin'] > qc.MARGIN
        assert np.array_equal(q[i], ref['Q'][-1]), i
        assert lens[i] == ref['len_M']


# -- the stand-alone policy -------------------------------------------------------------------------
def test_softmax_known_answers(Z):
    """cobel_softmax_n through Softmax: the reference's probabilities within the bound, exact zeros
    at beta = 1e4 without a NaN, uniform probabilities for equal values, masks, and the draw at both
    ends of [0, 1)."""
    from cobel_amd.policy import Softmax
    worst = 0.0
    for name, (v, mask, beta) in qc.KAT_ROWS.items():
        pol = Softmax(beta)
        m = None if mask is None else np.array(mask, dtype=bool)
        p = pol.get_action_probs(np.array(v), m)
        want, ref = qc.softmax_probs(v, beta, mask), Z['probs/' + name]
        assert p.shape == want.shape and p.dtype == np.float64 and not np.isnan(p).any(), name
        assert np.array_equal(p == 0, want == 0) and np.array_equal(p == 0, ref == 0), name
        nz = want != 0
        rel = float((np.abs(p[nz] - want[nz]) / want[nz]).max())
        worst = max(worst, rel)
        print('%-12s largest relative difference device / restatement %.17g' % (name, rel))
        # (the reference adds eight values pairwise, the device in action order: one more rounding)
        assert np.all(np.abs(p - ref) <= (PROB_BOUND + 2.0 ** -52) * ref), name
        allowed = np.flatnonzero(p > 0)
        assert pol.select_action(np.array(v), m, u=0.0) == allowed[0], name
        assert pol.select_action(np.array(v), m, u=1.0 - 2.0 ** -53) == allowed[-1], name
        if mask is not None:
            assert np.array_equal(p[~m], np.zeros((~m).sum())), name
    print('known-answer set: largest relative difference %.17g, bound %.17g' % (worst, PROB_BOUND))
    assert worst <= PROB_BOUND
    assert PROB_MEASURED <= PROB_BOUND <= 2 * PROB_MEASURED or PROB_MEASURED == 0.0
    assert PROB_BOUND <= 2.0 ** -48
    assert np.array_equal(Softmax(1.0).get_action_probs(np.full(8, 0.5)), np.full(8, 0.125))
    assert np.array_equal(Softmax(5.0).get_action_probs(np.full(4, -2.0)), np.full(4, 0.25))
    assert np.array_equal(Softmax(1e4).get_action_probs(np.array([0.7, -0.3, 0.7, 0.0])),
                          [0.5, 0.0, 0.5, 0.0])
    assert Softmax().select_action(np.array([0.3])) == 0
    with pytest.raises(AssertionError):
        Softmax().get_action_probs(np.zeros(3), np.zeros(3, dtype=bool))


def test_softmax_batches_select_as_the_restatement():
    """Rows of 1 .. 8 actions with one beta per row and injected draws: the action is the
    restatement's wherever the draw keeps the margin, the probabilities agree within the bound."""
    from cobel_amd.policy import Softmax
    rng = np.random.default_rng(3)
    worst = 0.0
    for A in range(1, 9):
        N = 67
        v = rng.normal(size=(N, A))
        v[::5] = np.round(v[::5])                 # exact ties
        beta = rng.choice([1e-3, 0.25, 1.0, 5.0, 10.0, 1e4], N)
        mask = rng.random((N, A)) < 0.7
        mask[np.arange(N), rng.integers(0, A, N)] = True
        u = rng.random(N)
        pol = Softmax(beta)
        p = pol.get_action_probs(v, mask)
        act = pol.select_action(v, mask, u=u).cpu().numpy()
        checked = 0
        for i in range(N):
            want = qc.softmax_probs(v[i], beta[i], mask[i])
            assert np.array_equal(p[i] == 0, want == 0), (A, i)
            nz = want != 0
            worst = max(worst, float((np.abs(p[i][nz] - want[nz]) / want[nz]).max()))
            cdf = qc.cdf_of(want)
            if A == 1 or np.abs(cdf[:-1] - u[i]).min() > qc.MARGIN:
                assert act[i] == qc.choose(want, u[i]), (A, i)
                checked += 1
        assert checked >= N - 1
    print('random rows: largest relative difference %.17g' % worst)
    assert worst <= PROB_BOUND
    # the policy's own draws: one double per selection from its stream and counter
    pol = Softmax(1.0, rng=5)
    a = pol.select_action(np.zeros((4, 3)))
    assert a.shape == (4,) and pol.counter.tolist() == [1, 1, 1, 1]


# -- the grid search on top -------------------------------------------------------------------------
def test_fit_vectorised_equals_fit_run_by_run(tmp_path):
    """A 2 x 2 grid with 3 runs of 24 trials: one launch of 12 instances gives exactly the losses of
    ``fit`` with a sequential simulation that runs each instance alone under the same number."""
    from cobel_amd.agent import QAgent
    from cobel_amd.interface import Sequence
    from cobel_amd.optimizer import GridSearchOptimizer
    from cobel_amd.optimizer.grid_search import spread_over_instances
    from cobel_amd.policy import Softmax
    from cobel_amd.spaces import Box
    schedule, obs = qc.demo_design(6)
    trials, runs, seed = len(schedule), 3, 77
    parameters = {'learning_rate': [0.3, 0.9], 'beta': [1, 5]}

    def make(n, ids, lr, beta):
        env = Sequence(schedule, obs, Box(0.0, 1.0, (4,)), 8, n_envs=n, seed=seed, instance_ids=ids)
        ag = QAgent(env.observation_space, env.action_space, Softmax(beta), learning_rate=lr)
        ag.train(env, trials, 100)
        return ag.trial_reward_trace.cpu().numpy()

    data = {'demo': list(make(runs, np.arange(1000, 1000 + runs), 0.9, 1.0))}
    loss = lambda sim, dat: float(np.sum(np.sqrt((np.mean(sim['demo'], axis=0)      # noqa: E731
                                                   - np.mean(dat['demo'], axis=0)) ** 2)))
    launches = []

    def simulation_batch(task, combos, nb_runs):
        par, which = spread_over_instances(combos, nb_runs)
        launches.append(len(which))
        rows = make(len(which), np.arange(len(which)), par['learning_rate'].astype(np.float64),
                    par['beta'].astype(np.float64))
        return [list(rows[which == k]) for k in range(len(combos))]

    os.makedirs(tmp_path / 'a')
    os.makedirs(tmp_path / 'b')
    opt = GridSearchOptimizer(str(tmp_path / 'a') + '/', parameters, runs)
    fit_v = opt.fit_vectorised(simulation_batch, {'demo': None}, data, loss)
    assert launches == [12]
    order = list(opt.parameter_combinations)
    count = {}

    def simulation(task, params):
        key = (params['learning_rate'], params['beta'])
        run = count.get(key, 0)
        count[key] = run + 1
        inst = order.index(key) * runs + run
        return make(1, np.array([inst]), float(params['learning_rate']), float(params['beta']))[0]

    fit_s = GridSearchOptimizer(str(tmp_path / 'b') + '/', parameters, runs).fit(
        simulation, {'demo': None}, data, loss)
    assert list(fit_v) == list(fit_s) and len(fit_v) == 4
    for key in fit_v:
        assert fit_v[key] == fit_s[key], key
