"""Randomised parity sweep for SFMA's per-instance parameter sets: one launch sequence of the HIP
path (cobel_sfma_run with ``param_index``, through SFMA / SFMAMemory with array-valued attributes)
against the NumPy restatement (oracle/sfma_loop.py) run with each instance's own parameters.

    python scripts/fuzz_sfma_sets.py [first_seed] [count]

Per seed: one world, one launch form, launch-wide switches, 1 .. 8 parameter sets whose fourteen
values and mode are drawn, 3 .. 40 instances spread over them; three instances are re-run by the
restatement and compared — escape latencies, every replayed experience with its TD error, Q, the
memory's tables (rewards, states, strengths C, recency T) and the |TD| sum.
tests/test_gpu_fuzz_sfma_sets.py runs a fixed slice, tests/test_host_sfma_sets.py says what it holds.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'cobel-rl_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MODES = ('default', 'reverse', 'forward', 'blend_forward', 'blend_reverse', 'interpolate',
         'sweeping')
BASE_SET = dict(alpha=0.99, gamma=0.99, epsilon=0.1, model_lr=0.9, decay_inhibition=0.9,
                decay_strength=1.0, C_step=1.0, I_step=1.0, R_threshold=1e-6, beta=20.0,
                reward_modulation=1.0, blend=0.1, interpolation_fwd=0.5, interpolation_rev=0.5)
CHOICES = dict(alpha=[0.5, 0.7, 0.9, 1.0], gamma=[0.5, 0.8, 0.9, 0.95], epsilon=[0.0, 0.05, 0.3, 1.0],
               model_lr=[0.3, 0.5, 1.0], decay_inhibition=[0.5, 0.8, 0.99, 1.0],
               decay_strength=[0.5, 0.9, 0.97], C_step=[0.25, 0.5, 2.0], I_step=[0.1, 0.3, 0.6],
               R_threshold=[0.0, 1e-3, 0.05], beta=[1.0, 5.0, 9.0, 40.0],
               reward_modulation=[0.5, 2.0, 2.5], blend=[0.3, 0.6, 1.0],
               interpolation_fwd=[0.0, 0.2, 0.8], interpolation_rev=[0.2, 0.9, 1.0])
FORMS = ('auto', 'general', 'one_wave', 'stream')


def draw_case(seed: int) -> dict:
    r = np.random.default_rng(9_000_011 * seed + 3)
    if r.random() < 0.8:
        h, w = int(r.integers(2, 9)), int(r.integers(2, 9))
    else:
        h, w = int(r.integers(9, 17)), int(r.integers(9, 17))
    S = h * w
    goal = int(r.integers(0, S))
    rew = {goal: float(r.choice([1.0, 1.0, 2.0, 0.5, -1.0]))}
    for _ in range(int(r.choice([0, 0, 1, 2]))):
        rew[int(r.integers(0, S))] = float(r.choice([0.5, -0.5, 1.0, 0.25]))
    walls = []
    for _ in range(int(r.integers(0, 5))):
        a = int(r.integers(0, S))
        b = a + int(r.choice([-1, 1, -w, w]))
        if 0 <= b < S and not (abs(b - a) == 1 and a // w != b // w):
            walls += [(a, b), (b, a)]
    opts = {}
    for k in ('recency', 'C_normalize', 'D_normalize', 'deterministic', 'reward_mod_local',
              'reward_mod', 'state_mod', 'dynamic', 'start_replay'):
        if r.random() < 0.2:
            opts[k] = True
    if r.random() < 0.2:
        opts['R_normalize'] = False
    if r.random() < 0.2:
        opts['nb_replays'] = int(r.choice([1, 2, 3]))
    if r.random() < 0.2:
        opts['noreplay_trials'] = 1
    if r.random() < 0.2:
        opts['test_trials'] = int(r.integers(1, 3))
    n = int(r.choice([3, 12, 40]))
    n_sets = int(r.choice([1, 2, 3, 5, 8]))
    sets = []
    for _ in range(n_sets):
        s = dict(BASE_SET)
        for k, values in CHOICES.items():
            if r.random() < 0.4:
                s[k] = float(r.choice(values))
        s['mode'] = MODES[int(r.integers(0, len(MODES)))]
        sets.append(s)
    which = [int(x) for x in r.integers(0, n_sets, n)]
    which[0], which[-1] = 0, n_sets - 1
    return dict(seed=seed, h=h, w=w, goal=goal, rew=rew, walls=walls, opts=opts,
                metric=str(r.choice(['DR', 'SR', 'Euclidean'])),
                steps=int(r.integers(3, 40 if S <= 64 else 60)),
                B=int(r.choice([1, 4, 8, 16, 24])), trials=int(r.integers(1, 5)),
                n=n, base=int(r.choice([0, 1000, 1 << 18])), sets=sets, which=which,
                form=str(r.choice(FORMS, p=[0.55, 0.15, 0.1, 0.2])))


def describe(c: dict) -> str:
    varied = sorted({k for s in c['sets'] for k in CHOICES if s[k] != BASE_SET[k]})
    return ('seed %(seed)d %(h)dx%(w)d %(metric)s form=%(form)s n=%(n)d base=%(base)d '
            'trials=%(trials)d steps=%(steps)d B=%(B)d' % c
            + ' sets=%d modes=%s varied=%s rew=%s walls=%d opts=%s'
            % (len(c['sets']), [s['mode'] for s in c['sets']], varied, c['rew'], len(c['walls']),
               c['opts']))


SKIPPED = []


def make_world(c: dict):
    """(the build's world or None if it has no start, metric.D)"""
    from cobel_amd.memory.utils import DR, SR, Euclidean
    from cobel_amd.misc.gridworld_tools import make_gridworld
    h, w = c['h'], c['w']
    rewards = np.array([[s, v] for s, v in c['rew'].items()], dtype=np.float64)
    world = make_gridworld(h, w, terminals=[c['goal']], rewards=rewards, goals=[c['goal']],
                           invalid_transitions=list(c['walls']))
    if len(world['starting_states']) == 0:
        return None, None
    if c['metric'] == 'DR':
        D = DR(w, h, world['next'], 0.9, world['invalid_transitions']).D
    elif c['metric'] == 'SR':
        D = SR(world['next'], 0.9).D
    else:
        D = Euclidean(w, h).D
    return world, D


def run_case(c: dict):
    import torch
    import sfma_sets_common as sc
    import test_gpu_sfma as T
    world, D = make_world(c)
    if world is None:
        return []
    opts = dict(c['opts'], mode='default')
    tab = dict(world.compact(), height=c['h'], width=c['w'], coordinates=world['coordinates'])
    cols = sc.columns(c['sets'], c['which'])
    env, agent = T.build(tab, D, opts, c['n'], c['base'], eps=cols['epsilon'])
    agent.learning_rate, agent.gamma = cols['alpha'], cols['gamma']
    agent.M.learning_rate = cols['model_lr']
    for k in sc.MEMORY:
        setattr(agent.M, k, cols[k])
    agent.M.mode = cols['mode']
    agent.force_general_kernel = c['form'] == 'general'
    agent.force_one_wave = c['form'] == 'one_wave'
    agent.force_stream_kernel = c['form'] == 'stream'
    T.run_schedule(env, agent, opts, c['trials'], c['steps'], c['B'])
    torch.cuda.synchronize()
    ow = T._oracle_world(world)
    total = c['trials'] + opts.get('noreplay_trials', 0) + opts.get('test_trials', 0)
    bad = []
    if not 1 <= agent.M._psets['agent']['n'] <= len(c['sets']):
        bad.append('%d sets on the device, %d drawn' % (agent.M._psets['agent']['n'], len(c['sets'])))
    for i in sorted({0, c['n'] // 2, c['n'] - 1}):
        p = c['sets'][c['which'][i]]
        try:
            ag = sc.oracle_run(ow, D, c['base'] + i, p, opts, c['trials'], c['steps'], c['B'])
        except ValueError as e:
            # NaN activation probabilities (0 / 0 strengths, overflowing exp without
            # R_normalize): the reference's rng.choice raises — nothing to compare with
            assert 'NaN' in str(e), e
            SKIPPED.append((c['seed'], i, 'reference raises'))
            continue
        if ag.M.nan_ratings:
            # deterministic mode walks on with NaN ratings (argmax = experience 0); the build
            # ends such a replay
            SKIPPED.append((c['seed'], i, 'NaN ratings'))
            continue

        def cmp(name, got, want, **kw):
            got, want = np.asarray(got), np.asarray(want)
            if got.shape != want.shape or not np.array_equal(got, want, **kw):
                bad.append('inst %d (set %d) %s' % (i, c['which'][i], name))

        def of(x):
            x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
            return x[i]

        cmp('steps', agent.monitors.lat_trace[i].cpu().numpy()[:total], ag.steps)
        rp = np.array(ag.replayed, dtype=np.float64).reshape(-1, 8)
        try:
            T.check_events(T.events_of(agent, i), rp)
        except AssertionError:
            bad.append('inst %d (set %d) replay events' % (i, c['which'][i]))
        cmp('Q', of(agent.Q), ag.Q)
        cmp('M.rewards', of(agent.M.rewards), ag.M.rewards)
        cmp('M.states', of(agent.M.states), ag.M.states)
        cmp('M.C', of(agent.M.C), ag.M.C)
        cmp('M.T', of(agent.M.T), ag.M.T)
        td = float(np.asarray(agent.td).reshape(-1)[i])
        if not (td == float(ag.td) or (np.isnan(td) and np.isnan(float(ag.td)))):
            bad.append('inst %d td' % i)
        if not opts.get('dynamic'):
            if agent.M.modes[i] != p['mode']:
                bad.append('inst %d mode' % i)
    return bad


def main() -> int:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    failed, t0 = [], time.time()
    for seed in range(first, first + count):
        c = draw_case(seed)
        try:
            bad = run_case(c)
        except Exception as e:
            bad = ['%s: %s' % (type(e).__name__, str(e)[:300])]
        if bad:
            failed.append(seed)
            print('MISMATCH', bad[:6], describe(c), flush=True)
        if (seed - first) % 10 == 9:
            print('... %d cases, %d failing, %.0f s' % (seed - first + 1, len(failed), time.time() - t0),
                  flush=True)
    print('cases %d, failing %d: %s; instances skipped because the reference has NaN ratings: %d'
          % (count, len(failed), failed, len(SKIPPED)))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
