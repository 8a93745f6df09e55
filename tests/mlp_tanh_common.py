"""The tanh form of cobel_dqn_replay (activation = 1) restated in plain float64 NumPy: Linear(D, 64)-
tanh-Linear(64, 64)-tanh-Linear(64, A).  Networks, moments and batches are the dicts of
tests/mlp_common.py, whose activation-free parts (adam, blend, the error measures, the struct
filler) are used as they are; what depends on the forward pass — ``forward``, ``grads``,
``dqn_targets``, ``dqn_step``, the top-two gap and the case builders that search for it — is said
again here with tanh.  The backward pass is the one the kernel is asked to perform:
delta_l = (delta_{l+1} W_{l+1}) * (1 - h_l * h_l).

tests/test_host_dqn_tanh.py checks this file against torch autograd + torch.optim.Adam in float64 on
the CPU; tests/test_gpu_dqn_replay_tanh.py checks the kernel against this file."""
import numpy as np

from mlp_common import (B, BATCH_KEYS, DQN_OPTIONS, GAP, H, KEYS, TABLE_ROWS,  # noqa: F401
                        adam, adam_from_moments, adam_kernel, blend, dqn_rows, draw_networks,
                        f32_bound, fill_dqn_replay, first_maximum, one, plant_tie, rel_err,
                        top_two_gap)

SATURATING_BIAS = 40.0      # tanh(40 + anything a drawn network adds) == 1.0 exactly in both dtypes


def forward(p, x):
    """h1, h2, q of one network on the rows of x [rows, D]."""
    h1 = np.tanh(x @ p['w1'].T + p['b1'])
    h2 = np.tanh(h1 @ p['w2'].T + p['b2'])
    return h1, h2, h2 @ p['w3'].T + p['b3']


def grads(p, x, y):
    """Gradient of the mean over the rows and the A outputs of (q - y)^2."""
    h1, h2, q = forward(p, x)
    rows, O = q.shape
    d3 = 2.0 * (q - y) / (rows * O)
    g = {'w3': d3.T @ h2, 'b3': d3.sum(axis=0)}
    d2 = (d3 @ p['w3']) * (1.0 - h2 * h2)
    g['w2'], g['b2'] = d2.T @ h1, d2.sum(axis=0)
    d1 = (d2 @ p['w2']) * (1.0 - h1 * h1)
    g['w1'], g['b1'] = d1.T @ x, d1.sum(axis=0)
    return g


def dqn_targets(p_online, p_target, x_next, rewards, nonterminal, gamma, ddqn):
    """mlp_common.dqn_targets on the tanh network."""
    qt = forward(p_target, x_next)[2]
    if ddqn:
        pick = first_maximum(forward(p_online, x_next)[2].T[None])[0]
        boot = qt[np.arange(qt.shape[0]), pick]
    else:
        boot = qt.max(axis=1)
    nt = np.asarray(nonterminal, dtype=np.float64)
    boot = np.where(nt != 0, boot, 0.0)
    return np.asarray(rewards, dtype=np.float64) + (boot * nt) * gamma


def dqn_step(net, batch, hyper, gamma, ddqn, obs=None):
    """mlp_common.dqn_step on the tanh network: the new state, the gradient and q_out."""
    x = np.asarray(batch['states'], dtype=np.float64)
    new = dqn_targets(net['p'], net['t'], np.asarray(batch['next_states'], dtype=np.float64),
                      batch['rewards'], batch['nonterminal'], gamma, ddqn)
    y = forward(net['p'], x)[2].copy()
    y[np.arange(y.shape[0]), np.asarray(batch['actions'])] = new
    g = grads(net['p'], x, y)
    out = dict(net)
    out['p'], out['m'], out['v'] = adam(net['p'], net['m'], net['v'], g, net['steps'], hyper['lr'],
                                        hyper['beta1'], hyper['beta2'], hyper['eps'],
                                        hyper['weight_decay'])
    if hyper['tau'] != 0.0:
        out['t'] = blend(net['t'], out['p'], hyper['tau'])
    q_out = None if obs is None else forward(out['p'], np.asarray(obs, dtype=np.float64)[None])[2][0]
    return out, g, q_out


def dqn_gap(p_online, p_target, x_next, ddqn):
    """The top-two gap of Q_target(s') and, with ``ddqn``, of Q_online(s') on the tanh network."""
    gap = top_two_gap(forward(p_target, x_next)[2])
    return min(gap, top_two_gap(forward(p_online, x_next)[2])) if ddqn else gap


def _draw(case, s, ddqn, online, target, plant):
    """mlp_common._dqn_draw with the gap of the tanh network."""
    n, D, A, dt = case['n'], case['D'], case['A'], case['dtype']
    rng = np.random.default_rng([s, 0xD0])
    case['table'] = rng.standard_normal((TABLE_ROWS, D))
    case['state_index'] = rng.integers(0, TABLE_ROWS, size=(n, B)).astype(np.int32)
    case['next_index'] = rng.integers(0, TABLE_ROWS, size=(n, B)).astype(np.int32)
    case['actions'] = rng.integers(0, A, size=(n, B)).astype(np.int64)
    case['rewards'] = rng.uniform(-1.0, 1.0, size=(n, B)).astype(dt)
    case['nonterminal'] = (rng.random((n, B)) < 0.8).astype(dt)
    case['exempt'] = set(plant(case)) if plant else set()
    nets_o = online or [one(case['P'], j) for j in range(n)]
    nets_t = target or [one(case['T'], j) for j in range(n)]
    return all(j in case['exempt'] or
               dqn_gap(nets_o[j], nets_t[j], dqn_rows(case, j)['next_states'], ddqn) >= GAP
               for j in range(n))


def dqn_draw_batch(case, seed, ddqn, online, target, tries=64):
    """A new table and batch for a case whose networks have moved on (mlp_common.dqn_draw_batch)."""
    for s in range(seed, seed + tries):
        if _draw(case, s, ddqn, online, target, None):
            return s
    raise AssertionError('no seed in %d .. %d keeps the top-two gap' % (seed, seed + tries - 1))


def dqn_case(seed, n, D, A, dtype, ddqn=True, zero_moments=False, steps=None, plant=None, tries=64):
    """mlp_common.dqn_case for the tanh network: the same draws, the first seed whose top-two gap
    (dqn_gap here) is at least GAP for every sample of every instance that ``plant`` does not
    exempt."""
    for s in range(seed, seed + tries):
        rng = np.random.default_rng(s)
        case = {'n': n, 'D': D, 'A': A, 'dtype': np.dtype(dtype).type, 'seed': s}
        case['P'] = draw_networks(rng, n, D, A, dtype)
        case['T'] = draw_networks(rng, n, D, A, dtype)
        case['M'] = {k: (0.0 if zero_moments else 0.01) * rng.standard_normal(a.shape).astype(dtype)
                     for k, a in case['P'].items()}
        case['V'] = {k: ((0.0 if zero_moments else 1e-4) * rng.uniform(0.05, 1.0, a.shape)).astype(dtype)
                     for k, a in case['P'].items()}
        case['steps'] = (np.resize(np.array([1.0, 2.0, 5.0, 1000.0, 3.0, 7.0, 17.0]), n)
                         if steps is None else np.asarray(steps, dtype=np.float64) * np.ones(n))
        if _draw(case, s, ddqn, None, None, plant):
            return case
    raise AssertionError('no seed in %d .. %d keeps the top-two gap' % (seed, seed + tries - 1))


def plant_ties(case):
    """Instance 0: Q_online(s') all equal; 1: the maximum twice (the first and the last action) —
    zero rows of w3 and equal b3, so exact in any summation order, and the target network rates the
    tied actions differently: only the FIRST maximum gives the reference's target."""
    A = case['A']
    plant_tie(case['P'], 0, range(A), 0.3)
    plant_tie(case['P'], 1, sorted({0, A - 1}), 10.0)
    return {0, 1}


SATURATED = (5, 9)          # the hidden unit of layer 1 / of layer 2 that plant_saturation pins at 1.0


def plant_saturation(case):
    """Every instance: unit SATURATED[0] of the first and SATURATED[1] of the second hidden layer
    get the bias 40, so their activations are exactly 1.0 on every row in both dtypes and
    1 - h * h is exactly 0: nothing may flow back through them."""
    case['P']['b1'][:, SATURATED[0]] = SATURATING_BIAS
    case['P']['b2'][:, SATURATED[1]] = SATURATING_BIAS
    return ()


SHAPES = [(2, 4), (3, 3), (6, 4), (9, 3), (32, 8)]       # (D, A) of tests/test_gpu_dqn_replay_tanh.py


def gpu_cases(D, A):
    """Every case tests/test_gpu_dqn_replay_tanh.py draws at one shape, by key: the arguments of
    dqn_case.  tests/test_host_dqn_tanh.py draws each of them in both dtypes, so that a search that
    fails is found without a GPU."""
    cases = {}
    for ddqn in (False, True):
        cases['backward', ddqn] = dict(seed=100 * D + 10 * A + ddqn, n=5, ddqn=ddqn,
                                       zero_moments=True, steps=1.0)
    cases['ties'] = dict(seed=200 * D + 10 * A, n=3, ddqn=True, plant=plant_ties)
    cases['saturation'] = dict(seed=250 * D + 10 * A, n=3, ddqn=False, zero_moments=True, steps=1.0,
                               plant=plant_saturation)
    cases['modes'] = dict(seed=400 * D + 10 * A, n=5, ddqn=True)
    cases['sit_out'] = dict(seed=500 * D + 10 * A, n=7, ddqn=False)
    for k, option in enumerate(DQN_OPTIONS):
        cases['options', option] = dict(seed=1000 * (1 + k) + 20 * D + A, n=5, ddqn=option == 'ddqn',
                                        steps=[1.0, 1e6, 1.0, 1e6, 2.0] if option == 'steps' else None)
    cases['q_out'] = dict(seed=600 * D + 10 * A, n=5, ddqn=False)
    return cases


def gpu_case(key, D, A, dtype):
    return dqn_case(D=D, A=A, dtype=dtype, **gpu_cases(D, A)[key])
