"""A plain float64 restatement of what csrc/mlp_fit.hip, csrc/mlp.hip and csrc/dsr_targets.hip
compute, in NumPy only (no torch, no project code), and the helpers that fill the launch structs of
cobel_mlp_forward / cobel_mlp_fit / cobel_dsr_targets / cobel_dqn_replay from dicts of tensors.

A network is a dict ``{'w1': [64, D], 'b1': [64], 'w2': [64, 64], 'b2': [64], 'w3': [O, 64],
'b3': [O]}`` — Linear(D, 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, O), weights as torch.nn.Linear
keeps them ([out][in]).  Moments and gradients are dicts of the same shape.  Every function returns
new arrays and leaves its arguments alone.

tests/test_host_mlp_reference.py checks this file against torch autograd + torch.optim.Adam in
float64 on the CPU; tests/test_gpu_mlp_edges.py and tests/test_gpu_dqn_replay_edges.py check the
kernels against this file."""
import numpy as np

KEYS = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
H, B = 64, 32                        # hidden units, samples per batch
F32_EPS = 2.0 ** -24                 # unit round-off of float32
F32_FLOOR = 64 * F32_EPS             # the plain bound of a 64-term float32 sum, relative
F32_FACTOR = 4.0                     # a different summation order, nothing else


# ---------------------------------------------------------------------------------------------
# the network
def forward(p, x):
    """h1, h2, q of one network on the rows of x [rows, D]."""
    h1 = np.maximum(x @ p['w1'].T + p['b1'], 0.0)
    h2 = np.maximum(h1 @ p['w2'].T + p['b2'], 0.0)
    return h1, h2, h2 @ p['w3'].T + p['b3']


def shapes(D, O):
    return {'w1': (H, D), 'b1': (H,), 'w2': (H, H), 'b2': (H,), 'w3': (O, H), 'b3': (O,)}


def draw_networks(rng, n, D, O, dtype):
    """n networks as stacked arrays [n, ...] in ``dtype``, drawn as torch.nn.Linear draws them
    (uniform in +- 1 / sqrt(fan_in))."""
    fan_in = {'w1': D, 'b1': D, 'w2': H, 'b2': H, 'w3': H, 'b3': H}
    return {k: rng.uniform(-1.0, 1.0, size=(n,) + s).astype(dtype) / np.sqrt(fan_in[k]).astype(dtype)
            for k, s in shapes(D, O).items()}


def one(stack, j):
    """Network j of a stack, in float64."""
    return {k: np.asarray(a[j], dtype=np.float64) for k, a in stack.items()}


def grads(p, x, y, mask=None):
    """Gradient of  sum over the marked samples s and the O outputs of (q - y)^2 / (max(count, 1) O)
    (mask None: all samples), the backward pass written out."""
    h1, h2, q = forward(p, x)
    rows, O = q.shape
    on = np.ones(rows) if mask is None else (np.asarray(mask) != 0).astype(np.float64)
    count = max(int(on.sum()), 1)
    d3 = 2.0 * (q - y) * on[:, None] / (count * O)
    g = {'w3': d3.T @ h2, 'b3': d3.sum(axis=0)}
    d2 = (d3 @ p['w3']) * (h2 > 0)
    g['w2'], g['b2'] = d2.T @ h1, d2.sum(axis=0)
    d1 = (d2 @ p['w2']) * (h1 > 0)
    g['w1'], g['b1'] = d1.T @ x, d1.sum(axis=0)
    return g


def adam(p, m, v, g, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam (no amsgrad) with ``step`` the count INCLUDING this step: returns the new
    parameters, first and second moments."""
    pn, mn, vn = {}, {}, {}
    step_size = lr / (1.0 - b1 ** step)
    bc2_sqrt = np.sqrt(1.0 - b2 ** step)
    for k in p:
        gk = g[k] + wd * p[k]
        mn[k] = m[k] + (1.0 - b1) * (gk - m[k])
        vn[k] = b2 * v[k] + (1.0 - b2) * gk * gk
        denom = np.sqrt(vn[k]) / bc2_sqrt + eps
        pn[k] = p[k] - step_size * (mn[k] / denom)
    return pn, mn, vn


def adam_from_moments(p, m_new, v_new, step, lr, b1, b2, eps):
    """The parameter update of ``adam`` alone, from moments that are already updated."""
    step_size, bc2_sqrt = lr / (1.0 - b1 ** step), np.sqrt(1.0 - b2 ** step)
    return {k: p[k] - step_size * (m_new[k] / (np.sqrt(v_new[k]) / bc2_sqrt + eps)) for k in p}


def _nudged(x, ulps):
    """x moved by ``ulps`` floating-point neighbours (per element)."""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(int(ulps))):
        x = np.nextafter(x, np.inf if ulps > 0 else -np.inf)
    return x


def adam_kernel(p, g, m, v, steps, hyper, dtype, target=None, active=None, pow_ulps=(0, 0)):
    """cobel_adam_step as k_adam (csrc/adam.hip) performs it: the kernel's operations in the
    kernel's order and dtype, one rounding each (the library builds with -ffp-contract=off), on
    arrays [n, per_instance] of ``dtype`` with ``steps`` [n] the counts INCLUDING this step.
    1 - beta1, beta2, eps, lr, weight_decay and tau are cast to ``dtype`` where the kernel casts
    them; the bias corrections 1 - beta1^t and sqrt(1 - beta2^t) are formed in Python float64 and
    cast (``pow_ulps``: beta1^t and beta2^t moved by that many float64 neighbours first — what
    another pow may return).  Rows of instances outside ``active`` come back as they are.
    Returns (param, exp_avg, exp_avg_sq, target or None)."""
    T = np.dtype(dtype).type
    for a in (p, g, m, v) + (() if target is None else (target,)):
        assert a.dtype == np.dtype(dtype) and a.ndim == 2
    lr, b1, b2, eps, wd, tau = (hyper[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay',
                                                   'tau'))
    x1 = _nudged([float(b1) ** float(t) for t in steps], pow_ulps[0])
    x2 = _nudged([float(b2) ** float(t) for t in steps], pow_ulps[1])
    with np.errstate(all='ignore'):
        bc1 = (1.0 - x1).astype(dtype)[:, None]
        bc2_sqrt = np.sqrt(1.0 - x2).astype(dtype)[:, None]
        step_size = T(lr) / bc1
        ge = g if wd == 0.0 else g + T(wd) * p
        mn = m + T(1.0 - b1) * (ge - m)
        vn = v * T(b2) + (T(1.0 - b2) * ge) * ge
        denom = np.sqrt(vn) / bc2_sqrt + T(eps)
        pn = p - step_size * (mn / denom)
        tn = None if target is None else target + T(tau) * (pn - target)
    for a in (mn, vn, pn) + (() if tn is None else (tn,)):
        assert a.dtype == np.dtype(dtype)
    if active is not None:
        on = (np.asarray(active) != 0)[:, None]
        pn, mn, vn = np.where(on, pn, p), np.where(on, mn, m), np.where(on, vn, v)
        tn = None if tn is None else np.where(on, tn, target)
    return pn, mn, vn, tn


def blend(t, p, tau):
    """The target network moved towards the online one: t + tau (p - t)."""
    return {k: t[k] + tau * (p[k] - t[k]) for k in t}


def fit_step(net, x, y, mask, train, hyper):
    """One cobel_mlp_fit step of ONE network held as ``net = {'p', 'm', 'v', 'steps'[, 't']}``:
    the optimiser step if ``train`` (also with nothing marked: a zero gradient), then the blend."""
    out = dict(net)
    if train:
        step = net['steps'] + 1.0
        g = grads(net['p'], x, y, mask)
        out['p'], out['m'], out['v'] = adam(net['p'], net['m'], net['v'], g, step, hyper['lr'],
                                            hyper['beta1'], hyper['beta2'], hyper['eps'],
                                            hyper['weight_decay'])
        out['steps'] = step
    if hyper['tau'] != 0.0 and net.get('t') is not None:
        out['t'] = blend(net['t'], out['p'], hyper['tau'])
    return out


# ---------------------------------------------------------------------------------------------
# the regression targets of DynaDSR.replay (include/cobel_hip.h, cobel_dsr_targets)
def first_maximum(value):
    """argmax over axis 1 of value [n, A, B], the FIRST maximum: a later action wins only if it
    is strictly greater."""
    best = np.zeros(value[:, 0].shape, dtype=np.int64)
    top = value[:, 0].copy()
    for a in range(1, value.shape[1]):
        better = value[:, a] > top
        top = np.where(better, value[:, a], top)
        best = np.where(better, a, best)
    return best


def dsr_targets(successor, value, table, state_index, next_index, actions, nonterminal, gamma,
                use_dr, follow_up, ignore_terminality, dtype=np.float64):
    """targets [n, B, O], took [n A, B], train [n A] from successor [n, A, B, O], value [n, A, B],
    the float64 observation table [rows, O], state / next rows [n, B], actions [n, B] and
    nonterminal [n, B] — every operation in ``dtype`` and in the order of the header's expressions
    (the use_dr mean adds the actions in ascending order and divides once)."""
    T = np.dtype(dtype).type
    fsr, val = np.asarray(successor, dtype=dtype), np.asarray(value, dtype=dtype)
    n, A, rows, O = fsr.shape
    nxt = np.asarray(table)[np.asarray(next_index)].astype(dtype)               # [n, B, O]
    base = nxt if follow_up else np.asarray(table)[np.asarray(state_index)].astype(dtype)
    nt = (np.asarray(nonterminal) != 0).astype(dtype)                            # [n, B]
    if use_dr:
        total = fsr[:, 0].copy()
        for a in range(1, A):
            total = total + fsr[:, a]
        boot_sr = total / T(A)
    else:
        best = first_maximum(val)                                                # [n, B]
        boot_sr = np.take_along_axis(fsr, best[:, None, :, None], axis=1)[:, 0]
    follow, ignore = T(1.0 if follow_up else 0.0), T(1.0 if ignore_terminality else 0.0)
    c1 = T((1.0 - float(follow)) * (1.0 - float(ignore)))
    boot = (nxt * c1) * (T(1.0) - nt)[..., None]
    boot = boot + boot_sr * np.minimum(nt + ignore, T(1.0))[..., None]
    targets = base + T(gamma) * boot
    assert targets.dtype == np.dtype(dtype)
    took = np.asarray(actions)[:, None, :] == np.arange(A)[None, :, None]        # [n, A, B]
    took = took.reshape(n * A, rows)
    return targets, took.astype(np.uint8), took.any(axis=1).astype(np.uint8)


def dsr_magnitude(successor, value, table, state_index, next_index, gamma, follow_up):
    """|base| + |gamma| (|next| + sum_a |successor[a]|): every partial result of a target is at most
    this large, so (A + 4) roundings of it bound the distance between two evaluation orders."""
    fsr = np.abs(np.asarray(successor, dtype=np.float64))
    nxt = np.abs(np.asarray(table)[np.asarray(next_index)])
    base = nxt if follow_up else np.abs(np.asarray(table)[np.asarray(state_index)])
    return base + abs(gamma) * (nxt + fsr.sum(axis=1))


def dsr_case(seed, n, A, O, dtype, rows=11):
    """Inputs of cobel_dsr_targets (arrays by the struct's field names, successor [n, A, B, O] and
    value [n, A, B] in ``dtype``) with the cases an argmax and a ballot go wrong on planted:
    values from a handful of numbers (ties everywhere), and in every agent sample 0 all actions
    equal, 1 the strict maximum at the first action, 2 at the last, 3 the maximum twice (actions 1
    and 3, as far as they exist); nonterminal 0 / 1 / 0.5; agent 1 one sample with an action nobody
    else took, agent 2 all 32 samples on one action."""
    assert n >= 3
    rng = np.random.default_rng(seed)
    value = rng.integers(-2, 3, size=(n, A, B)).astype(dtype) * np.dtype(dtype).type(0.25)
    value[:, :, 0] = 0.75
    value[:, :, 1], value[:, 0, 1] = -1.0, 1.5
    value[:, :, 2], value[:, A - 1, 2] = -1.0, 1.5
    value[:, :, 3] = -1.0
    value[:, min(1, A - 1), 3] = value[:, min(3, A - 1), 3] = 2.0
    actions = rng.integers(0, A, size=(n, B)).astype(np.int64)
    actions[1], actions[1, 17] = 0, A - 1
    actions[2] = A - 1
    nonterminal = np.resize(np.array([0.0, 1.0, 0.5]), n * B).reshape(n, B).astype(dtype)
    return {
        'successor': rng.standard_normal((n, A, B, O)).astype(dtype),
        'value': value,
        'table': rng.standard_normal((rows, O)),
        'state_index': rng.integers(0, rows, size=(n, B)).astype(np.int32),
        'next_index': rng.integers(0, rows, size=(n, B)).astype(np.int32),
        'actions': actions,
        'nonterminal': nonterminal,
    }


# ---------------------------------------------------------------------------------------------
# the DQN replay step (include/cobel_hip.h, cobel_dqn_replay)
GAP = 1e-3                           # least top-two gap of a drawn sample's Q row, relative to max |Q|
TABLE_ROWS = 13                      # rows of a dqn_case's observation table


def dqn_targets(p_online, p_target, x_next, rewards, nonterminal, gamma, ddqn):
    """new [rows] = r + (boot * nt) * gamma in the header's operation order: boot the maximum of
    Q_target(s'), with ``ddqn`` Q_target(s') at the FIRST maximum of Q_online(s').  A sample with
    nt == 0 does not look at the target network (boot counts as 0 there, whatever it holds)."""
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
    """One cobel_dqn_replay step of ONE instance held as ``net = {'p', 'm', 'v', 'steps', 't'}``,
    ``steps`` the count INCLUDING this step (it stays as it is), on ``batch = {'states' [32, D],
    'next_states', 'actions' [32], 'rewards', 'nonterminal'}``: the regression target is Q_online(s)
    with entry actions[s] replaced by new[s], the loss the mean over the 32 x A outputs.  Returns
    the new state, the gradient, and q_out = forward(new p, obs) for an observation row (or None)."""
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


def top_two_gap(q):
    """The least distance between the largest and the second largest entry of a row of q [rows, A],
    relative to max |q| (infinite with one action: nothing to confuse)."""
    q = np.asarray(q, dtype=np.float64)
    if q.shape[1] < 2:
        return np.inf
    top = np.sort(q, axis=1)
    return float((top[:, -1] - top[:, -2]).min()) / max(float(np.abs(q).max()), np.finfo(np.float64).tiny)


def dqn_gap(p_online, p_target, x_next, ddqn):
    """The top-two gap a float32 kernel has to resolve on these next states: of Q_target(s') and,
    with ``ddqn``, of Q_online(s')."""
    gap = top_two_gap(forward(p_target, x_next)[2])
    return min(gap, top_two_gap(forward(p_online, x_next)[2])) if ddqn else gap


def dqn_rows(case, j, dtype=np.float64):
    """The batch of instance j of a dqn_case as dqn_step takes it: the table rows in the case's
    dtype (what every input mode hands the kernel), converted to ``dtype``."""
    table = case['table'].astype(case['dtype'])
    return {'states': table[case['state_index'][j]].astype(dtype),
            'next_states': table[case['next_index'][j]].astype(dtype),
            'actions': case['actions'][j], 'rewards': case['rewards'][j].astype(dtype),
            'nonterminal': case['nonterminal'][j].astype(dtype)}


def _dqn_draw(case, s, ddqn, online, target, plant):
    """One try of dqn_draw_batch: the table and the batch of seed s; False if a gap is too small."""
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
    """A new observation table (float64, 13 rows) and batch for a dqn_case whose networks have
    moved on — state / next rows of the table, actions, rewards and non-terminal flags (0 / 1, a
    fifth terminal) [n, 32] — from the first of seed, seed + 1, ... for which every sample of every
    instance keeps the gap GAP (dqn_gap) under the networks ``online`` / ``target`` (lists of
    float64 parameter dicts).  Returns the seed; raises if none of ``tries`` seeds will do."""
    for s in range(seed, seed + tries):
        if _dqn_draw(case, s, ddqn, online, target, None):
            return s
    raise AssertionError('no seed in %d .. %d keeps the top-two gap' % (seed, seed + tries - 1))


def dqn_case(seed, n, D, A, dtype, ddqn=True, zero_moments=False, steps=None, plant=None, tries=64):
    """n instances of cobel_dqn_replay: online networks 'P' and target networks 'T' (different),
    moments 'M' / 'V' of the size they have in the middle of a run (zero_moments: none), step counts
    'steps' (INCLUDING the step to come, one per instance and all different unless given), and a
    batch drawn from a float64 observation table of 13 rows — so the same case can be given
    gathered, through rings, and as table rows.  Stacked arrays in ``dtype``.
    Everything is drawn from the first of seed, seed + 1, ... ('seed' of the result) for which
    every sample of every instance keeps the gap GAP (dqn_gap: of Q_target(s') and, with ``ddqn``,
    of Q_online(s')).  ``plant(case)`` edits the drawn case in place before the condition is looked
    at and returns the instances it exempts (planted ties: exact in any summation order).  Raises
    if none of ``tries`` seeds will do."""
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
        if _dqn_draw(case, s, ddqn, None, None, plant):
            return case
    raise AssertionError('no seed in %d .. %d keeps the top-two gap' % (seed, seed + tries - 1))


def plant_tie(stack, j, actions, value):
    """Network j of ``stack`` rates ``actions`` at exactly ``value`` on every input, in any
    summation order: their rows of w3 are zero and their b3 equal."""
    for a in actions:
        stack['w3'][j, a] = 0.0
        stack['b3'][j, a] = value


BATCH_KEYS = ('state_index', 'next_index', 'actions', 'rewards', 'nonterminal')


def plant_ddqn(case):
    """Instances 0 .. 3: Q_online(s') all equal; a strict maximum at the first action; at the last;
    the maximum twice (actions 1 and 3, as far as they exist) — exact in any summation order, and
    the target networks rate the tied actions differently.  4: every sample terminal.  5: two
    samples with the same row.  6: all 32 samples with the same row."""
    A = case['A']
    plant_tie(case['P'], 0, range(A), 0.3)
    plant_tie(case['P'], 1, [0], 10.0)
    plant_tie(case['P'], 2, [A - 1], 10.0)
    plant_tie(case['P'], 3, sorted({min(1, A - 1), min(3, A - 1)}), 10.0)
    case['nonterminal'][4] = 0.0
    for key in BATCH_KEYS:
        case[key][5, 5] = case[key][5, 4]
        case[key][6, :] = case[key][6, 0]
    return {0, 1, 2, 3}


def plant_plain(case):
    """Instance 0: all 32 samples with one action, from zero moments (rewards 2 .. 3, above every
    Q-value: the 32 loss gradients of that action then have one sign, and their sum — the only
    entry of db3 that is not zero, so the one its max-norm is taken over — does not cancel).
    1: actions 0 and A - 1 both present.  2: every sample terminal and the target network NaN."""
    A = case['A']
    case['actions'][0] = min(2, A - 1)
    case['rewards'][0] = 2.0 + np.arange(B) / B
    for k in KEYS:
        case['M'][k][0], case['V'][k][0] = 0.0, 0.0
        case['T'][k][2] = np.nan
    case['actions'][1, 0], case['actions'][1, 1] = 0, A - 1
    case['nonterminal'][2] = 0.0
    return {2}


def plant_one_row(case):
    """Every instance: all 32 samples the same row (what a ring of one row holds)."""
    for key in BATCH_KEYS:
        case[key][:, :] = case[key][:, :1]
    return ()


DQN_OPTIONS = ['weight_decay', 'tau0', 'tau1', 'steps', 'gamma0', 'ddqn']


def dqn_gpu_cases(D, A):
    """Every case tests/test_gpu_dqn_replay_edges.py draws at one shape, by key: the arguments of
    dqn_case (seed base, instances, plants).  tests/test_host_mlp_reference.py draws each of them
    in both dtypes, so that a search that fails is found without a GPU."""
    cases = {}
    for ddqn in (False, True):
        cases['backward', ddqn] = dict(seed=100 * D + 10 * A + ddqn, n=5, ddqn=ddqn,
                                       zero_moments=True, steps=1.0)
        cases['plain', ddqn] = dict(seed=300 * D + 10 * A + ddqn, n=3, ddqn=ddqn, plant=plant_plain)
    cases['ties'] = dict(seed=200 * D + 10 * A, n=7, ddqn=True, plant=plant_ddqn)
    for ring_slots in (1, 32, 33, 40):
        cases['modes', ring_slots] = dict(seed=400 * D + 10 * A + ring_slots, n=5,
                                          ddqn=ring_slots in (1, 33),
                                          plant=plant_one_row if ring_slots == 1 else None)
    cases['sit_out'] = dict(seed=500 * D + 10 * A, n=7, ddqn=False)
    for k, option in enumerate(DQN_OPTIONS):
        cases['options', option] = dict(seed=1000 * (1 + k) + 20 * D + A, n=5, ddqn=option == 'ddqn',
                                        steps=[1.0, 1e6, 1.0, 1e6, 2.0] if option == 'steps' else None)
    cases['q_out'] = dict(seed=600 * D + 10 * A, n=5, ddqn=False)
    if A == 4:
        cases['two_forms'] = dict(seed=700 * D, n=5, ddqn=True)
    return cases


def dqn_gpu_case(key, D, A, dtype):
    return dqn_case(D=D, A=A, dtype=dtype, **dqn_gpu_cases(D, A)[key])


# ---------------------------------------------------------------------------------------------
# error measures
def rel_err(got, ref):
    """max |got - ref| / max |ref| (max-norm relative, per tensor); 0 only if they are equal."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    diff = float(np.abs(got - ref).max()) if ref.size else 0.0
    if diff == 0.0:
        return 0.0
    return diff / max(float(np.abs(ref).max()), np.finfo(np.float64).tiny)


def f32_bound(torch_err):
    """What a float32 kernel may differ from the float64 reference by, given what torch's float32
    on the CPU differs by on the same inputs."""
    return max(F32_FACTOR * torch_err, F32_FLOOR)


# ---------------------------------------------------------------------------------------------
# launch structs from dicts of (stacked, contiguous) torch tensors; ``lib`` is cobel_amd._lib
def _three(lib, dst, tensors, names):
    for k, name in enumerate(names):
        dst[k] = lib.ptr(tensors[name]) if tensors is not None else None


def fill_forward(lib, params, out, n, D, O, net_div=1, act_div=1, active=None, in_table=None,
                 in_index=None, in_div=1, in_dense=None):
    run = lib.MLPForward()
    _three(lib, run.w, params, ('w1', 'w2', 'w3'))
    _three(lib, run.b, params, ('b1', 'b2', 'b3'))
    run.active, run.act_div, run.net_div = lib.ptr(active), act_div, net_div
    run.in_table, run.in_index, run.in_div = lib.ptr(in_table), lib.ptr(in_index), in_div
    run.in_dense, run.out = lib.ptr(in_dense), lib.ptr(out)
    run.n, run.n_inputs, run.n_outputs = n, D, O
    run.is_float64 = int(params['w1'].element_size() == 8)
    return run


def fill_fit(lib, params, m, v, steps, targets, n, D, O, hyper, target_params=None, train=None,
             active=None, act_div=1, in_table=None, in_index=None, in_div=1, in_dense=None,
             tgt_div=1, sample_mask=None, ep_table=None, ep_index=None, ep_dense=None, ep_div=1,
             ep_rows=0, ep_out=None):
    run = lib.MLPFit()
    for w, b, src in ((run.w, run.b, params), (run.m_w, run.m_b, m), (run.v_w, run.v_b, v),
                      (run.w_target, run.b_target, target_params)):
        _three(lib, w, src, ('w1', 'w2', 'w3'))
        _three(lib, b, src, ('b1', 'b2', 'b3'))
    run.steps, run.train, run.active = lib.ptr(steps), lib.ptr(train), lib.ptr(active)
    run.in_table, run.in_index = lib.ptr(in_table), lib.ptr(in_index)
    run.in_dense = lib.ptr(in_dense)
    run.targets, run.sample_mask = lib.ptr(targets), lib.ptr(sample_mask)
    run.ep_table, run.ep_index = lib.ptr(ep_table), lib.ptr(ep_index)
    run.ep_dense, run.ep_out = lib.ptr(ep_dense), lib.ptr(ep_out)
    run.n, run.n_inputs, run.n_outputs = n, D, O
    run.is_float64 = int(params['w1'].element_size() == 8)
    run.in_div, run.tgt_div, run.act_div = in_div, tgt_div, act_div
    run.ep_div, run.ep_rows = ep_div, ep_rows
    run.lr, run.beta1, run.beta2 = hyper['lr'], hyper['beta1'], hyper['beta2']
    run.eps, run.weight_decay, run.tau = hyper['eps'], hyper['weight_decay'], hyper['tau']
    return run


def fill_dsr(lib, t, n, A, O, is_float64, gamma, use_dr, follow_up, ignore_terminality):
    """``t``: tensors by the struct's field names."""
    run = lib.DSRTargets()
    for name in ('successor', 'value', 'table', 'state_index', 'next_index', 'actions',
                 'nonterminal', 'targets', 'took', 'train'):
        setattr(run, name, lib.ptr(t.get(name)))
    run.n, run.n_actions, run.n_outputs, run.is_float64 = n, A, O, int(is_float64)
    run.use_dr, run.follow_up = int(bool(use_dr)), int(bool(follow_up))
    run.ignore_terminality, run.gamma = int(bool(ignore_terminality)), float(gamma)
    return run


def fill_dqn_replay(lib, params, target_params, m, v, steps, batch, n, D, A, hyper, gamma, ddqn,
                    active=None, obs_index=None, obs_table=None, q_out=None):
    """``batch``: tensors by the struct's field names — gathered 'states' / 'next_states' [n, 32, D],
    'actions', 'rewards', 'nonterminal' [n, 32]; the same five as rings [n, ring_slots, ..] with
    'batch_slots' [n, 32] and 'ring_slots'; or 'state_index' / 'next_index' [n, 32] with the
    [n, 32] 'actions', 'rewards', 'nonterminal' (``obs_table`` holds the rows)."""
    run = lib.DQNReplay()
    for w, b, src in ((run.w, run.b, params), (run.w_target, run.b_target, target_params),
                      (run.m_w, run.m_b, m), (run.v_w, run.v_b, v)):
        _three(lib, w, src, ('w1', 'w2', 'w3'))
        _three(lib, b, src, ('b1', 'b2', 'b3'))
    run.steps, run.active = lib.ptr(steps), lib.ptr(active)
    for name in ('states', 'next_states', 'actions', 'rewards', 'nonterminal', 'batch_slots',
                 'state_index', 'next_index'):
        setattr(run, name, lib.ptr(batch.get(name)))
    run.ring_slots = int(batch.get('ring_slots', 0))
    run.obs_index, run.obs_table, run.q_out = lib.ptr(obs_index), lib.ptr(obs_table), lib.ptr(q_out)
    run.n, run.n_inputs, run.n_hidden1, run.n_hidden2, run.n_actions, run.batch = n, D, H, H, A, B
    run.is_float64, run.ddqn = int(params['w1'].element_size() == 8), int(bool(ddqn))
    run.gamma, run.lr, run.beta1, run.beta2 = gamma, hyper['lr'], hyper['beta1'], hyper['beta2']
    run.eps, run.weight_decay, run.tau = hyper['eps'], hyper['weight_decay'], hyper['tau']
    return run
