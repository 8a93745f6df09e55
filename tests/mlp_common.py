"""A plain float64 restatement of what csrc/mlp_fit.hip and csrc/dsr_targets.hip compute, in NumPy
only (no torch, no project code), and the helpers that fill the launch structs of
cobel_mlp_forward / cobel_mlp_fit / cobel_dsr_targets from dicts of tensors.

A network is a dict ``{'w1': [64, D], 'b1': [64], 'w2': [64, 64], 'b2': [64], 'w3': [O, 64],
'b3': [O]}`` — Linear(D, 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, O), weights as torch.nn.Linear
keeps them ([out][in]).  Moments and gradients are dicts of the same shape.  Every function returns
new arrays and leaves its arguments alone.

tests/test_host_mlp_reference.py checks this file against torch autograd + torch.optim.Adam in
float64 on the CPU; tests/test_gpu_mlp_edges.py checks the kernels against this file."""
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
