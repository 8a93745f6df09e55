"""The float64 reference of the stacked-network kernels (tests/mlp_common.py) against torch on
the CPU — autograd, torch.optim.Adam, lerp, and the torch expressions of DynaDSR.replay's PyTorch
path and of the DQN replay step's — and the argument checks of cobel_mlp_query / cobel_mlp_forward /
cobel_mlp_fit / cobel_dsr_targets / cobel_dqn_replay, which return before any launch.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402

HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3, tau=0.07)


def torch_forward(torch, tp, x):
    h = torch.relu(x @ tp['w1'].T + tp['b1'])
    h = torch.relu(h @ tp['w2'].T + tp['b2'])
    return h @ tp['w3'].T + tp['b3']


def torch_loss(torch, tp, x, y, mask):
    q = torch_forward(torch, tp, x)
    on = torch.ones(x.shape[0], dtype=x.dtype) if mask is None else \
        torch.as_tensor(np.asarray(mask) != 0).to(x.dtype)
    return (((q - y) ** 2) * on[:, None]).sum() / (max(float(on.sum()), 1.0) * q.shape[1])


@pytest.mark.parametrize('D,O', [(1, 1), (7, 17), (32, 32)])
def test_reference_matches_torch_autograd_and_adam(D, O):
    """Three masked steps from a pre-seeded optimizer state (step count 5, non-zero moments) with
    weight decay: gradients to 1e-12 (max-norm relative per tensor; NumPy and torch differ by
    1.1e-14 here), parameters, moments and the blended target to rtol 1e-9 / atol 1e-12."""
    import torch
    rng = np.random.default_rng(100 * D + O)
    p = mc.one(mc.draw_networks(rng, 1, D, O, np.float64), 0)
    t = mc.one(mc.draw_networks(rng, 1, D, O, np.float64), 0)
    m = {k: 0.01 * rng.standard_normal(a.shape) for k, a in p.items()}
    v = {k: 1e-4 * rng.random(a.shape) for k, a in p.items()}
    net = {'p': p, 'm': m, 'v': v, 't': t, 'steps': 5.0}
    x, y = rng.standard_normal((mc.B, D)), rng.standard_normal((mc.B, O))
    single = np.zeros(mc.B, dtype=np.uint8)
    single[16] = 1
    masks = [(rng.random(mc.B) < 0.4).astype(np.uint8), single, None]

    tp = {k: torch.tensor(a, requires_grad=True) for k, a in p.items()}
    tt = {k: torch.tensor(a) for k, a in t.items()}
    opt = torch.optim.Adam([tp[k] for k in mc.KEYS], lr=HYPER['lr'], eps=HYPER['eps'],
                           betas=(HYPER['beta1'], HYPER['beta2']),
                           weight_decay=HYPER['weight_decay'])
    for k in mc.KEYS:
        opt.state[tp[k]] = {'step': torch.tensor(5.0), 'exp_avg': torch.tensor(m[k]),
                            'exp_avg_sq': torch.tensor(v[k])}
    tx, ty = torch.tensor(x), torch.tensor(y)
    for it, mask in enumerate(masks):
        h1, h2, q = mc.forward(net['p'], x)
        with torch.no_grad():
            assert mc.rel_err(torch_forward(torch, tp, tx).numpy(), q) <= 1e-12
        opt.zero_grad()
        torch_loss(torch, tp, tx, ty, mask).backward()
        g = mc.grads(net['p'], x, y, mask)
        for k in mc.KEYS:
            assert mc.rel_err(g[k], tp[k].grad.numpy()) <= 1e-12, (it, k)
        opt.step()
        net = mc.fit_step(net, x, y, mask, True, HYPER)
        with torch.no_grad():
            for k in mc.KEYS:
                tt[k] = torch.lerp(tt[k], tp[k], HYPER['tau'])
        for k in mc.KEYS:
            st = opt.state[tp[k]]
            for name, got, want in (('p', net['p'][k], tp[k].detach()), ('m', net['m'][k], st['exp_avg']),
                                    ('v', net['v'][k], st['exp_avg_sq']), ('t', net['t'][k], tt[k])):
                assert np.allclose(got, want.numpy(), rtol=1e-9, atol=1e-12), (it, k, name)
            assert float(st['step']) == net['steps'] == 6.0 + it


def test_adam_in_kernel_order_matches_torch_adam():
    """mlp_common.adam_kernel (k_adam's operations in k_adam's order) in float64 against
    torch.optim.Adam on the CPU: 5 steps with weight decay from non-zero moments and step counts
    0 and 7, three instances with one sitting out — parameters and both moments to rtol 1e-12,
    the blended target against torch.lerp; in float32 the same function stays in float32."""
    import torch
    rng = np.random.default_rng(17)
    n, per = 3, 41
    hyper = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3, tau=0.05)
    p = rng.standard_normal((n, per))
    m, v = 0.01 * rng.standard_normal((n, per)), 1e-4 * rng.random((n, per))
    m[0], v[0] = 0.0, 0.0
    t = rng.standard_normal((n, per))
    steps = np.array([0.0, 7.0, 3.0])
    active = np.array([1, 1, 0], dtype=np.uint8)
    tp = [torch.tensor(p[j], requires_grad=True) for j in range(n)]
    tt = [torch.tensor(t[j]) for j in range(n)]
    opts = []
    for j in range(n):
        opt = torch.optim.Adam([tp[j]], lr=hyper['lr'], eps=hyper['eps'],
                               betas=(hyper['beta1'], hyper['beta2']),
                               weight_decay=hyper['weight_decay'])
        opt.state[tp[j]] = {'step': torch.tensor(steps[j]), 'exp_avg': torch.tensor(m[j]),
                            'exp_avg_sq': torch.tensor(v[j])}
        opts.append(opt)
    for it in range(5):
        g = rng.standard_normal((n, per)) * 10.0 ** rng.integers(-6, 1, size=(n, per))
        steps = steps + active
        p, m, v, t = mc.adam_kernel(p, g, m, v, steps, hyper, np.float64, target=t, active=active)
        for j in range(n):
            if not active[j]:
                continue
            tp[j].grad = torch.tensor(g[j])
            opts[j].step()
            with torch.no_grad():
                tt[j] = torch.lerp(tt[j], tp[j], hyper['tau'])
        for j in range(n):
            st = opts[j].state[tp[j]]
            for name, got, want in (('p', p[j], tp[j].detach()), ('m', m[j], st['exp_avg']),
                                    ('v', v[j], st['exp_avg_sq']), ('t', t[j], tt[j])):
                assert np.allclose(got, want.numpy(), rtol=1e-12, atol=0.0), (it, j, name)
            assert float(st['step']) == steps[j]
    f32 = [a.astype(np.float32) for a in (p, g, m, v, t)]
    out = mc.adam_kernel(f32[0], f32[1], f32[2], f32[3], steps, hyper, np.float32, target=f32[4])
    assert all(a.dtype == np.float32 for a in out)


def test_reference_empty_mask_and_no_training():
    """Nothing marked: the count clamps to 1 and the gradient is exactly zero, as torch's; a
    network that does not train keeps everything but its blended target."""
    import torch
    rng = np.random.default_rng(3)
    D, O = 9, 15
    p = mc.one(mc.draw_networks(rng, 1, D, O, np.float64), 0)
    x, y = rng.standard_normal((mc.B, D)), rng.standard_normal((mc.B, O))
    none = np.zeros(mc.B, dtype=np.uint8)
    g = mc.grads(p, x, y, none)
    tp = {k: torch.tensor(a, requires_grad=True) for k, a in p.items()}
    torch_loss(torch, tp, torch.tensor(x), torch.tensor(y), none).backward()
    for k in mc.KEYS:
        assert not g[k].any() and not tp[k].grad.numpy().any()
    net = {'p': p, 'm': p, 'v': p, 't': g, 'steps': 2.0}
    out = mc.fit_step(net, x, y, None, False, HYPER)
    assert out['steps'] == 2.0 and out['p'] is p and out['m'] is p and out['v'] is p
    for k in mc.KEYS:
        assert np.array_equal(out['t'][k], HYPER['tau'] * p[k])


@pytest.mark.parametrize('A', [1, 3, 4, 8])
@pytest.mark.parametrize('switches', [False, True])
def test_reference_dsr_targets_match_torch_expressions(A, switches):
    """dsr_targets against the torch expressions of DynaDSR.replay's PyTorch path in float64:
    bit for bit with use_DR off; with it on torch's mean may add the actions in another order, so
    within (A + 4) roundings of the largest partial result."""
    import torch
    n, O, gamma = 5, 7, 0.9
    c = mc.dsr_case(40 + A, n, A, O, np.float64)
    use_dr = follow_up = switches
    ignore_terminality = switches
    targets, took, train = mc.dsr_targets(gamma=gamma, use_dr=use_dr, follow_up=follow_up,
                                          ignore_terminality=ignore_terminality, **c)
    future, val = torch.tensor(c['successor']), torch.tensor(c['value'])
    tab, ni, si = torch.tensor(c['table']), torch.tensor(c['next_index']), torch.tensor(c['state_index'])
    bt, ba = torch.tensor(c['nonterminal']), torch.tensor(c['actions'])
    follow, ignore = float(follow_up), float(ignore_terminality)
    if use_dr:
        boot_sr = future.mean(dim=1)
    else:
        best = val.argmax(dim=1)
        assert np.array_equal(best.numpy(), mc.first_maximum(c['value']))
        boot_sr = torch.gather(future, 1, best[:, None, :, None].expand(n, 1, 32, O))[:, 0]
    nxt, nonterminal = tab[ni.to(torch.int64)], (bt != 0).to(torch.float64)
    boot = nxt * ((1.0 - follow) * (1.0 - ignore)) * (1.0 - nonterminal)[..., None]
    boot = boot + boot_sr * torch.clamp(nonterminal + ignore, max=1.0)[..., None]
    want = (nxt if follow_up else tab[si.to(torch.int64)]) + gamma * boot
    mine = (ba[:, None, :] == torch.arange(A)[None, :, None]).reshape(n * A, 32)
    assert np.array_equal(took, mine.numpy().astype(np.uint8))
    assert np.array_equal(train, mine.any(dim=1).numpy().astype(np.uint8))
    if use_dr:
        bound = (A + 4) * 2.0 ** -53 * mc.dsr_magnitude(
            c['successor'], c['value'], c['table'], c['state_index'], c['next_index'], gamma, follow_up)
        assert (np.abs(targets - want.numpy()) <= bound).all()
    else:
        assert np.array_equal(targets, want.numpy())
    # the planted cases are what they claim to be
    best = mc.first_maximum(c['value'])
    assert (best[:, 0] == 0).all() and (best[:, 1] == 0).all() and (best[:, 2] == A - 1).all()
    assert (best[:, 3] == min(1, A - 1)).all()
    assert train.reshape(n, A)[2].tolist() == [0] * (A - 1) + [1]
    assert took.reshape(n, A, 32)[1, A - 1].sum() == (1 if A > 1 else 32)


# ---------------------------------------------------------------------------------------------
# the DQN replay step
@pytest.mark.parametrize('ddqn', [False, True])
@pytest.mark.parametrize('D,A', [(6, 4), (25, 4), (31, 6), (1, 1)])
def test_reference_dqn_step_matches_torch_replay_path(D, A, ddqn):
    """dqn_step against this package's PyTorch replay path restated in float64 on the CPU
    (targets = forward(s).clone(), scatter_ of r + boot * nt * gamma, MSE, autograd,
    torch.optim.Adam, lerp), from a pre-seeded optimizer state with weight decay: gradients to
    1e-12, parameters, moments, the blended target and q_out to rtol 1e-9 / atol 1e-12."""
    import torch
    gamma = 0.8
    c = mc.dqn_case(10 * D + A, 3, D, A, np.float64, ddqn=ddqn)
    for j in range(3):
        net = {'p': mc.one(c['P'], j), 't': mc.one(c['T'], j), 'm': mc.one(c['M'], j),
               'v': mc.one(c['V'], j), 'steps': float(c['steps'][j])}
        b = mc.dqn_rows(c, j)
        obs = c['table'][j]
        out, g, q_out = mc.dqn_step(net, b, HYPER, gamma, ddqn, obs)
        assert out['steps'] == net['steps']

        tp = {k: torch.tensor(a, requires_grad=True) for k, a in net['p'].items()}
        tt = {k: torch.tensor(a) for k, a in net['t'].items()}
        opt = torch.optim.Adam([tp[k] for k in mc.KEYS], lr=HYPER['lr'], eps=HYPER['eps'],
                               betas=(HYPER['beta1'], HYPER['beta2']),
                               weight_decay=HYPER['weight_decay'])
        for k in mc.KEYS:     # (the optimizer counts the steps before this one)
            opt.state[tp[k]] = {'step': torch.tensor(net['steps'] - 1.0),
                                'exp_avg': torch.tensor(net['m'][k]),
                                'exp_avg_sq': torch.tensor(net['v'][k])}
        s, ns = torch.tensor(b['states']), torch.tensor(b['next_states'])
        a, r, nt = torch.tensor(b['actions']), torch.tensor(b['rewards']), torch.tensor(b['nonterminal'])
        with torch.no_grad():
            targets = torch_forward(torch, tp, s).clone()
            boot = torch_forward(torch, tt, ns)
            pick = (torch_forward(torch, tp, ns) if ddqn else boot).argmax(dim=1)
            boot = torch.gather(boot, 1, pick[:, None])[:, 0]
            new = r + boot * nt * gamma
            targets.scatter_(1, a[:, None], new[:, None])
        assert np.allclose(mc.dqn_targets(net['p'], net['t'], b['next_states'], b['rewards'],
                                          b['nonterminal'], gamma, ddqn), new.numpy(),
                           rtol=1e-9, atol=1e-12)
        ((torch_forward(torch, tp, s) - targets) ** 2).mean().backward()
        for k in mc.KEYS:
            assert mc.rel_err(g[k], tp[k].grad.numpy()) <= 1e-12, (j, k)
        opt.step()
        with torch.no_grad():
            for k in mc.KEYS:
                tt[k] = torch.lerp(tt[k], tp[k], HYPER['tau'])
            want_q = torch_forward(torch, tp, torch.tensor(obs)[None])[0]
        for k in mc.KEYS:
            st = opt.state[tp[k]]
            for name, got, want in (('p', out['p'][k], tp[k].detach()), ('m', out['m'][k], st['exp_avg']),
                                    ('v', out['v'][k], st['exp_avg_sq']), ('t', out['t'][k], tt[k])):
                assert np.allclose(got, want.numpy(), rtol=1e-9, atol=1e-12), (j, k, name)
            assert float(st['step']) == net['steps']
        assert np.allclose(q_out, want_q.numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('A', [1, 2, 3, 4, 8])
def test_reference_dqn_targets_on_planted_ties(A):
    """Tied actions planted so that they are exact in any summation order (zero rows of w3, equal
    b3): the first tied action is taken, and the target network's value at it is the bootstrap."""
    rng = np.random.default_rng(A)
    D, gamma = 5, 0.9
    x = rng.standard_normal((mc.B, D))
    r, nt = rng.standard_normal(mc.B), np.ones(mc.B)
    t = mc.one(mc.draw_networks(rng, 1, D, A, np.float64), 0)
    qt = mc.forward(t, x)[2]
    plans = [(list(range(A)), 0.3), ([0], 10.0), ([A - 1], 10.0),
             (sorted({min(1, A - 1), min(3, A - 1)}), 10.0)]
    for tied, value in plans:
        stack = mc.draw_networks(rng, 1, D, A, np.float32)
        mc.plant_tie(stack, 0, tied, value)
        p = mc.one(stack, 0)
        q = mc.forward(p, x)[2]
        assert (q[:, tied] == np.float64(np.float32(value))).all()        # exact, every sample
        assert (mc.first_maximum(q.T[None])[0] == tied[0]).all()
        new = mc.dqn_targets(p, t, x, r, nt, gamma, True)
        assert np.array_equal(new, r + (qt[:, tied[0]] * nt) * gamma)
        if len(tied) > 1:        # ... which is not what a later tied action would have given
            assert (qt[:, tied[0]] != qt[:, tied[-1]]).all()
    # a terminal sample does not look at the target network
    nan = {k: np.full_like(a, np.nan) for k, a in t.items()}
    assert np.array_equal(mc.dqn_targets(p, nan, x, r, np.zeros(mc.B), gamma, False), r)
    assert np.array_equal(mc.dqn_targets(p, nan, x, r, np.zeros(mc.B), gamma, True), r)


def _gpu_test_shapes():
    lds = [(D, 4) for D in (1, 8, 9, 16, 17, 32)]
    return lds + [(1, 1), (7, 8), (8, 4), (9, 3), (17, 5), (24, 2), (31, 6), (32, 4)]


@pytest.mark.parametrize('D,A', sorted(set(_gpu_test_shapes())))
def test_dqn_case_seed_search_succeeds_for_every_gpu_case(D, A):
    """Every case the GPU tests draw (mlp_common.dqn_gpu_cases: their seed bases, instance counts
    and plants), at every shape they use and in both dtypes: dqn_case finds a seed within its 64
    tries, the gap condition holds at that seed for every instance the plant does not exempt, and
    the search is deterministic."""
    for key, kw in mc.dqn_gpu_cases(D, A).items():
        for dt in (np.float64, np.float32):
            c = mc.dqn_gpu_case(key, D, A, dt)
            n, ddqn = kw['n'], kw['ddqn']
            assert kw['seed'] <= c['seed'] < kw['seed'] + 64 and c['n'] == n, key
            assert bool(c['exempt']) == (key == 'ties' or key[0] == 'plain'), key
            for j in set(range(n)) - c['exempt']:
                p, t, b = mc.one(c['P'], j), mc.one(c['T'], j), mc.dqn_rows(c, j)
                assert mc.top_two_gap(mc.forward(t, b['next_states'])[2]) >= mc.GAP, (key, j)
                if ddqn:
                    assert mc.top_two_gap(mc.forward(p, b['next_states'])[2]) >= mc.GAP, (key, j)
                assert not np.array_equal(c['P']['w2'][j], c['T']['w2'][j])
            assert c['P']['w1'].dtype == dt and c['rewards'].dtype == dt
            if kw.get('steps') is None:
                assert len(set(c['steps'].tolist())) == n
            zero = not any(c['V'][k].any() for k in mc.KEYS)
            assert zero == bool(kw.get('zero_moments')), key
        again = mc.dqn_gpu_case(key, D, A, np.float32)
        assert again['seed'] == c['seed']
        assert all(np.array_equal(again[k], c[k]) for k in ('table', 'next_index', 'actions'))
        assert np.array_equal(again['P']['w3'], c['P']['w3'])
    q = np.array([[0.0, 1.0, 1.0 - 0.5e-3], [2.0, -1.0, 0.0]])
    assert abs(mc.top_two_gap(q) - 0.25e-3) < 1e-12 and mc.top_two_gap(q[:, :1]) == np.inf


# ---------------------------------------------------------------------------------------------
# argument checks through the C ABI: every call below returns before it would launch anything
FAKE = 0x10000           # a 16-byte aligned address nobody dereferences


def _forward_run(_lib):
    run = _lib.MLPForward()
    for k in range(3):
        run.w[k] = run.b[k] = FAKE
    run.in_dense = run.out = FAKE
    run.n, run.n_inputs, run.n_outputs, run.is_float64 = 0, 9, 15, 1
    run.net_div = run.in_div = run.act_div = 1
    return run


def _fit_run(_lib):
    run = _lib.MLPFit()
    for field in (run.w, run.b, run.m_w, run.m_b, run.v_w, run.v_b, run.w_target, run.b_target):
        for k in range(3):
            field[k] = FAKE
    run.steps = run.targets = run.in_dense = FAKE
    run.n, run.n_inputs, run.n_outputs, run.is_float64 = 0, 9, 15, 1
    run.in_div = run.tgt_div = run.act_div = run.ep_div = 1
    run.lr, run.beta1, run.beta2, run.eps, run.tau = 3e-3, 0.9, 0.999, 1e-8, 0.07
    return run


def _dsr_run(_lib):
    run = _lib.DSRTargets()
    for name in ('successor', 'value', 'table', 'state_index', 'next_index', 'actions',
                 'nonterminal', 'targets', 'took', 'train'):
        setattr(run, name, FAKE)
    run.n, run.n_actions, run.n_outputs, run.is_float64, run.gamma = 0, 4, 20, 1, 0.9
    return run


def test_dsr_targets_argument_checks():
    from cobel_amd import _lib
    lib = _lib.lib()
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_dsr_targets(None, None))
    for name in ('successor', 'value', 'table', 'state_index', 'next_index', 'actions',
                 'nonterminal', 'targets', 'took', 'train'):
        run = _dsr_run(_lib)
        setattr(run, name, None)
        with pytest.raises(AssertionError):
            _lib.check(lib.cobel_dsr_targets(C.byref(run), None))
    for field, bad in (('n_actions', 0), ('n_actions', 9), ('n_outputs', 0), ('n', -1)):
        run = _dsr_run(_lib)
        setattr(run, field, bad)
        with pytest.raises(IndexError):
            _lib.check(lib.cobel_dsr_targets(C.byref(run), None))
    for A, O in ((1, 1), (8, 33), (5, 1000)):        # every accepted extreme, nothing to do: OK
        run = _dsr_run(_lib)
        run.n_actions, run.n_outputs = A, O
        assert lib.cobel_dsr_targets(C.byref(run), None) == _lib.OK


def test_mlp_argument_checks():
    from cobel_amd import _lib
    lib = _lib.lib()
    # nothing to do: OK, before any launch
    assert lib.cobel_mlp_forward(C.byref(_forward_run(_lib)), None) == _lib.OK
    assert lib.cobel_mlp_fit(C.byref(_fit_run(_lib)), None) == _lib.OK
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_forward(None, None))
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_fit(None, None))

    run = _fit_run(_lib)
    run.ep_rows = 5                                   # at most four extra rows
    with pytest.raises(IndexError):
        _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
    run = _fit_run(_lib)
    run.ep_rows = -1
    with pytest.raises(IndexError):
        _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
    for layer in range(3):                            # a blend needs all six target tensors
        for field in ('w_target', 'b_target'):
            run = _fit_run(_lib)
            getattr(run, field)[layer] = None
            with pytest.raises(AssertionError):
                _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
            run.tau = 0.0                             # ... and none without one
            assert lib.cobel_mlp_fit(C.byref(run), None) == _lib.OK
    run = _fit_run(_lib)                              # a table supplies ONE extra row
    run.ep_table = run.ep_index = run.ep_out = FAKE
    run.ep_rows = 1
    assert lib.cobel_mlp_fit(C.byref(run), None) == _lib.OK
    run.ep_rows = 2
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
    run.ep_table, run.ep_dense = None, FAKE           # (dense rows: up to four)
    assert lib.cobel_mlp_fit(C.byref(run), None) == _lib.OK
    run.ep_dense = None                               # extra rows asked for, none given
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
    run.ep_rows = 0                                   # ep_rows = 0: ep_out is simply not written
    assert lib.cobel_mlp_fit(C.byref(run), None) == _lib.OK
    for field in ('in_div', 'tgt_div', 'act_div', 'ep_div'):
        run = _fit_run(_lib)
        setattr(run, field, 0)
        with pytest.raises(IndexError):
            _lib.check(lib.cobel_mlp_fit(C.byref(run), None))
    run = _fit_run(_lib)
    run.w[1] = FAKE + 8                               # the 64-wide matrices: whole vector loads
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_fit(C.byref(run), None))

    for field in ('net_div', 'in_div', 'act_div'):
        run = _forward_run(_lib)
        setattr(run, field, 0)
        with pytest.raises(IndexError):
            _lib.check(lib.cobel_mlp_forward(C.byref(run), None))
    run = _forward_run(_lib)
    run.in_table = FAKE                               # a table without row numbers
    with pytest.raises(AssertionError):
        _lib.check(lib.cobel_mlp_forward(C.byref(run), None))

    lds = C.c_int32()
    for D, O in ((0, 4), (33, 4), (4, 33), (4, 0)):
        with pytest.raises(NotImplementedError):
            _lib.check(lib.cobel_mlp_query(D, 64, 64, O, 32, 1, C.byref(lds)))
        for call, make in ((lib.cobel_mlp_forward, _forward_run), (lib.cobel_mlp_fit, _fit_run)):
            run = make(_lib)
            run.n_inputs, run.n_outputs = D, O
            with pytest.raises(NotImplementedError):
                _lib.check(call(C.byref(run), None))
    for D, O in ((1, 1), (32, 32)):
        _lib.check(lib.cobel_mlp_query(D, 64, 64, O, 32, 1, C.byref(lds)))
        assert 50000 < lds.value <= 53 * 1024         # activations only, whatever the shape
        _lib.check(lib.cobel_mlp_query(D, 64, 64, O, 32, 0, C.byref(lds)))
        assert 25000 < lds.value <= 27 * 1024


def _dqn_run(_lib):
    run = _lib.DQNReplay()
    for field in (run.w, run.b, run.w_target, run.b_target, run.m_w, run.m_b, run.v_w, run.v_b):
        for k in range(3):
            field[k] = FAKE
    run.steps = run.states = run.next_states = run.actions = run.rewards = run.nonterminal = FAKE
    run.n, run.n_inputs, run.n_hidden1, run.n_hidden2, run.n_actions, run.batch = 0, 9, 64, 64, 4, 32
    run.is_float64 = 1
    run.gamma, run.lr, run.beta1, run.beta2, run.eps, run.tau = 0.9, 3e-3, 0.9, 0.999, 1e-8, 0.07
    return run


def test_dqn_replay_argument_checks():
    from cobel_amd import _lib
    lib = _lib.lib()

    def call(run):
        _lib.check(lib.cobel_dqn_replay(C.byref(run), None))

    call(_dqn_run(_lib))                              # nothing to do: OK, before any launch
    run = _dqn_run(_lib)                              # the batch as table rows ...
    run.states = run.next_states = None
    run.state_index = run.next_index = run.obs_table = FAKE
    call(run)
    run.batch_slots, run.ring_slots = FAKE, 40        # ... which the rings' slots do not go with
    with pytest.raises(AssertionError):
        call(run)
    for missing in ('next_index', 'obs_table'):
        run = _dqn_run(_lib)
        run.state_index = run.next_index = run.obs_table = FAKE
        setattr(run, missing, None)
        with pytest.raises(AssertionError):
            call(run)
    run = _dqn_run(_lib)                              # q_out: the row number of every instance
    run.q_out = run.obs_table = FAKE
    with pytest.raises(AssertionError):
        call(run)
    run.obs_index = FAKE
    call(run)
    run.obs_table = None
    with pytest.raises(AssertionError):
        call(run)
    run = _dqn_run(_lib)                              # slots into rings of no rows
    run.batch_slots = FAKE
    with pytest.raises(IndexError):
        call(run)
    run.ring_slots = 1
    call(run)
    for field, layer in (('w', 1), ('w', 2), ('w_target', 1), ('w_target', 2)):
        run = _dqn_run(_lib)                          # the 64-wide matrices: whole vector loads
        getattr(run, field)[layer] = FAKE + 8
        with pytest.raises(AssertionError):
            call(run)
    for field, bad in (('n_actions', 9), ('n_actions', 0), ('batch', 31), ('n_hidden1', 32),
                       ('n_hidden2', 32), ('n_inputs', 33)):
        run = _dqn_run(_lib)
        setattr(run, field, bad)
        with pytest.raises(NotImplementedError):
            call(run)
    for A in (1, 8):                                  # every accepted action count
        run = _dqn_run(_lib)
        run.n_actions = A
        call(run)
