"""cobel_dqn_replay with activation = 1 (tanh on both hidden layers; the streaming kernel,
k_dqn_replay in csrc/mlp_fit.hip, at every width) against the plain float64 restatement of
tests/mlp_tanh_common.py (itself checked against torch autograd + torch.optim.Adam by
tests/test_host_dqn_tanh.py), built like tests/test_gpu_dqn_replay_edges.py: at most 7 instances a
launch, all 24 state tensors and q_out framed by sentinels, the reference of a launch started from
the device state read back before it, the top-two gap of every drawn sample asserted per launch.

Shapes (D, A): the step robot's (2, 4) and the wheel robot's (3, 3) of the Continuous2D demo,
(6, 4) and (9, 3) — where a ReLU step of four actions in float64 takes the staging form and where
it does not; tanh takes the streaming form at both, confirmed through cobel_dqn_replay_query with
the form pinned — and (32, 8), the widest of both.

Tolerances.  float64: gradients 1e-12 (max-norm relative per tensor), everything else rtol 1e-9 /
atol 1e-12.  float32: no bound of its own — per case the kernel's error against the float64
reference must stay within mlp_common.f32_bound (factor 4, floor 64 * 2^-24) of the error torch's
float32 on the CPU makes evaluating the same tanh network on the same inputs; an instance that
starts from zero second moments is held link by link under the same bound, as in
tests/test_gpu_dqn_replay_edges.py (Adam divides by |g| + 1e-8 there).  The worst figures per shape
are printed at the end of the module; docs/MEASUREMENTS.md section 21 quotes them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402
import mlp_tanh_common as tc  # noqa: E402
from mlp_gpu_common import Framed, _dev, _host, _launch, _np, _torch_dtype, agree  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = ['D%d-A%d' % s for s in tc.SHAPES]
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, tau=0.07)
GAMMA = 0.9
KINDS = {'p': 'P', 't': 'T', 'm': 'M', 'v': 'V'}
FIGURES = {}      # (what, dtype, D, A) -> (kernel error, torch float32 error), the worst seen
TANH, RELU = 1, 0

shapes = pytest.mark.parametrize('D,A', tc.SHAPES, ids=IDS)
dtypes = pytest.mark.parametrize('name', ['f64', 'f32'])


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    yield torch
    worst = {}
    for (what, name, D, A), (kernel, yard) in FIGURES.items():
        ratio = kernel / mc.f32_bound(yard)
        if (D, A) not in worst or ratio > worst[D, A][0]:
            worst[D, A] = (ratio, what, kernel, yard)
    for (D, A), (ratio, what, kernel, yard) in sorted(worst.items()):
        print('dqn-tanh figure f32 D %2d A %d  worst at %-7s kernel %.2e  torch-f32 %.2e  (%.2f of '
              'its allowance)' % (D, A, what, kernel, yard, ratio))


def pin_stream(monkeypatch, name, D, A):
    """Pins the streaming form and confirms through the query that it is the one a launch takes."""
    from cobel_amd import _lib
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_DQN_KERNEL', 'stream')
    lds = C.c_int32()
    _lib.check(_lib.lib().cobel_dqn_replay_query(D, 64, 64, A, 32, int(name == 'f64'), C.byref(lds)))
    # fit_lds_elems of csrc/mlp_fit.hip: x and q [32][33], h1 and h2 [32][66], qt [32][8], 64 + 2 + 32
    elems = 2 * 32 * 33 + 2 * 32 * 66 + 32 * 8 + 64 + 2 + 32
    assert lds.value == elems * (8 if name == 'f64' else 4), lds.value


def _t32_forward(torch, p, x):
    h = torch.tanh(x @ p['w1'].T + p['b1'])
    h = torch.tanh(h @ p['w2'].T + p['b2'])
    return h @ p['w3'].T + p['b3']


def _t32_step(torch, net, b, hyper, gamma, ddqn, obs):
    """This package's PyTorch replay path on ONE instance in float32 on the CPU: the new state as
    {'p', 'm', 'v', 't'}, the gradient, and q_out (or None)."""
    with torch.no_grad():
        y = _t32_forward(torch, net['p'], b['states']).clone()
        boot = _t32_forward(torch, net['t'], b['next_states'])
        pick = (_t32_forward(torch, net['p'], b['next_states']) if ddqn else boot).argmax(dim=1)
        boot = torch.gather(boot, 1, pick[:, None])[:, 0]
        boot = torch.where(b['nonterminal'] != 0, boot, torch.zeros_like(boot))
        y.scatter_(1, b['actions'][:, None], (b['rewards'] + boot * b['nonterminal'] * gamma)[:, None])
    leaf = {k: a.clone().requires_grad_() for k, a in net['p'].items()}
    opt = torch.optim.Adam([leaf[k] for k in mc.KEYS], lr=hyper['lr'], eps=hyper['eps'],
                           betas=(hyper['beta1'], hyper['beta2']), weight_decay=hyper['weight_decay'])
    for k in mc.KEYS:     # (the optimizer counts the steps BEFORE this one)
        opt.state[leaf[k]] = {'step': torch.tensor(float(net['steps']) - 1.0),
                              'exp_avg': net['m'][k].clone(), 'exp_avg_sq': net['v'][k].clone()}
    ((_t32_forward(torch, leaf, b['states']) - y) ** 2).mean().backward()
    grad = {k: leaf[k].grad.clone() for k in mc.KEYS}
    opt.step()
    out = {'p': {k: leaf[k].detach() for k in mc.KEYS},
           'm': {k: opt.state[leaf[k]]['exp_avg'] for k in mc.KEYS},
           'v': {k: opt.state[leaf[k]]['exp_avg_sq'] for k in mc.KEYS}, 't': net['t']}
    if hyper['tau'] != 0.0:
        out['t'] = {k: torch.lerp(net['t'][k], out['p'][k], hyper['tau']) for k in mc.KEYS}
    q = None if obs is None else _t32_forward(torch, out['p'], torch.from_numpy(obs)[None])[0]
    return out, grad, q


class Replay:
    """The state of a mlp_tanh_common.dqn_case on the device, every tensor framed; ``run`` launches
    cobel_dqn_replay once with the given activation and holds every instance against the
    reference."""

    def __init__(self, torch, case, name):
        self.torch, self.case, self.name = torch, case, name
        self.n, self.D, self.A = case['n'], case['D'], case['A']
        self.framed = {(kind, k): Framed(torch, case[stack][k].shape, _torch_dtype(torch, name))
                       for kind, stack in KINDS.items() for k in mc.KEYS}
        self.d_table = _dev(torch, case['table'])
        self.reset()

    def reset(self):
        for (kind, k), f in self.framed.items():
            f.view.copy_(_dev(self.torch, self.case[KINDS[kind]][k]))
        self.steps = np.array(self.case['steps'], dtype=np.float64)

    def stack(self, kind):
        return {k: self.framed[kind, k].view for k in mc.KEYS}

    def nets(self, kind):
        host = {k: _host(self.framed[kind, k].view).astype(np.float64) for k in mc.KEYS}
        return [{k: host[k][j] for k in mc.KEYS} for j in range(self.n)]

    def redraw(self, seed, ddqn):
        tc.dqn_draw_batch(self.case, seed, ddqn, online=self.nets('p'), target=self.nets('t'))
        self.d_table = _dev(self.torch, self.case['table'])

    def batch(self, mode='gathered', ring_slots=40, spoil=()):
        """The case's batch on the device by the struct's field names: 'gathered', 'rings' of
        ``ring_slots`` > 32 rows (slots 0 and the last both named, every row no slot names NaN, its
        action 2^40) or 'index'.  Instances in ``spoil`` get NaN everywhere."""
        torch, c, n, dt = self.torch, self.case, self.n, _np(self.name)
        rows = [tc.dqn_rows(c, j, dt) for j in range(n)]
        g = {key: np.stack([r[key] for r in rows])
             for key in ('states', 'next_states', 'actions', 'rewards', 'nonterminal')}
        for j in spoil:
            for key in ('states', 'next_states', 'rewards', 'nonterminal'):
                g[key][j] = np.nan
        if mode == 'index':
            g['state_index'], g['next_index'] = c['state_index'], c['next_index']
            del g['states'], g['next_states']
        elif mode == 'rings':
            R, rng = ring_slots, np.random.default_rng([c['seed'], ring_slots])
            slots = np.zeros((n, mc.B), dtype=np.int32)
            for j in range(n):
                named = np.concatenate([[0, R - 1], 1 + rng.permutation(R - 2)[:mc.B - 2]])
                slots[j] = rng.permutation(named)
            rings = {}
            for key, a in g.items():
                rings[key] = np.full((n, R) + a.shape[2:], 2 ** 40 if key == 'actions' else np.nan,
                                     dtype=a.dtype)
                for j in range(n):
                    rings[key][j, slots[j]] = a[j]
            g = dict(rings, batch_slots=slots)
        out = {key: _dev(torch, a) for key, a in g.items()}
        if mode == 'rings':
            out['ring_slots'] = ring_slots
        return out

    def launch(self, batch, hyper, gamma, ddqn, activation, active=None, obs_index=None):
        """One launch; returns (state before, state after [+ 'q_out'], the q_out frame)."""
        from cobel_amd import _lib
        torch, n = self.torch, self.n
        before = {key: _host(f.view) for key, f in self.framed.items()}
        d_steps = _dev(torch, self.steps)
        d_active = None if active is None else _dev(torch, np.asarray(active, dtype=np.uint8))
        q = d_obs = None
        if obs_index is not None:
            q = Framed(torch, (n, self.A), _torch_dtype(torch, self.name))
            d_obs = _dev(torch, np.asarray(obs_index, dtype=np.int32))
        table = self.d_table if q is not None or 'state_index' in batch else None
        run = tc.fill_dqn_replay(_lib, self.stack('p'), self.stack('t'), self.stack('m'),
                                 self.stack('v'), d_steps, batch, n, self.D, self.A, hyper, gamma,
                                 ddqn, active=d_active, obs_index=d_obs, obs_table=table,
                                 q_out=None if q is None else q.view)
        if activation is not None:
            run.activation = activation
        _launch('cobel_dqn_replay', run)
        torch.cuda.synchronize()
        assert all(f.intact() for f in self.framed.values()) and (q is None or q.intact())
        assert np.array_equal(_host(d_steps), self.steps)
        after = {key: _host(f.view) for key, f in self.framed.items()}
        if q is not None:
            after['q_out'] = _host(q.view)
        return before, after, q

    def run(self, batch, hyper=HYPER, gamma=GAMMA, ddqn=False, active=None, obs_index=None,
            gradient=False, where=None):
        """One tanh launch held against mlp_tanh_common.dqn_step from the state it started from
        (``gradient``: exp_avg / (1 - beta1) against the reference's gradient as well, which it is
        after one step from zero moments).  Returns the state after the launch."""
        torch, c, n, D, A, name = self.torch, self.case, self.n, self.D, self.A, self.name
        before, after, q = self.launch(batch, hyper, gamma, ddqn, TANH, active, obs_index)
        figure = (name, D, A)
        c1, c2 = 1.0 - hyper['beta1'], 1.0 - hyper['beta2']
        if name == 'f32':     # the constants as the kernel holds them
            c1, c2 = float(np.float32(c1)), float(np.float32(c2))
        for j in range(n):
            if active is not None and not active[j]:
                for key in before:
                    assert after[key][j].tobytes() == before[key][j].tobytes(), (where, j, key)
                assert q is None or q.untouched(j), (where, j)
                continue
            net = {kind: {k: before[kind, k][j].astype(np.float64) for k in mc.KEYS} for kind in KINDS}
            net['steps'] = float(self.steps[j])
            b = tc.dqn_rows(c, j)
            if j not in c['exempt']:
                gap = tc.dqn_gap(net['p'], net['t'], b['next_states'], ddqn)
                assert gap >= tc.GAP, (where, j, 'top-two gap %.3e' % gap)
            obs = None if q is None else c['table'][obs_index[j]].astype(_np(name))
            ref, g, q_ref = tc.dqn_step(net, b, hyper, gamma, ddqn, obs)
            t32 = g32 = q32 = None
            if name == 'f32':
                n32 = {kind: {k: torch.from_numpy(before[kind, k][j].copy()) for k in mc.KEYS}
                       for kind in KINDS}
                b32 = {key: torch.from_numpy(np.ascontiguousarray(a))
                       for key, a in tc.dqn_rows(c, j, np.float32).items()}
                t32, g32, q32 = _t32_step(torch, dict(n32, steps=net['steps']), b32, hyper, gamma,
                                          ddqn, obs)
            # float32 from ZERO second moments: held link by link (the module's docstring)
            steep = name == 'f32' and not any(before['v', k][j].any() for k in mc.KEYS)
            if steep:
                def f64(stack):
                    return {k: np.asarray(_host(a) if hasattr(a, 'detach') else a, dtype=np.float64)
                            for k, a in stack.items()}

                def links(m, v, p):
                    out = {'p': mc.adam_from_moments(net['p'], f64(m), f64(v), net['steps'],
                                                     hyper['lr'], hyper['beta1'], hyper['beta2'],
                                                     hyper['eps'])}
                    out['t'] = mc.blend(net['t'], f64(p), hyper['tau'])
                    out['q'] = None if q is None else \
                        tc.forward(f64(p), obs.astype(np.float64)[None])[2][0]
                    return out
                mine = {kind: {k: after[kind, k][j] for k in mc.KEYS} for kind in 'pmv'}
                own = links(mine['m'], mine['v'], mine['p'])
                own32 = links(t32['m'], t32['v'], t32['p'])
            for kind in KINDS:
                for k in mc.KEYS:
                    got, at = after[kind, k][j], (where, j, kind, k)
                    if kind == 't' and hyper['tau'] == 0.0:      # no blend: every byte stays
                        assert got.tobytes() == before[kind, k][j].tobytes(), at
                        continue
                    assert np.isfinite(got).all(), at
                    if steep and kind in 'pt':
                        agree(FIGURES, (kind + '-own',) + figure, name, got, own[kind][k], t32[kind][k],
                              where=at, after_adam=True, t32_ref=own32[kind][k])
                        continue
                    agree(FIGURES, (kind,) + figure, name, got, ref[kind][k],
                          t32[kind][k] if t32 else None, where=at, after_adam=True)
                    if gradient and kind in 'mv':
                        cg = c1 if kind == 'm' else c2
                        power = (lambda a: a) if kind == 'm' else (lambda a: a * a)
                        agree(FIGURES, ('grad' if kind == 'm' else 'gradsq',) + figure, name,
                              got.astype(np.float64) / cg, power(g[k]),
                              power(g32[k]) if g32 else None, grad=True, where=at)
            if q is not None:
                assert np.isfinite(after['q_out'][j]).all(), (where, j)
                if steep:
                    agree(FIGURES, ('q-own',) + figure, name, after['q_out'][j], own['q'], q32,
                          where=(where, j, 'q_out'), after_adam=True, t32_ref=own32['q'])
                else:
                    agree(FIGURES, ('q_out',) + figure, name, after['q_out'][j], q_ref, q32,
                          where=(where, j, 'q_out'), after_adam=True)
        return after


def _case(key, D, A, name):
    return tc.gpu_case(key, D, A, _np(name))


# ---------------------------------------------------------------------------------------------
@shapes
@dtypes
def test_gradients_in_isolation(torch_cuda, monkeypatch, name, D, A):
    """One step from zero moments, steps = 1, no weight decay, DQN and DDQN: exp_avg / (1 - beta1)
    is the gradient the kernel formed — through tanh forward and (1 - h * h) backward — tensor by
    tensor against grads(); exp_avg_sq / (1 - beta2) its square."""
    pin_stream(monkeypatch, name, D, A)
    for ddqn in (False, True):
        rp = Replay(torch_cuda, _case(('backward', ddqn), D, A, name), name)
        rp.run(rp.batch(), hyper=dict(HYPER, tau=0.0), ddqn=ddqn, gradient=True, where=ddqn)


@pytest.mark.parametrize('option', mc.DQN_OPTIONS)
@shapes
@dtypes
def test_options_over_three_steps(torch_cuda, monkeypatch, name, D, A, option):
    """Three consecutive steps on the state the kernel left in device memory, one option away from
    the base form (DQN, gamma 0.9, tau 0.07, no weight decay), each against the reference started
    from the state read back before it, on a table and batch drawn anew so that the top-two gap
    holds for that state."""
    pin_stream(monkeypatch, name, D, A)
    hyper, gamma, ddqn = dict(HYPER), GAMMA, option == 'ddqn'
    if option == 'weight_decay':
        hyper['weight_decay'] = 1e-3
    elif option in ('tau0', 'tau1'):
        hyper['tau'] = float(option[-1])
    elif option == 'gamma0':
        gamma = 0.0
    case = _case(('options', option), D, A, name)
    rp = Replay(torch_cuda, case, name)
    for it in range(3):
        if it:
            rp.redraw(case['seed'] + 100 * it, ddqn)
        rp.run(rp.batch(), hyper=hyper, gamma=gamma, ddqn=ddqn, where=(option, it))
        rp.steps += 1.0


@shapes
@dtypes
def test_input_modes_agree(torch_cuda, monkeypatch, name, D, A):
    """The same case gathered, through rings of 40 rows + batch_slots, and as rows of the
    observation table (q_out asked for in all three): each against the reference, in float64 the
    three against each other; nothing non-finite comes out of the NaN in the rows no slot names."""
    pin_stream(monkeypatch, name, D, A)
    rp = Replay(torch_cuda, _case('modes', D, A, name), name)
    results = {}
    for mode in ('gathered', 'rings', 'index'):
        rp.reset()
        results[mode] = rp.run(rp.batch(mode), ddqn=True, obs_index=[12, 0, 7, 7, 3], where=mode)
    if name == 'f64':
        for mode in ('rings', 'index'):
            for key, a in results[mode].items():
                assert np.allclose(a, results['gathered'][key], rtol=1e-9, atol=1e-12), (mode, key)


@shapes
@dtypes
def test_an_instance_that_sits_out(torch_cuda, monkeypatch, name, D, A):
    """active = 1 0 1 0 0 1 1 and NULL: an instance that sits out keeps every byte of its 24
    tensors and its q_out row, with steps = 0 and NaN all over its batch; the others match."""
    pin_stream(monkeypatch, name, D, A)
    rp = Replay(torch_cuda, _case('sit_out', D, A, name), name)
    for active in ([1, 0, 1, 0, 0, 1, 1], None):
        rp.reset()
        idle = [j for j in range(7) if active is not None and not active[j]]
        rp.steps[idle] = 0.0
        rp.run(rp.batch('gathered', spoil=idle), active=active, obs_index=[0, 12, 1, 2, 3, 4, 5],
               where=active)


@shapes
@dtypes
def test_q_out_and_exact_ddqn_ties(torch_cuda, monkeypatch, name, D, A):
    """q_out is forward(UPDATED parameters, row obs_index[i]) through tanh — the first and the last
    row of the table among them; and DDQN's first-maximum rule on ties that are exact in any
    summation order (zero rows of w3, equal b3: tanh's rounding cannot break them)."""
    pin_stream(monkeypatch, name, D, A)
    last = mc.TABLE_ROWS - 1
    rp = Replay(torch_cuda, _case('q_out', D, A, name), name)
    rp.run(rp.batch(), obs_index=[0, last, 5, last, 0], where='q_out')
    rp = Replay(torch_cuda, _case('ties', D, A, name), name)
    rp.run(rp.batch(), ddqn=True, obs_index=[1, 2, 3], where='ties')


@shapes
@dtypes
def test_saturated_units_pass_nothing_back(torch_cuda, monkeypatch, name, D, A):
    """One hidden unit of each layer has bias 40: h == 1.0 exactly in both dtypes, 1 - h * h == 0,
    so after one step from zero moments the exp_avg rows of its incoming weights and of its bias
    are exactly zero — a backward pass that multiplied in another order, or by 1 - h^2 of a
    recomputed h, would leave rounding there — while its outgoing column matches the reference."""
    pin_stream(monkeypatch, name, D, A)
    case = _case('saturation', D, A, name)
    rp = Replay(torch_cuda, case, name)
    after = rp.run(rp.batch(), hyper=dict(HYPER, tau=0.0), gradient=True, where='saturation')
    u1, u2 = tc.SATURATED
    zero = np.zeros((), dtype=_np(name))
    for j in range(case['n']):
        for kind in 'mv':
            assert np.array_equal(after[kind, 'w1'][j][u1], np.zeros(D, dtype=_np(name))), (j, kind)
            assert np.array_equal(after[kind, 'b1'][j][u1], zero), (j, kind)
            assert np.array_equal(after[kind, 'w2'][j][u2], np.zeros(64, dtype=_np(name))), (j, kind)
            assert np.array_equal(after[kind, 'b2'][j][u2], zero), (j, kind)
        # (the outgoing columns were held against the reference by run(); they are not zero)
        assert after['m', 'w2'][j][:, u1].any() and after['m', 'w3'][j][:, u2].any(), j


@pytest.mark.parametrize('D,A', [(6, 4), (9, 3)], ids=['D6-A4', 'D9-A3'])
@dtypes
def test_activation_zero_is_the_launch_it_always_was(torch_cuda, monkeypatch, name, D, A):
    """A ReLU case launched with activation = 0 written and with the field left as the struct's
    constructor leaves it: the same bytes in all 24 tensors and q_out, in the form the dispatcher
    chooses by itself and in each pinned form; and the same case with activation = 1 differs."""
    torch = torch_cuda
    case = mc.dqn_gpu_case('q_out', D, A, _np(name))
    rp = Replay(torch, case, name)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    for form in (None, 'stream', 'lds'):
        if form is None:
            monkeypatch.delenv('COBEL_DEBUG_DQN_KERNEL', raising=False)
        else:
            monkeypatch.setenv('COBEL_DEBUG_DQN_KERNEL', form)
        results = []
        for activation in (None, RELU):
            rp.reset()
            results.append(rp.launch(rp.batch(), HYPER, GAMMA, True, activation,
                                     obs_index=[0, 1, 2, 3, 12])[1])
        for key, a in results[0].items():
            assert a.tobytes() == results[1][key].tobytes(), (form, key)
    monkeypatch.setenv('COBEL_DEBUG_DQN_KERNEL', 'stream')
    rp.reset()
    other = rp.launch(rp.batch(), HYPER, GAMMA, True, TANH, obs_index=[0, 1, 2, 3, 12])[1]
    assert not np.array_equal(other['m', 'w1'], results[1]['m', 'w1'])
