"""The tanh form of the DQN replay step without a GPU: its float64 restatement
(tests/mlp_tanh_common.py) against torch autograd + torch.optim.Adam on the CPU, the seed searches
of the cases the GPU test draws, the recogniser ``StackedTorchNetwork._mlp3_activation``, the
``activation`` field's place in cobel_dqn_replay_t, and the refusals that return before a launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_tanh_common as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3, tau=0.07)
FAKE = 0x10000           # a 16-byte aligned address nobody dereferences


def torch_forward(torch, tp, x):
    h = torch.tanh(x @ tp['w1'].T + tp['b1'])
    h = torch.tanh(h @ tp['w2'].T + tp['b2'])
    return h @ tp['w3'].T + tp['b3']


@pytest.mark.parametrize('ddqn', [False, True])
@pytest.mark.parametrize('D,A', [(2, 4), (3, 3), (31, 6)])
def test_tanh_reference_matches_torch_autograd_and_adam(D, A, ddqn):
    """Three consecutive dqn_step calls against the PyTorch replay path restated in float64 on the
    CPU (targets = forward(s).clone(), scatter_ of r + boot * nt * gamma, MSE, autograd,
    torch.optim.Adam, lerp) from a pre-seeded optimizer state with weight decay, a new batch per
    step: gradients to 1e-12 (max-norm relative per tensor), parameters, moments, the blended
    target, the Q-learning targets and q_out to rtol 1e-9 / atol 1e-12."""
    import torch
    gamma = 0.8
    c = tc.dqn_case(10 * D + A, 2, D, A, np.float64, ddqn=ddqn)
    for j in range(2):
        net = {'p': tc.one(c['P'], j), 't': tc.one(c['T'], j), 'm': tc.one(c['M'], j),
               'v': tc.one(c['V'], j), 'steps': float(c['steps'][j])}
        tp = {k: torch.tensor(a, requires_grad=True) for k, a in net['p'].items()}
        tt = {k: torch.tensor(a) for k, a in net['t'].items()}
        opt = torch.optim.Adam([tp[k] for k in tc.KEYS], lr=HYPER['lr'], eps=HYPER['eps'],
                               betas=(HYPER['beta1'], HYPER['beta2']),
                               weight_decay=HYPER['weight_decay'])
        for k in tc.KEYS:     # (the optimizer counts the steps before this one)
            opt.state[tp[k]] = {'step': torch.tensor(net['steps'] - 1.0),
                                'exp_avg': torch.tensor(net['m'][k]),
                                'exp_avg_sq': torch.tensor(net['v'][k])}
        for it in range(3):
            if it:
                tc.dqn_draw_batch(c, c['seed'] + 100 * it, ddqn, None, None)
            b = tc.dqn_rows(c, j)
            obs = c['table'][j]
            out, g, q_out = tc.dqn_step(net, b, HYPER, gamma, ddqn, obs)
            s, ns = torch.tensor(b['states']), torch.tensor(b['next_states'])
            a, r = torch.tensor(b['actions']), torch.tensor(b['rewards'])
            nt = torch.tensor(b['nonterminal'])
            with torch.no_grad():
                targets = torch_forward(torch, tp, s).clone()
                boot = torch_forward(torch, tt, ns)
                pick = (torch_forward(torch, tp, ns) if ddqn else boot).argmax(dim=1)
                boot = torch.gather(boot, 1, pick[:, None])[:, 0]
                new = r + boot * nt * gamma
                targets.scatter_(1, a[:, None], new[:, None])
            assert np.allclose(tc.dqn_targets(net['p'], net['t'], b['next_states'], b['rewards'],
                                              b['nonterminal'], gamma, ddqn), new.numpy(),
                               rtol=1e-9, atol=1e-12)
            opt.zero_grad()
            ((torch_forward(torch, tp, s) - targets) ** 2).mean().backward()
            for k in tc.KEYS:
                assert tc.rel_err(g[k], tp[k].grad.numpy()) <= 1e-12, (j, it, k)
            opt.step()
            with torch.no_grad():
                for k in tc.KEYS:
                    tt[k] = torch.lerp(tt[k], tp[k], HYPER['tau'])
                want_q = torch_forward(torch, tp, torch.tensor(obs)[None])[0]
            for k in tc.KEYS:
                st = opt.state[tp[k]]
                for name, got, want in (('p', out['p'][k], tp[k].detach()),
                                        ('m', out['m'][k], st['exp_avg']),
                                        ('v', out['v'][k], st['exp_avg_sq']), ('t', out['t'][k], tt[k])):
                    assert np.allclose(got, want.numpy(), rtol=1e-9, atol=1e-12), (j, it, k, name)
                assert float(st['step']) == net['steps']
            assert np.allclose(q_out, want_q.numpy(), rtol=1e-9, atol=1e-12)
            net = dict(out, steps=net['steps'] + 1.0)


@pytest.mark.parametrize('D,A', tc.SHAPES)
def test_every_gpu_case_is_found_and_holds_its_conditions(D, A):
    """Every case tests/test_gpu_dqn_replay_tanh.py draws, in both dtypes: the seed search ends
    within its tries and is deterministic, the top-two gap holds on the tanh network for every
    instance that is not exempt, the planted ties are exact, and the saturated units are exactly
    1.0 on every row in float64 and float32 arithmetic."""
    for key, kw in tc.gpu_cases(D, A).items():
        for dt in (np.float64, np.float32):
            c = tc.gpu_case(key, D, A, dt)
            assert kw['seed'] <= c['seed'] < kw['seed'] + 64 and c['n'] == kw['n'], key
            for j in set(range(kw['n'])) - c['exempt']:
                gap = tc.dqn_gap(tc.one(c['P'], j), tc.one(c['T'], j),
                                 tc.dqn_rows(c, j)['next_states'], kw['ddqn'])
                assert gap >= tc.GAP, (key, j)
            assert tc.gpu_case(key, D, A, dt)['seed'] == c['seed']
        if key == 'ties':
            for j, first in ((0, 0), (1, 0)):
                q = tc.forward(tc.one(c['P'], j), tc.dqn_rows(c, j)['next_states'])[2]
                assert (tc.first_maximum(q.T[None])[0] == first).all()
                assert (q[:, 0] == q[:, A - 1]).all()
        if key == 'saturation':
            for j in range(kw['n']):
                x = tc.dqn_rows(c, j, dt)['states']
                p = {k: a[j] for k, a in c['P'].items()}
                h1 = np.tanh(x @ p['w1'].T + p['b1'])
                h2 = np.tanh(h1 @ p['w2'].T + p['b2'])
                assert h1.dtype == dt and (h1[:, tc.SATURATED[0]] == 1.0).all()
                assert (h2[:, tc.SATURATED[1]] == 1.0).all()
                g = tc.dqn_step({'p': tc.one(c['P'], j), 't': tc.one(c['T'], j),
                                 'm': tc.one(c['M'], j), 'v': tc.one(c['V'], j), 'steps': 1.0},
                                tc.dqn_rows(c, j), dict(HYPER, weight_decay=0.0), 0.9, False)[1]
                assert not g['w1'][tc.SATURATED[0]].any() and g['b1'][tc.SATURATED[0]] == 0.0
                assert not g['w2'][tc.SATURATED[1]].any() and g['b2'][tc.SATURATED[1]] == 0.0
                assert g['w2'][:, tc.SATURATED[0]].any() and g['w3'][:, tc.SATURATED[1]].any()


# ---------------------------------------------------------------------------------------------
def _models(torch, dtype):
    nn = torch.nn

    class Demo(nn.Module):              # the shape of the reference's demo models: a custom forward
        def __init__(self, act, act2=None, n_in=2, n_out=4):
            super().__init__()
            self.layer_dense_1 = nn.Linear(n_in, 64)
            self.layer_dense_2 = nn.Linear(64, 64)
            self.layer_output = nn.Linear(64, n_out)
            self.act, self.act2 = act, act if act2 is None else act2
            self.to(dtype)

        def forward(self, x):
            x = self.act(self.layer_dense_1(x))
            x = self.act2(self.layer_dense_2(x))
            return self.layer_output(x)

    def seq(*acts, n_in=3, n_out=3):
        return nn.Sequential(nn.Linear(n_in, 64), acts[0], nn.Linear(64, 64), acts[1],
                             nn.Linear(64, n_out)).to(dtype)
    return Demo, seq


@pytest.mark.parametrize('dtype_name', ['float64', 'float32'])
def test_recogniser_tells_tanh_from_its_look_alikes(dtype_name):
    """``_mlp3_activation()``: ('tanh', names) for the demo's custom-forward tanh model and for an
    nn.Sequential with nn.Tanh, ('relu', names) where ``_mlp3_names()`` gives names, None for
    hardtanh, softsign, clamp(-1, 1) in a custom forward and mixed Tanh / ReLU; ``_mlp3_names()``
    stays None for every tanh model (ADQN and the Dyna agents route on it)."""
    import torch
    from cobel_amd.network import TorchNetwork
    nn, F = torch.nn, torch.nn.functional
    dtype = getattr(torch, dtype_name)
    Demo, seq = _models(torch, dtype)
    torch.manual_seed(3)

    def stack(model):
        return TorchNetwork(model).replicate(2)

    demo = stack(Demo(torch.tanh))
    assert demo._mlp3_activation() == ('tanh', ['layer_dense_1', 'layer_dense_2', 'layer_output'])
    assert demo._mlp3_names() is None
    assert demo._mlp3_activation() is demo._mlp3_activation()          # cached
    s = stack(seq(nn.Tanh(), nn.Tanh()))
    assert s._mlp3_activation() == ('tanh', ['0', '2', '4']) and s._mlp3_names() is None
    for relu in (stack(Demo(torch.relu)), stack(seq(nn.ReLU(), nn.ReLU()))):
        names = relu._mlp3_names()
        assert names is not None and relu._mlp3_activation() == ('relu', names)
    for act in (F.hardtanh, F.softsign, lambda v: v.clamp(-1, 1), torch.sigmoid,
                lambda v: torch.tanh(v) * 1.001):
        other = stack(Demo(act))
        assert other._mlp3_activation() is None and other._mlp3_names() is None
    for a, b in ((nn.Tanh(), nn.ReLU()), (nn.ReLU(), nn.Tanh()), (nn.Hardtanh(), nn.Hardtanh()),
                 (nn.Tanh(), nn.Softsign())):
        assert stack(seq(a, b))._mlp3_activation() is None
    assert stack(Demo(torch.tanh, torch.relu))._mlp3_activation() is None
    assert stack(Demo(torch.relu, torch.tanh))._mlp3_activation() is None
    # weights too small for a hidden unit to leave tanh's linear stretch: nothing can be told, so
    # nothing is claimed
    tiny = Demo(torch.tanh)
    with torch.no_grad():
        for p in tiny.parameters():
            p.mul_(1e-3)
    assert stack(tiny)._mlp3_activation() is None


# ---------------------------------------------------------------------------------------------
def test_activation_takes_the_reserved_field():
    """sizeof(cobel_dqn_replay_t) is what it was (three pointers of 8 bytes behind the old
    ``reserved_``, which followed ``ring_slots``), ``activation`` sits at that offset, and the
    ctypes mirror agrees with the C compiler."""
    from cobel_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cobel_hip.h"\n'
           'int main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(cobel_dqn_replay_t), '
           'offsetof(cobel_dqn_replay_t, activation), offsetof(cobel_dqn_replay_t, ring_slots), '
           'offsetof(cobel_dqn_replay_t, obs_index), COBEL_ACT_RELU, COBEL_ACT_TANH);return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'layout.c')
        with open(path, 'w') as f:
            f.write(src)
        exe = os.path.join(tmp, 'layout')
        subprocess.check_call(['cc', '-I', os.path.join(ROOT, 'include'), path, '-o', exe])
        size, act, ring, obs, relu, tanh = map(int, subprocess.check_output([exe]).split())
    R = _lib.DQNReplay
    assert size == C.sizeof(R) and act == R.activation.offset and ring == R.ring_slots.offset
    assert act == ring + 4 and obs == act + 4          # the old reserved_: between the two
    assert (relu, tanh) == (_lib.ACT_RELU, _lib.ACT_TANH) == (0, 1)
    assert not hasattr(R, 'reserved_')
    assert R().activation == 0                         # a zeroed struct asks for ReLU


def _dqn_run(_lib):
    run = _lib.DQNReplay()
    for field in (run.w, run.b, run.w_target, run.b_target, run.m_w, run.m_b, run.v_w, run.v_b):
        for k in range(3):
            field[k] = FAKE
    run.steps = run.states = run.next_states = run.actions = run.rewards = run.nonterminal = FAKE
    run.n, run.n_inputs, run.n_hidden1, run.n_hidden2, run.n_actions, run.batch = 0, 2, 64, 64, 4, 32
    run.is_float64 = 1
    run.gamma, run.lr, run.beta1, run.beta2, run.eps, run.tau = 0.9, 3e-3, 0.9, 0.999, 1e-8, 0.07
    return run


def test_activation_refusals_before_any_launch(monkeypatch):
    """activation 0 and 1 pass the checks (n = 0: nothing is launched), every other value is an
    argument error, and tanh with the staging form pinned is refused as unsupported — at a width
    where ReLU would take that form and at one where it would not."""
    from cobel_amd import _lib
    lib = _lib.lib()

    def call(run):
        _lib.check(lib.cobel_dqn_replay(C.byref(run), None))

    for ok in (_lib.ACT_RELU, _lib.ACT_TANH):
        run = _dqn_run(_lib)
        run.activation = ok
        call(run)
    for bad in (2, -1, 1 << 20):
        run = _dqn_run(_lib)
        run.activation = bad
        with pytest.raises(AssertionError):
            call(run)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    for form, refused in (('lds', True), ('stream', False)):
        monkeypatch.setenv('COBEL_DEBUG_DQN_KERNEL', form)
        for D, A in ((2, 4), (3, 3)):
            run = _dqn_run(_lib)
            run.n_inputs, run.n_actions, run.activation = D, A, _lib.ACT_TANH
            if refused:
                with pytest.raises(NotImplementedError):
                    call(run)
            else:
                call(run)
            run.activation = _lib.ACT_RELU               # ReLU: both pins are served
            call(run)
