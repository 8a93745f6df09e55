"""cobel_dqn_replay at its edges, in both hand-written forms — the parameter-staging kernel
(csrc/mlp.hip, four actions) and the streaming kernel (k_dqn_replay in csrc/mlp_fit.hip, 1 .. 8
actions) — against the plain float64 reference of tests/mlp_common.py (dqn_targets / dqn_step,
themselves checked against torch autograd + torch.optim.Adam by tests/test_host_mlp_reference.py).

Input widths on both sides of the staging form's 8 / 16 / 32 boundaries and of the streaming form's
K quarters, every action count, both dtypes (their accumulator row layouts differ): the backward
pass in isolation, planted batch contents (exact DDQN ties, terminal samples under a NaN target
network, repeated samples, one action only), the three input modes, instances that sit out, every
option over three steps carried through device memory, q_out from the UPDATED parameters, and the
two forms on the same case.  Each form is pinned with COBEL_DEBUG_DQN_KERNEL and the pin is
confirmed through cobel_dqn_replay_query.

All 24 state tensors (online and target parameters, both moments) and q_out are views into the
middle of buffers filled with a sentinel; the frames must be intact after every launch.  The
reference of a launch starts from the device state read back before it, converted to float64, so
float32 divergence cannot accumulate into a different argmax; for every drawn (not planted) sample
the reference's top-two gap is at least 1e-3 of max |Q| (mlp_common.GAP), asserted per launch.

Tolerances, as in tests/test_gpu_mlp_edges.py.  float64: gradients 1e-12 (max-norm relative per
tensor), everything else rtol 1e-9 / atol 1e-12.  float32: the kernel's error against the float64
reference must stay within 4x of the error torch's float32 on the CPU makes on the same inputs,
with 64 * 2^-24 as the floor; a float32 instance that starts from zero second moments is held
under the same bound link by link (gradient, parameters from the kernel's own moments, target and
q_out from the kernel's own parameters: Replay.run says why).  Measured figures:
docs/MEASUREMENTS.md section 15."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402
from mlp_gpu_common import (Framed, _dev, _host, _launch, _np, _t32_fit_step,  # noqa: E402
                            _t32_forward, _t32_grads, _torch_dtype, agree)

pytestmark = pytest.mark.gpu

LDS_D = (1, 8, 9, 16, 17, 32)
STREAM = [(1, 1), (7, 8), (8, 4), (9, 3), (17, 5), (24, 2), (31, 6), (32, 4)]
CONFIGS = [('lds', D, 4) for D in LDS_D] + [('stream', D, A) for D, A in STREAM]
IDS = ['%s-D%d-A%d' % c for c in CONFIGS]
DTYPES = ['f64', 'f32']
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, tau=0.07)
GAMMA = 0.9
KINDS = {'p': 'P', 't': 'T', 'm': 'M', 'v': 'V'}
FIGURES = {}      # (what, form, dtype, D, A) -> (kernel error, torch float32 error), the worst seen

configs = pytest.mark.parametrize('form,D,A', CONFIGS, ids=IDS)
dtypes = pytest.mark.parametrize('name', DTYPES)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    yield torch
    for key in sorted(FIGURES):
        print('dqn-edges figure %-7s %-6s %s D %2d A %d  kernel %.2e  torch-f32 %.2e'
              % (key + FIGURES[key]))


def staging_lds_bytes(D, name):
    """mlp_lds_elems of csrc/mlp.hip."""
    elems = 64 * 66 + 64 * D + 4 * 64 + 64 + 64 + 8 + 32 * D + 2 * 32 * 66 + 2 * 32 * 4 + 32 + 4 * 32
    return elems * (8 if name == 'f64' else 4)


def pin(monkeypatch, form, name, D, A):
    """Pins one form of the step and confirms that it is the one the library will launch."""
    from cobel_amd import _lib
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_DQN_KERNEL', form)
    lds = C.c_int32()
    _lib.check(_lib.lib().cobel_dqn_replay_query(D, 64, 64, A, 32, int(name == 'f64'), C.byref(lds)))
    assert (lds.value == staging_lds_bytes(D, name)) == (form == 'lds'), (form, lds.value)


def _t32_dqn_targets(torch, net, b, gamma, ddqn):
    """The regression targets of the replay step as this package's PyTorch path forms them, in
    float32 (a terminal sample does not look at the target network)."""
    with torch.no_grad():
        y = _t32_forward(torch, net['p'], b['states']).clone()
        boot = _t32_forward(torch, net['t'], b['next_states'])
        pick = (_t32_forward(torch, net['p'], b['next_states']) if ddqn else boot).argmax(dim=1)
        boot = torch.gather(boot, 1, pick[:, None])[:, 0]
        boot = torch.where(b['nonterminal'] != 0, boot, torch.zeros_like(boot))
        y.scatter_(1, b['actions'][:, None], (b['rewards'] + boot * b['nonterminal'] * gamma)[:, None])
    return y


class Replay:
    """The state of a mlp_common.dqn_case on the device, every tensor framed; ``run`` launches
    cobel_dqn_replay once and holds every instance against the reference."""

    def __init__(self, torch, case, name, form):
        self.torch, self.case, self.name, self.form = torch, case, name, form
        self.n, self.D, self.A = case['n'], case['D'], case['A']
        self.framed = {(kind, k): Framed(torch, case[stack][k].shape, _torch_dtype(torch, name))
                       for kind, stack in KINDS.items() for k in mc.KEYS}
        self.d_table = _dev(torch, case['table'])
        self.reset()

    def reset(self):
        """The case's own state again."""
        for (kind, k), f in self.framed.items():
            f.view.copy_(_dev(self.torch, self.case[KINDS[kind]][k]))
        self.steps = np.array(self.case['steps'], dtype=np.float64)

    def stack(self, kind):
        return {k: self.framed[kind, k].view for k in mc.KEYS}

    def nets(self, kind):
        """The networks as they are on the device, in float64."""
        host = {k: _host(self.framed[kind, k].view).astype(np.float64) for k in mc.KEYS}
        return [{k: host[k][j] for k in mc.KEYS} for j in range(self.n)]

    def redraw(self, seed, ddqn):
        """A new observation table and batch that keep the gap under the networks as they are on
        the device now."""
        mc.dqn_draw_batch(self.case, seed, ddqn, online=self.nets('p'), target=self.nets('t'))
        self.d_table = _dev(self.torch, self.case['table'])

    def batch(self, mode='gathered', ring_slots=0, spoil=()):
        """The case's batch on the device by the struct's field names: 'gathered', 'rings' of
        ``ring_slots`` rows (slots 0 and ring_slots - 1 both named; every row that no slot names
        NaN, its action 2^40) or 'index'.  Instances in ``spoil`` get NaN everywhere."""
        torch, c, n, dt = self.torch, self.case, self.n, _np(self.name)
        rows = [mc.dqn_rows(c, j, dt) for j in range(n)]
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
            if R >= mc.B:
                for j in range(n):
                    named = np.concatenate([[0, R - 1], 1 + rng.permutation(R - 2)[:mc.B - 2]])
                    slots[j] = rng.permutation(named)
                    assert len(set(slots[j])) == mc.B and {0, R - 1} <= set(slots[j].tolist())
            else:           # fewer rows than samples: the case has to repeat its samples accordingly
                slots[:] = np.arange(mc.B) % R
                for key in g:
                    for s in range(R, mc.B):
                        assert np.array_equal(g[key][:, s], g[key][:, s % R]), key
            rings = {}
            for key, a in g.items():
                fill = 2 ** 40 if key == 'actions' else np.nan
                rings[key] = np.full((n, R) + a.shape[2:], fill, dtype=a.dtype)
                for j in range(n):
                    rings[key][j, slots[j]] = a[j]
            g = dict(rings, batch_slots=slots)
        out = {key: _dev(torch, a) for key, a in g.items()}
        if mode == 'rings':
            out['ring_slots'] = ring_slots
        return out

    def run(self, batch, hyper=HYPER, gamma=GAMMA, ddqn=False, active=None, obs_index=None,
            gradient=False, where=None):
        """One launch.  Frames intact, step counts untouched, instances outside ``active`` keep
        every byte; every other instance against mlp_common.dqn_step from the state the launch
        started from (``gradient``: exp_avg / (1 - beta1) against the reference's gradient as
        well, which it is after one step from zero moments).  Returns the state after the launch
        (and 'q_out'), as host arrays."""
        from cobel_amd import _lib
        torch, c, n, D, A, name = self.torch, self.case, self.n, self.D, self.A, self.name
        before = {key: _host(f.view) for key, f in self.framed.items()}
        d_steps = _dev(torch, self.steps)
        d_active = None if active is None else _dev(torch, np.asarray(active, dtype=np.uint8))
        q = d_obs = None
        if obs_index is not None:
            q = Framed(torch, (n, A), _torch_dtype(torch, name))
            d_obs = _dev(torch, np.asarray(obs_index, dtype=np.int32))
        table = self.d_table if q is not None or 'state_index' in batch else None
        run = mc.fill_dqn_replay(_lib, self.stack('p'), self.stack('t'), self.stack('m'),
                                 self.stack('v'), d_steps, batch, n, D, A, hyper, gamma, ddqn,
                                 active=d_active, obs_index=d_obs, obs_table=table,
                                 q_out=None if q is None else q.view)
        _launch('cobel_dqn_replay', run)
        torch.cuda.synchronize()
        assert all(f.intact() for f in self.framed.values()) and (q is None or q.intact()), where
        assert np.array_equal(_host(d_steps), self.steps), where
        after = {key: _host(f.view) for key, f in self.framed.items()}
        if q is not None:
            after['q_out'] = _host(q.view)
        figure = (self.form, name, D, A)
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
            b = mc.dqn_rows(c, j)
            if j not in c['exempt']:
                gap = mc.dqn_gap(net['p'], net['t'], b['next_states'], ddqn)
                assert gap >= mc.GAP, (where, j, 'top-two gap %.3e' % gap)
            obs = None if q is None else c['table'][obs_index[j]].astype(_np(name))
            ref, g, q_ref = mc.dqn_step(net, b, hyper, gamma, ddqn, obs)
            t32 = g32 = q32 = None
            if name == 'f32':
                n32 = {kind: {k: torch.from_numpy(before[kind, k][j].copy()) for k in mc.KEYS}
                       for kind in KINDS}
                b32 = {key: torch.from_numpy(np.ascontiguousarray(a))
                       for key, a in mc.dqn_rows(c, j, np.float32).items()}
                y32 = _t32_dqn_targets(torch, n32, b32, gamma, ddqn)
                # (the optimizer counts the steps BEFORE this one)
                t32 = _t32_fit_step(torch, dict(n32, steps=net['steps'] - 1.0), b32['states'], y32,
                                    None, True, hyper)
                if gradient:
                    g32 = _t32_grads(torch, n32['p'], b32['states'], y32, None)
                if q is not None:
                    q32 = _t32_forward(torch, t32['p'], torch.from_numpy(obs)[None])[0]
            # float32 from ZERO second moments: the step divides by sqrt((1 - beta2) g^2) + eps, so
            # an element with |g| of the size of eps = 1e-8 turns a gradient error dg into up to
            # lr dg / eps = 3e5 dg of parameter, and which elements those are differs between any
            # two float32 implementations (docs/MEASUREMENTS.md sections 14 and 15).  Such an
            # instance is held link by link instead, under the same bound: its moments against the
            # reference (they ARE its gradient); its parameters against float64 Adam applied to the
            # moments the kernel itself wrote (the division, the bias corrections and the
            # write-back, without the amplification); its target network and q_out against blend()
            # and forward() of the parameters the kernel itself wrote.  torch's float32 is measured
            # the same way, each result against the float64 operation on torch's own inputs.
            steep = name == 'f32' and not any(before['v', k][j].any() for k in mc.KEYS)
            if steep:
                def f64(stack):
                    return {k: np.asarray(_host(a) if hasattr(a, 'detach') else a, dtype=np.float64)
                            for k, a in stack.items()}

                def links(p_old, t_old, m, v, p):
                    """float64 parameters from moments, target and q_out from parameters."""
                    out = {'p': mc.adam_from_moments(p_old, f64(m), f64(v), net['steps'], hyper['lr'],
                                                     hyper['beta1'], hyper['beta2'], hyper['eps'])}
                    out['t'] = mc.blend(t_old, f64(p), hyper['tau'])
                    out['q'] = None if q is None else mc.forward(f64(p), obs.astype(np.float64)[None])[2][0]
                    return out
                mine = {kind: {k: after[kind, k][j] for k in mc.KEYS} for kind in 'pmv'}
                own = links(net['p'], net['t'], mine['m'], mine['v'], mine['p'])
                own32 = links(net['p'], net['t'], t32['m'], t32['v'], t32['p'])
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
    """The case of mlp_common.dqn_gpu_cases by its key (the host tests draw every one of them)."""
    return mc.dqn_gpu_case(key, D, A, _np(name))


# ---------------------------------------------------------------------------------------------
@configs
@dtypes
def test_backward_pass_in_isolation(torch_cuda, monkeypatch, name, form, D, A):
    """One step from zero moments, steps = 1, no weight decay, DQN and DDQN: exp_avg / (1 - beta1)
    is the gradient the kernel formed — targets, pick, the loss gradient at the action taken, the
    six gradient products and the three bias sums, tensor by tensor against grads() without Adam's
    division in between; exp_avg_sq / (1 - beta2) its square."""
    pin(monkeypatch, form, name, D, A)
    hyper = dict(HYPER, tau=0.0)
    for ddqn in (False, True):
        case = _case(('backward', ddqn), D, A, name)
        rp = Replay(torch_cuda, case, name, form)
        rp.run(rp.batch(), hyper=hyper, ddqn=ddqn, gradient=True, where=ddqn)


@configs
@dtypes
def test_planted_batch_contents(torch_cuda, monkeypatch, name, form, D, A):
    """DDQN's first-maximum rule on exact ties (a wrong pick changes the target, so the gradient);
    terminal samples, whose targets are the rewards whatever the target network holds — NaN must
    not reach parameters, moments or q_out; repeated samples; a batch with one action only, whose
    other rows of w3 / b3 come back bit for bit with zero moments."""
    pin(monkeypatch, form, name, D, A)
    torch = torch_cuda
    case = _case('ties', D, A, name)
    rp = Replay(torch, case, name, form)
    rp.run(rp.batch(), ddqn=True, where='ties')
    for ddqn in (False, True):
        case = _case(('plain', ddqn), D, A, name)
        rp = Replay(torch, case, name, form)
        after = rp.run(rp.batch(), hyper=dict(HYPER, tau=0.0), ddqn=ddqn, obs_index=[3, 0, 12],
                       where=('plain', ddqn))
        taken = min(2, A - 1)
        for a in range(A):
            if a == taken:
                continue
            for kind, k in (('p', 'w3'), ('p', 'b3')):
                assert after[kind, k][0][a].tobytes() == case['P'][k][0][a].tobytes(), (ddqn, a, k)
            for kind in 'mv':
                assert not after[kind, 'w3'][0][a].any() and not after[kind, 'b3'][0][a].any()
        assert after['m', 'b3'][0][taken] != 0.0


@pytest.mark.parametrize('ring_slots', [1, 32, 33, 40])
@configs
@dtypes
def test_input_modes_agree(torch_cuda, monkeypatch, name, form, D, A, ring_slots):
    """The same case given gathered, through rings + batch_slots and as rows of the observation
    table (q_out asked for in all three): each against the reference, in float64 the three against
    each other; nothing non-finite comes out of the NaN that fills every ring row no slot names."""
    pin(monkeypatch, form, name, D, A)
    ddqn = mc.dqn_gpu_cases(D, A)['modes', ring_slots]['ddqn']
    case = _case(('modes', ring_slots), D, A, name)
    rp = Replay(torch_cuda, case, name, form)
    results = {}
    for mode in ('gathered', 'rings', 'index'):
        rp.reset()
        results[mode] = rp.run(rp.batch(mode, ring_slots), ddqn=ddqn, obs_index=[12, 0, 7, 7, 3],
                               where=mode)
    if name == 'f64':
        for mode in ('rings', 'index'):
            for key, a in results[mode].items():
                assert np.allclose(a, results['gathered'][key], rtol=1e-9, atol=1e-12), (mode, key)


@configs
@dtypes
def test_instances_that_sit_out(torch_cuda, monkeypatch, name, form, D, A):
    """active = 1 0 1 0 0 1 1, one instance only, NULL: an instance that sits out keeps every byte
    of its 24 tensors and its q_out row — with steps = 0 and NaN all over its batch — and the
    others match the reference."""
    pin(monkeypatch, form, name, D, A)
    n = 7
    case = _case('sit_out', D, A, name)
    rp = Replay(torch_cuda, case, name, form)
    for active in ([1, 0, 1, 0, 0, 1, 1], [0, 0, 0, 1, 0, 0, 0], None):
        rp.reset()
        idle = [j for j in range(n) if active is not None and not active[j]]
        rp.steps[idle] = 0.0
        rp.run(rp.batch('gathered', spoil=idle), active=active, obs_index=[0, 12, 1, 2, 3, 4, 5],
               where=active)


OPTIONS = mc.DQN_OPTIONS


@pytest.mark.parametrize('option', OPTIONS)
@configs
@dtypes
def test_options_over_three_steps(torch_cuda, monkeypatch, name, form, D, A, option):
    """Three consecutive steps on the state the kernel left in device memory, one option away from
    the base form (DQN, gamma 0.9, tau 0.07, no weight decay, step counts 1 2 5 1000 3): every step
    against the reference started from the state read back before it, on a table and batch drawn anew so that
    the top-two gap holds for that state (no sample skipped, no step dropped: a step whose search
    fails, fails the test).  The table and batch of steps 2 and 3 are searched against the networks
    read back from the kernel, so they are a function of the seed AND of the kernel's output: two
    float32 builds whose results differ in the last bits may end the search at different seeds and
    test different batches.  Each is held to the reference of its own batch, and the gap is asserted
    for it in run()."""
    pin(monkeypatch, form, name, D, A)
    hyper, gamma, ddqn = dict(HYPER), GAMMA, False
    if option == 'weight_decay':
        hyper['weight_decay'] = 1e-3
    elif option == 'tau0':
        hyper['tau'] = 0.0          # (run() holds the target network to its bytes)
    elif option == 'tau1':
        hyper['tau'] = 1.0
    elif option == 'steps':
        pass                        # (the case's step counts: at 1e6 both bias corrections round to 1)
    elif option == 'gamma0':
        gamma = 0.0
    elif option == 'ddqn':
        ddqn = True
    case = _case(('options', option), D, A, name)
    seed = case['seed']
    rp = Replay(torch_cuda, case, name, form)
    for it in range(3):
        if it:
            rp.redraw(seed + 100 * it, ddqn)
        rp.run(rp.batch(), hyper=hyper, gamma=gamma, ddqn=ddqn, where=(option, it))
        rp.steps += 1.0


@configs
@dtypes
def test_q_out_from_the_updated_parameters(torch_cuda, monkeypatch, name, form, D, A):
    """q_out of instance i is forward(UPDATED parameters, row obs_index[i]) — rows 0 and the last
    one among them — in both forms (float32 of the staging form: its split sums); and the step
    without q_out, obs_index and obs_table."""
    pin(monkeypatch, form, name, D, A)
    case = _case('q_out', D, A, name)
    rp = Replay(torch_cuda, case, name, form)
    last = mc.TABLE_ROWS - 1
    rp.run(rp.batch(), obs_index=[0, last, 5, last, 0], where='q_out')
    rp.reset()
    rp.run(rp.batch(), where='no q_out')


@pytest.mark.parametrize('D', LDS_D)
@dtypes
def test_the_two_forms_on_one_case(torch_cuda, monkeypatch, name, D):
    """Four actions are served by both forms: both meet the same bound against the reference on
    the same case (their summation orders differ by design: no claim between them)."""
    case = _case('two_forms', D, 4, name)
    for form in ('lds', 'stream'):
        pin(monkeypatch, form, name, D, 4)
        rp = Replay(torch_cuda, case, name, form)
        rp.run(rp.batch(), ddqn=True, obs_index=[1, 2, 3, 4, 12], where=form)
