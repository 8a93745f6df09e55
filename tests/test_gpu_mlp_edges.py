"""cobel_mlp_forward / cobel_mlp_fit (csrc/mlp_fit.hip) and cobel_dsr_targets
(csrc/dsr_targets.hip) at their edges, against the plain float64 reference of tests/mlp_common.py
(itself checked against torch autograd + torch.optim.Adam by tests/test_host_mlp_reference.py).

Shapes that straddle the 8-wide K quarters of layer 1, the 16-wide dW1 tile and the two output
tiles, in both dtypes (their accumulator row layouts differ); every workgroup group of the
forward kernel, with instances that sit a launch out; the backward pass in isolation (one step from
zero moments: exp_avg / (1 - beta1) IS the gradient the kernel formed); masks at the tile edges;
every option of the fit over three consecutive steps; the targets kernel with planted ties.

Parameters, inputs and targets are drawn in the kernel's dtype and handed to the reference
converted to float64.  Every output is a view into the middle of a larger buffer filled with a
sentinel; the frame must be intact after every launch.

Tolerances.  float64: gradients 1e-12 (max-norm relative per tensor), everything else rtol 1e-9 /
atol 1e-12.  float32: no number fixed in advance — the kernel's error against the float64 reference
(max-norm relative per tensor) must stay within 4x of the error torch's float32 on the CPU makes on
the same inputs, with 64 * 2^-24 (a 64-term sum) as the floor.  Measured figures: docs/MEASUREMENTS.md
section 14."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402

from mlp_gpu_common import (DEV, SENTINEL_U8, Framed, _dev, _host, _launch, _np,  # noqa: E402
                            _stack_dev, _stack_host, _t32_fit_step, _t32_forward, _t32_grads,
                            _torch_dtype, agree)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 17), (8, 16), (9, 15), (17, 31), (24, 2), (31, 32), (32, 1)]
RAGGED = [(9, 15), (17, 31)]
DTYPES = ['f64', 'f32']
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, tau=0.07)
FIGURES = {}               # (what, dtype, D, O) -> (kernel error, torch float32 error), the worst seen


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert DEV != 'cuda' or torch.cuda.is_available(), 'GPU tests need an MI355X'
    yield torch
    for key in sorted(FIGURES):
        print('mlp-edges figure %-12s %s D %2d O %2d  kernel %.2e  torch-f32 %.2e' % (key + FIGURES[key]))


def _agree(what, name, D, O, got, ref, t32=None, grad=False, where=None):
    """The kernel's ``got`` against the float64 ``ref``; float32: measured against torch's."""
    agree(FIGURES, (what, name, D, O), name, got, ref, t32, grad, where,
          after_adam=what.startswith('fit-'))


# ---------------------------------------------------------------------------------------------
# forward
class ForwardCase:
    """``nets`` networks and the 32 input rows of ``n`` instances: dense, or rows of a float64 table
    that ``in_div`` consecutive instances share."""

    def __init__(self, torch, seed, nets, n, D, O, name, in_div=1):
        self.torch, self.name, self.n, self.D, self.O = torch, name, n, D, O
        rng = np.random.default_rng(seed)
        dt = _np(name)
        self.P = mc.draw_networks(rng, nets, D, O, dt)
        self.in_div, rows = in_div, 13
        self.table = rng.standard_normal((rows, D))
        self.index = rng.integers(0, rows, size=(-(-n // in_div), mc.B)).astype(np.int32)
        self.X = np.stack([self.table[self.index[j // in_div]].astype(dt) for j in range(n)])
        self.dP = _stack_dev(torch, self.P)
        self.d_table, self.d_index, self.d_X = (_dev(torch, a) for a in (self.table, self.index, self.X))
        self.keep = []

    def launch(self, dense, net_div=1, act_div=1, active=None):
        from cobel_amd import _lib
        torch = self.torch
        out = Framed(torch, (self.n, mc.B, self.O), _torch_dtype(torch, self.name))
        d_active = None if active is None else _dev(torch, np.asarray(active, dtype=np.uint8))
        kw = dict(in_dense=self.d_X) if dense else \
            dict(in_table=self.d_table, in_index=self.d_index, in_div=self.in_div)
        run = mc.fill_forward(_lib, self.dP, out.view, self.n, self.D, self.O, net_div=net_div,
                              act_div=act_div, active=d_active, **kw)
        _launch('cobel_mlp_forward', run)
        assert out.intact()
        return out

    def check(self, what, out, net_div=1, act_div=1, active=None):
        torch = self.torch
        got = _host(out.view)
        for j in range(self.n):
            if active is not None and not active[j // act_div]:
                assert out.untouched(j), (what, j)
                continue
            p = mc.one(self.P, j // net_div)
            ref = mc.forward(p, self.X[j].astype(np.float64))[2]
            t32 = None
            if self.name == 'f32':
                p32 = {k: torch.from_numpy(self.P[k][j // net_div]) for k in mc.KEYS}
                t32 = _t32_forward(torch, p32, torch.from_numpy(self.X[j]))
            _agree(what, self.name, self.D, self.O, got[j], ref, t32, where=j)


@pytest.mark.parametrize('D,O', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_forward_input_forms(torch_cuda, name, D, O):
    """n = 7 instances with a network each: a dense block, and rows of a table by an index array of
    ceil(n / in_div) rows for in_div 1 and 3; the three agree with the reference, and dense and
    table rows (the same numbers) bit for bit with each other."""
    for in_div in (1, 3):
        case = ForwardCase(torch_cuda, 1000 * D + 10 * O + in_div, 7, 7, D, O, name, in_div)
        out = case.launch(dense=False)
        case.check('forward', out)
        dense = case.launch(dense=True)
        assert torch_cuda.equal(out.view, dense.view)


GROUPS = [(2, 10, 2), (3, 6, 3), (4, 6, 2), (5, 5, 1), (4, 8, 4)]     # net_div, n, the group it takes


@pytest.mark.parametrize('D,O', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_forward_groups(torch_cuda, name, D, O):
    """Instances that share a network go to one workgroup, 4, 3, 2 or 1 of them: every instance
    against the reference on network j // net_div (table rows shared by two instances, so the
    index row changes inside a group)."""
    for net_div, n, group in GROUPS:
        assert group == next(g for g in (4, 3, 2, 1) if net_div % g == 0 and n % g == 0)
        case = ForwardCase(torch_cuda, 77 * D + O + net_div, -(-n // net_div), n, D, O, name, in_div=2)
        out = case.launch(dense=(net_div == 3), net_div=net_div)
        case.check('forward-grp', out, net_div=net_div)


@pytest.mark.parametrize('D,O', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_forward_instances_that_sit_out(torch_cuda, name, D, O):
    """Groups of four in which some instances sit the launch out (``skip``, then ``continue`` past
    the trailing barrier): the running ones are right, the others keep their sentinel."""
    case = ForwardCase(torch_cuda, 31 * D + O, 4, 16, D, O, name, in_div=1)
    active = [1, 0, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0]
    out = case.launch(dense=False, net_div=4, active=active)
    case.check('forward-act', out, net_div=4, active=active)
    pairs = [1, 0, 0, 1, 0, 0, 1, 1]                       # act_div = 2: [1100] [0011] [0000] [1111]
    out = case.launch(dense=True, net_div=4, act_div=2, active=pairs)
    case.check('forward-act', out, net_div=4, act_div=2, active=pairs)
    # groups of two (net_div 2) whose flags change inside and between groups (act_div 3)
    case = ForwardCase(torch_cuda, 31 * D + O + 1, 5, 10, D, O, name, in_div=3)
    triples = [1, 0, 1, 0]
    out = case.launch(dense=False, net_div=2, act_div=3, active=triples)
    case.check('forward-act', out, net_div=2, act_div=3, active=triples)


# ---------------------------------------------------------------------------------------------
# fit
class FitCase:
    """n networks with optimizer state and target networks on the device, the float64 reference
    and (float32) torch's float32 replica of each; ``step`` launches cobel_mlp_fit once and moves
    the replicas along, ``compare`` holds them against each other."""

    def __init__(self, torch, seed, n, D, O, name, hyper, steps=None, zero_moments=(), zero_first=(),
                 target=True, table=True, in_div=1, tgt_div=1):
        self.torch, self.name, self.n, self.D, self.O = torch, name, n, D, O
        self.hyper, self.in_div, self.tgt_div, self.has_table = dict(hyper), in_div, tgt_div, table
        rng = self.rng = np.random.default_rng(seed)
        dt = _np(name)
        self.P = mc.draw_networks(rng, n, D, O, dt)
        self.T = mc.draw_networks(rng, n, D, O, dt) if target else None
        # optimizer state as it is in the middle of a run: moments of the size of the gradients
        # (zero_moments: networks that start from nothing, or all of them with True; zero_first:
        #  networks whose first moment alone is zero)
        self.M = {k: (0.01 * rng.standard_normal(a.shape)).astype(dt) for k, a in self.P.items()}
        self.V = {k: (1e-4 * rng.uniform(0.05, 1.0, a.shape)).astype(dt) for k, a in self.P.items()}
        for j in (range(n) if zero_moments is True else zero_moments):
            for k in mc.KEYS:
                self.M[k][j], self.V[k][j] = 0.0, 0.0
        for j in zero_first:
            for k in mc.KEYS:
                self.M[k][j] = 0.0
        self.steps = np.zeros(n) if steps is None else np.asarray(steps, dtype=np.float64)
        rows = 13
        self.table = rng.standard_normal((rows, D))
        self.index = rng.integers(0, rows, size=(-(-n // in_div), mc.B)).astype(np.int32)
        if table:
            self.X = np.stack([self.table[self.index[j // in_div]].astype(dt) for j in range(n)])
        else:
            self.X = rng.standard_normal((n, mc.B, D)).astype(dt)
        self.Y = rng.standard_normal((-(-n // tgt_div), mc.B, O)).astype(dt)
        self.dP, self.dM, self.dV = (_stack_dev(torch, s) for s in (self.P, self.M, self.V))
        self.dT = _stack_dev(torch, self.T) if target else None
        self.d_steps = _dev(torch, self.steps)
        self.d_table, self.d_index, self.d_X, self.d_Y = (
            _dev(torch, a) for a in (self.table, self.index, self.X, self.Y))
        self.ref = [{'p': mc.one(self.P, j), 'm': mc.one(self.M, j), 'v': mc.one(self.V, j),
                     't': mc.one(self.T, j) if target else None, 'steps': float(self.steps[j])}
                    for j in range(n)]
        self.t32 = None
        if name == 'f32':
            def t(stack, j):
                return {k: torch.from_numpy(stack[k][j].copy()) for k in mc.KEYS}
            self.t32 = [{'p': t(self.P, j), 'm': t(self.M, j), 'v': t(self.V, j),
                         't': t(self.T, j) if target else None, 'steps': float(self.steps[j])}
                        for j in range(n)]

    def _state(self):
        stacks = [('p', self.dP), ('m', self.dM), ('v', self.dV)] + ([('t', self.dT)] if self.dT else [])
        return {(kind, k): s[k] for kind, s in stacks for k in mc.KEYS}

    def step(self, mask=None, train=None, active=None, act_div=1, ep=None, ep_rows=0, ep_div=1,
             ep_out=True):
        """``mask`` [n, 32], ``train`` [n], ``active`` [ceil(n / act_div)] (None: NULL pointers);
        ``ep``: None, 'dense' or 'table'.  Returns the framed ep_out (or None)."""
        from cobel_amd import _lib
        torch, n, dt = self.torch, self.n, _np(self.name)
        before = {key: a.clone() for key, a in self._state().items()}
        steps_before = self.d_steps.clone()
        as_u8 = lambda a: None if a is None else _dev(torch, np.asarray(a, dtype=np.uint8))  # noqa: E731
        d_mask, d_train, d_active = as_u8(mask), as_u8(train), as_u8(active)
        kw, framed = {}, None
        ep_x = None
        if ep == 'dense':
            ep_x = self.rng.standard_normal((n, max(ep_rows, 1), self.D)).astype(dt)
            kw['ep_dense'] = d_ep = _dev(torch, ep_x)                                  # noqa: F841
        elif ep == 'table':
            ep_index = self.rng.integers(0, self.table.shape[0], size=-(-n // ep_div)).astype(np.int32)
            ep_x = np.stack([self.table[ep_index[j // ep_div]].astype(dt)[None] for j in range(n)])
            kw['ep_table'], kw['ep_index'] = self.d_table, _dev(torch, ep_index)
        if ep_out:
            framed = Framed(torch, (n, max(ep_rows, 1), self.O), _torch_dtype(torch, self.name))
            kw['ep_out'] = framed.view
        kw.update(dict(in_table=self.d_table, in_index=self.d_index, in_div=self.in_div)
                  if self.has_table else dict(in_dense=self.d_X))
        run = mc.fill_fit(_lib, self.dP, self.dM, self.dV, self.d_steps, self.d_Y, n, self.D, self.O,
                          self.hyper, target_params=self.dT, train=d_train, active=d_active,
                          act_div=act_div, tgt_div=self.tgt_div, sample_mask=d_mask, ep_div=ep_div,
                          ep_rows=ep_rows, **kw)
        _launch('cobel_mlp_fit', run)
        self.idle, self.running = [], []
        for j in range(n):
            if active is not None and not active[j // act_div]:
                self.idle.append(j)
                continue
            self.running.append(j)
            tr = True if train is None else bool(train[j])
            mk = None if mask is None else np.asarray(mask[j], dtype=np.uint8)
            x, y = self.X[j], self.Y[j // self.tgt_div]
            self.ref[j] = mc.fit_step(self.ref[j], x.astype(np.float64), y.astype(np.float64), mk, tr,
                                      self.hyper)
            if self.t32:
                self.t32[j] = _t32_fit_step(torch, self.t32[j], torch.from_numpy(x),
                                            torch.from_numpy(y), mk, tr, self.hyper)
            if not tr:        # no optimiser step: parameters, moments and step count bit for bit
                for (kind, k), a in self._state().items():
                    assert kind == 't' or torch.equal(a[j], before[(kind, k)][j]), (j, kind, k)
                assert float(self.d_steps[j]) == float(steps_before[j])
        for j in self.idle:   # nothing at all
            for key, a in self._state().items():
                assert torch.equal(a[j], before[key][j]), (j, key)
            assert float(self.d_steps[j]) == float(steps_before[j])
            assert framed is None or framed.untouched(j)
        if framed is not None:
            assert framed.intact()
            if ep is None or ep_rows == 0:
                assert all(framed.untouched(j) for j in range(n))
            else:
                got = _host(framed.view)
                for j in self.running:      # (also the networks that did not train)
                    ref = mc.forward(self.ref[j]['p'], ep_x[j].astype(np.float64))[2]
                    t32 = _t32_forward(torch, self.t32[j]['p'], torch.from_numpy(ep_x[j])) \
                        if self.t32 else None
                    _agree('fit-ep_out', self.name, self.D, self.O, got[j], ref, t32, where=j)
        return framed

    def compare(self, where=None, kinds=('p', 'm', 'v', 't')):
        state = {key: _host(a) for key, a in self._state().items()}
        assert np.array_equal(_host(self.d_steps), [r['steps'] for r in self.ref]), where
        for j in range(self.n):
            for (kind, k), a in state.items():
                if kind in kinds:
                    _agree('fit-' + kind, self.name, self.D, self.O, a[j], self.ref[j][kind][k],
                           self.t32[j][kind][k] if self.t32 else None, where=(where, j, kind, k))


@pytest.mark.parametrize('D,O', SHAPES)
@pytest.mark.parametrize('name', DTYPES)
def test_fit_backward_pass_in_isolation(torch_cuda, name, D, O):
    """One step from zero moments, steps = 0, no weight decay: exp_avg / (1 - beta1) is the
    gradient the kernel formed — the six gradient products and the three bias sums, tensor by
    tensor against grads(), without Adam's division in between; exp_avg_sq / (1 - beta2) its
    square.  Once with all samples (sample_mask NULL), once with masks."""
    torch = torch_cuda
    hyper = dict(HYPER, tau=0.0)
    c1, c2 = 1.0 - hyper['beta1'], 1.0 - hyper['beta2']
    if name == 'f32':     # the constants as the kernel holds them
        c1, c2 = float(np.float32(c1)), float(np.float32(c2))
    n = 4
    for masked in (False, True):
        case = FitCase(torch, 13 * D + O + masked, n, D, O, name, hyper, zero_moments=True,
                       target=False, table=masked, in_div=3 if masked else 1)
        mask = None
        if masked:
            mask = (case.rng.random((n, mc.B)) < 0.4).astype(np.uint8)
            mask[1], mask[2] = 0, 0
            mask[1, 16] = 1                    # a single sample
            mask[2, 10:21] = 1                 # across the two row tiles
        case.step(mask=mask)
        assert np.array_equal(_host(case.d_steps), np.ones(n))
        m, v = _stack_host(case.dM), _stack_host(case.dV)
        for j in range(n):
            mk = None if mask is None else mask[j]
            g = mc.grads(mc.one(case.P, j), case.X[j].astype(np.float64),
                         case.Y[j].astype(np.float64), mk)
            g32 = None
            if name == 'f32':
                g32 = _t32_grads(torch, {k: torch.from_numpy(case.P[k][j]) for k in mc.KEYS},
                                 torch.from_numpy(case.X[j]), torch.from_numpy(case.Y[j]), mk)
            for k in mc.KEYS:
                _agree('grad-' + k, name, D, O, m[k][j].astype(np.float64) / c1, g[k],
                       g32[k] if g32 else None, grad=True, where=(masked, j, k))
                _agree('gradsq', name, D, O, v[k][j].astype(np.float64) / c2, g[k] * g[k],
                       g32[k] * g32[k] if g32 else None, grad=True, where=(masked, j, k))


@pytest.mark.parametrize('D,O', RAGGED)
@pytest.mark.parametrize('name', DTYPES)
def test_fit_masks_at_the_tile_edges(torch_cuda, name, D, O):
    """One network per mask: exactly one sample at row 0, 15, 16, 31; rows 0 .. 15 only; rows
    16 .. 31 only; all rows; none marked with train = 1 (the count clamps to 1: an Adam step on a
    zero gradient from non-zero moments, and the step count increments); none marked with
    train = 0 (blend only, step count unchanged); and one sample at row 6 and at row 27, which the
    two accumulator layouts (4 v + lane / 16, 4 (lane / 16) + v) keep in different registers.  The
    networks with samples start from a zero first moment, so their exp_avg is the gradient alone."""
    n = 11
    mask = np.zeros((n, mc.B), dtype=np.uint8)
    for j, s in enumerate((0, 15, 16, 31)):
        mask[j, s] = 1
    mask[4, :16], mask[5, 16:], mask[6, :] = 1, 1, 1
    # (rows 0, 15, 16 and 31 sit at the same place in both accumulator layouts: two that do not)
    mask[9, 6], mask[10, 27] = 1, 1
    train = np.array([1] * 8 + [0, 1, 1], dtype=np.uint8)
    case = FitCase(torch_cuda, 5 * D + O, n, D, O, name, HYPER, steps=[3.0] * n,
                   zero_first=(0, 1, 2, 3, 4, 5, 6, 9, 10))
    case.step(mask=mask, train=train)
    case.compare()
    assert _host(case.d_steps).tolist() == [4.0] * 8 + [3.0, 4.0, 4.0]
    # the zero gradient moved the parameters of network 7 (its moments were not zero)
    assert not np.array_equal(_host(case.dP['w2'][7]), case.P['w2'][7])


def _masks(rng, n):
    """Random masks; network 1 without samples (train = 0: blend only), network 2 one sample."""
    mask = (rng.random((n, mc.B)) < 0.4).astype(np.uint8)
    mask[1] = 0
    mask[2] = 0
    mask[2, int(rng.integers(0, mc.B))] = 1
    return mask, mask.any(axis=1).astype(np.uint8)


OPTIONS = ['train_null', 'act_div2', 'tgt_div1', 'tgt_div3', 'tau0', 'weight_decay', 'step_counts',
           'ep_dense2', 'ep_dense3', 'ep_dense4', 'ep_table_div3', 'ep_out_null', 'ep_rows0',
           'dense_inputs']


@pytest.mark.parametrize('option', OPTIONS)
@pytest.mark.parametrize('D,O', RAGGED)
@pytest.mark.parametrize('name', DTYPES)
def test_fit_options_over_three_steps(torch_cuda, name, D, O, option):
    """n = 7 networks, three consecutive steps, one option away from the base form (inputs by
    table rows shared by three networks, masks with train derived from them, tau 0.07): parameters,
    both moments, target networks and step counts after every step; ep_out is the forward pass of
    the UPDATED parameters, also for networks that did not train; networks excluded by ``active``
    keep every byte."""
    n = 7
    hyper, kw, step_kw = dict(HYPER), dict(in_div=3, tgt_div=2), {}
    if option == 'tgt_div1':
        kw['tgt_div'] = 1
    elif option == 'tgt_div3':
        kw['tgt_div'] = 3
    elif option == 'tau0':
        hyper['tau'], kw['target'] = 0.0, False          # NULL target pointers
    elif option == 'weight_decay':
        hyper['weight_decay'] = 1e-3
    elif option == 'step_counts':
        kw['steps'], kw['zero_moments'] = [0, 1, 5, 1000, 2, 0, 17], (0, 5)
    elif option.startswith('ep_dense'):
        step_kw = dict(ep='dense', ep_rows=int(option[-1]))
    elif option == 'ep_table_div3':
        step_kw = dict(ep='table', ep_rows=1, ep_div=3)
    elif option == 'ep_out_null':
        step_kw = dict(ep='dense', ep_rows=2, ep_out=False)
    elif option == 'ep_rows0':
        step_kw = dict(ep='dense', ep_rows=0)
    elif option == 'dense_inputs':
        kw['table'] = False
    seed = 1000 * OPTIONS.index(option) + 10 * D + O
    case = FitCase(torch_cuda, seed, n, D, O, name, hyper, **kw)
    for it in range(3):
        mask, train = _masks(case.rng, n)
        if option == 'train_null':
            train = None                                 # (network 1: nothing marked, trains anyway)
        if option == 'act_div2':
            step_kw = dict(active=[[1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1]][it], act_div=2)
        case.step(mask=mask, train=train, **step_kw)
        case.compare(where=it)
        if option == 'act_div2':
            assert case.idle == [[2, 3], [0, 1, 6], [4, 5]][it]


# ---------------------------------------------------------------------------------------------
# the regression targets
# use_dr, follow_up, ignore_terminality (with use_dr the argmax is not looked at: the follow-up and
# terminality switches also run without it, so that the ties count under them too)
SWITCHES = {'off': (0, 0, 0), 'on': (1, 1, 1), 'dr': (1, 0, 0), 'follow': (0, 1, 0), 'ignore': (0, 0, 1)}


@pytest.mark.parametrize('switches', sorted(SWITCHES))
@pytest.mark.parametrize('name', DTYPES)
def test_dsr_targets_with_planted_ties(torch_cuda, name, switches):
    """A in (1, 3, 4, 5, 8) (odd A leaves half a wave outside the took / train ballot), O in
    (1, 7, 32, 33), n = 5: took and train exact, targets bit for bit the reference evaluated in the
    kernel's dtype in the same operation order, and within (A + 4) roundings of the float64 one.
    The values hold ties (all equal; maximum first, last, twice: the first wins), nonterminal 0, 1
    and 0.5, an action one sample alone took, an agent whose samples all took one action."""
    from cobel_amd import _lib
    torch = torch_cuda
    use_dr, follow_up, ignore = SWITCHES[switches]
    n, gamma, dt = 5, 0.9, _np(name)
    eps = 2.0 ** -53 if name == 'f64' else 2.0 ** -24
    for A in (1, 3, 4, 5, 8):
        for O in (1, 7, 32, 33):
            c = mc.dsr_case(100 * A + O, n, A, O, dt)
            t = {k: _dev(torch, a) for k, a in c.items()}
            targets = Framed(torch, (n, mc.B, O), _torch_dtype(torch, name))
            took = Framed(torch, (n * A, mc.B), torch.uint8, SENTINEL_U8)
            train = Framed(torch, (n * A,), torch.uint8, SENTINEL_U8)
            t.update(targets=targets.view, took=took.view, train=train.view)
            _launch('cobel_dsr_targets', mc.fill_dsr(_lib, t, n, A, O, name == 'f64', gamma, use_dr,
                                                     follow_up, ignore))
            assert targets.intact() and took.intact() and train.intact(), (A, O)
            same, ref_took, ref_train = mc.dsr_targets(
                gamma=gamma, use_dr=use_dr, follow_up=follow_up, ignore_terminality=ignore, dtype=dt, **c)
            exact = mc.dsr_targets(gamma=gamma, use_dr=use_dr, follow_up=follow_up,
                                   ignore_terminality=ignore, dtype=np.float64, **c)[0]
            assert np.array_equal(_host(took.view), ref_took), (A, O)
            assert np.array_equal(_host(train.view), ref_train), (A, O)
            got = _host(targets.view)
            assert got.dtype == same.dtype and np.array_equal(got, same), \
                (A, O, float(np.abs(got - same).max()))
            bound = (A + 4) * eps * mc.dsr_magnitude(c['successor'], c['value'], c['table'],
                                                     c['state_index'], c['next_index'], gamma, follow_up)
            assert (np.abs(got.astype(np.float64) - exact) <= bound).all(), (A, O)
