"""cobel_adam_step (csrc/adam.hip, k_adam) at its edges, against mlp_common.adam_kernel — the
kernel's operations in the kernel's order and dtype, one rounding each, in NumPy — and against
the float64 Adam of the same file (mlp_common.adam, checked against torch.optim.Adam by
tests/test_host_mlp_reference.py).

What is compared, and how closely (measured figures: docs/MEASUREMENTS.md section 17).

exp_avg and exp_avg_sq, both dtypes: bit for bit.  The library builds with -ffp-contract=off and
no pow is involved, so every operand order and every cast of 1 - beta1, beta2, weight_decay shows.
Instances outside `active` keep every bit of their four or five tensors, NaN gradients or not.

param and target.  They depend on 1 - beta1^t and sqrt(1 - beta2^t), which the kernel forms from
the device's float64 pow and the restatement from the host's.  The HIP math API documents its
double-precision pow as accurate to 1 ulp, the host's libm stays below 1 ulp: the two values of
beta^t are at most POW_ULPS = 2 float64 neighbours apart.
  - An instance must equal the restatement bit for bit for SOME pair of beta1^t, beta2^t within
    that distance of the host's (pow_ulps of adam_kernel): at once wherever the two pows round
    alike, which includes t = 1 (beta^1 is beta) and every t from which beta^t no longer changes
    1 - beta^t.
  - Whatever pair it is, the distance to the restatement with the host's pow is bounded.  An
    error of POW_ULPS * 2^-52 relative in beta^t is at most POW_ULPS * 2^-52 / (1 - beta^t)
    relative in 1 - beta^t (the cancellation), all of that in step_size = lr / (1 - beta1^t) and
    half of it in sqrt(1 - beta2^t), so relative in the step s = step_size * (m / denom)
        rho = POW_ULPS * 2^-52 * (1 / (1 - beta1^t) + 0.5 / (1 - beta2^t)),
    i.e. rho / unit ulps of it (unit = 2^-53 or 2^-24); both casts of the corrections and the four
    operations behind them may each end one neighbour further: 8 ulps more.  The step is read off
    as param_new - param_old, which can lie in the binade below the product's: twice the count.
        |param - restated| <= 2 (rho / unit + 8) ulp(step) + ulp(param)
        |target - restated| <= the same + ulp(param - target_old) + 2 ulp(target)     (|tau| <= 1)
    and never more than the project's tolerances so far: rtol 1e-12 / atol 1e-14 in float64,
    rtol 2e-5 / atol 1e-7 in float32.

The meaning of the update, float32: the kernel against float64 Adam evaluated on the kernel's own
float32 inputs, link by link as in tests/test_gpu_dqn_replay_edges.py, the bound counting the
float32 roundings of each link (u = 2^-24):
  - moments: exp_avg takes at most 7 roundings of terms no larger than |m| + |g| + |wd p|,
    exp_avg_sq at most 10 of |v| + (1 - beta2) g^2 (g squared doubles its error): 8 u and 12 u of
    those, and 4 * 2^-149 absolute where the square of a gradient underflows;
  - parameters from the kernel's OWN moments: the casts of lr, both corrections and eps, three
    divisions, the square root, the sum and the product are 10 roundings of the step, the
    subtraction one of the parameter: 12 u |step| + u |param|;
  - target from the kernel's OWN parameters: 4 u |tau| (|param| + |target|) + u |target|.

Not covered: the grid.y cap of 65 535 chunks needs more than 67 million elements per instance,
out of reach of a test of a few seconds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_common as mc  # noqa: E402
from mlp_gpu_common import Framed, PAD, _dev, _host, _np, _torch_dtype  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ['f64', 'f32']
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, tau=0.05)
STEPS = np.array([1.0, 2.0, 10.0, 1000.0, 1e6])
POW_ULPS = 2
TOL = {'f64': (1e-12, 1e-14), 'f32': (2e-5, 1e-7)}
U32, TINY32 = 2.0 ** -24, 2.0 ** -149
E_ARG, E_RANGE = -1, -2
FIGURES = {}          # (what, dtype) -> [largest deviation / bound, largest deviation in ulps, bound in ulps there]
COUNTS = {}           # dtype -> [instances compared, instances whose pow differs from the host's]

dtypes = pytest.mark.parametrize('name', DTYPES)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    yield torch
    for key in sorted(FIGURES):
        print('adam-edges figure %-12s %s  deviation/bound %.3e  (%.4g ulps, bound %.4g ulps)'
              % (key + tuple(FIGURES[key])))
    for name in sorted(COUNTS):
        print('adam-edges pow %s: %d instances, %d with another beta^t than the host'
              % ((name,) + tuple(COUNTS[name])))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _note(what, name, dev, bound, unit):
    """Holds ``dev <= bound`` elementwise and keeps the worst ratio (``unit``: one ulp there)."""
    ratio = np.where(dev == 0.0, 0.0, dev / np.maximum(bound, np.finfo(np.float64).tiny))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    if (what, name) not in FIGURES or ratio[at] > FIGURES[what, name][0]:
        FIGURES[what, name] = [float(ratio[at]), float(dev[at] / unit[at]), float(bound[at] / unit[at])]
    assert (dev <= bound).all(), (what, name, float(ratio[at]), float(dev[at]), float(bound[at]))


def draw(seed, n, per, name, moments=True):
    """Parameters, gradients over six decades, mid-run moments (or none) and a target."""
    rng, dt = np.random.default_rng(seed), _np(name)
    p = rng.uniform(-1.0, 1.0, (n, per)).astype(dt)
    g = (rng.standard_normal((n, per)) * 10.0 ** rng.integers(-6, 1, size=(n, per))).astype(dt)
    m = ((0.01 if moments else 0.0) * rng.standard_normal((n, per))).astype(dt)
    v = ((1e-4 if moments else 0.0) * rng.uniform(0.05, 1.0, (n, per))).astype(dt)
    t = rng.uniform(-1.0, 1.0, (n, per)).astype(dt)
    return {'p': p, 'g': g, 'm': m, 'v': v, 't': t}


def launch(torch, name, x, steps, hyper, active=None, target=True, n=None, per=None, nulls=()):
    """One cobel_adam_step on framed copies of x: (return code, tensors afterwards, frames)."""
    from cobel_amd import _lib
    dt = _torch_dtype(torch, name)
    fr = {k: Framed(torch, a.shape, dt) for k, a in x.items()}
    for k, a in x.items():
        fr[k].view.copy_(_dev(torch, a))
    fr['steps'] = Framed(torch, steps.shape, torch.float64)
    fr['steps'].view.copy_(_dev(torch, steps))
    if active is not None:
        fr['active'] = Framed(torch, active.shape, torch.uint8, fill=0x5A)
        fr['active'].view.copy_(_dev(torch, active))

    def ptr(k):
        f = fr.get(k)
        return None if f is None or k in nulls else f.buf.data_ptr() + PAD * f.buf.element_size()
    rc = _lib.lib().cobel_adam_step(
        ptr('p'), ptr('g'), ptr('m'), ptr('v'), ptr('steps'), ptr('active'),
        x['p'].shape[0] if n is None else n, x['p'].shape[1] if per is None else per,
        int(name == 'f64'), hyper['lr'], hyper['beta1'], hyper['beta2'], hyper['eps'],
        hyper['weight_decay'], ptr('t') if target else None, hyper['tau'], None)
    torch.cuda.synchronize()
    return rc, {k: _host(f.view) for k, f in fr.items()}, fr


def check(torch, name, x, steps, hyper=HYPER, active=None, target=True, where=None):
    """One launch held against the restatement and, in float32, against float64 Adam."""
    dt, unit = _np(name), 2.0 ** -53 if name == 'f64' else U32
    steps = np.asarray(steps, dtype=np.float64)
    rc, got, fr = launch(torch, name, x, steps, hyper, active, target)
    assert rc == 0, where
    assert all(f.intact() for f in fr.values()), where
    assert _same_bits(got['g'], x['g']) and np.array_equal(got['steps'], steps), where
    assert active is None or np.array_equal(got['active'], active), where
    on = np.ones(len(steps), dtype=bool) if active is None else active != 0
    for k in 'pmvt':                                    # an instance that sits out keeps every bit
        assert _same_bits(got[k][~on], x[k][~on]), (where, k)
    if not target:
        assert _same_bits(got['t'], x['t']), where
    if not on.any():
        return got
    sel = {k: a[on] for k, a in x.items()}
    st = steps[on]
    have = {k: got[k][on] for k in 'pmvt'}
    old_t = sel['t'] if target else None
    with np.errstate(all='ignore'):
        ref = dict(zip('pmvt', mc.adam_kernel(sel['p'], sel['g'], sel['m'], sel['v'], st, hyper, dt,
                                              target=old_t)))
    # --- moments: bit for bit
    assert _same_bits(have['m'], ref['m']), (where, 'exp_avg')
    assert _same_bits(have['v'], ref['v']), (where, 'exp_avg_sq')
    # --- param and target: bit for bit for some beta^t within POW_ULPS of the host's ...
    kinds = 'pt' if target else 'p'
    differs = np.zeros(len(st), dtype=bool)
    for k in kinds:
        differs |= (_bits(have[k]) != _bits(ref[k])).any(axis=1)
    odd = np.flatnonzero(differs)
    tally = COUNTS.setdefault(name, [0, 0])
    tally[0] += len(st)
    tally[1] += len(odd)
    left = set(odd.tolist())
    for d1 in range(-POW_ULPS, POW_ULPS + 1):
        for d2 in range(-POW_ULPS, POW_ULPS + 1):
            if not left or (d1 == 0 and d2 == 0):
                continue
            j = np.array(sorted(left))
            with np.errstate(all='ignore'):
                alt = dict(zip('pmvt', mc.adam_kernel(
                    sel['p'][j], sel['g'][j], sel['m'][j], sel['v'][j], st[j], hyper, dt,
                    target=None if old_t is None else old_t[j], pow_ulps=(d1, d2))))
            explained = np.ones(len(j), dtype=bool)
            for k in kinds:
                explained &= (_bits(have[k][j]) == _bits(alt[k])).all(axis=1)
            left -= set(j[explained].tolist())
    assert not left, (where, 'no beta^t within %d ulps explains instances' % POW_ULPS, sorted(left)[:5],
                      st[sorted(left)[:5]])
    # ... and within the bound of the module's docstring whichever it is
    f = {k: a.astype(np.float64) for k, a in ref.items() if a is not None}
    rho = POW_ULPS * 2.0 ** -52 * (1.0 / (1.0 - hyper['beta1'] ** st) +
                                   0.5 / (1.0 - hyper['beta2'] ** st))
    count = 2.0 * (rho / unit + 8.0)[:, None]
    ulp = lambda a: np.spacing(np.abs(a).astype(dt)).astype(np.float64)   # noqa: E731
    rtol, atol = TOL[name]
    bound_p = count * ulp(f['p'] - sel['p'].astype(np.float64)) + ulp(f['p'])
    dev = np.abs(have['p'].astype(np.float64) - f['p'])
    _note('param', name, dev, np.minimum(bound_p, rtol * np.abs(f['p']) + atol), ulp(f['p']))
    if target:
        bound_t = bound_p + ulp(f['p'] - old_t.astype(np.float64)) + 2.0 * ulp(f['t'])
        dev = np.abs(have['t'].astype(np.float64) - f['t'])
        _note('target', name, dev, np.minimum(bound_t, rtol * np.abs(f['t']) + atol), ulp(f['t']))
    if name == 'f32':
        meaning(sel, have, st, hyper, old_t)
    return got


def meaning(x, have, steps, hyper, old_t):
    """The float32 kernel against float64 Adam on the kernel's own float32 inputs, link by link."""
    x64 = {k: a.astype(np.float64) for k, a in x.items()}
    k64 = {k: a.astype(np.float64) for k, a in have.items()}
    lr, b1, b2, eps, wd, tau = (hyper[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'tau'))
    t = steps[:, None]
    one = lambda a: {'x': a}          # noqa: E731
    _, m64, v64 = (d['x'] for d in mc.adam(one(x64['p']), one(x64['m']), one(x64['v']),
                                              one(x64['g']), t, lr, b1, b2, eps, wd))
    ge = np.abs(x64['g']) + np.abs(wd * x64['p'])
    unit_m, unit_v = U32 * np.maximum(np.abs(m64), TINY32 / U32), U32 * np.maximum(v64, TINY32 / U32)
    _note('mean-m', 'f32', np.abs(k64['m'] - m64), 8 * U32 * (np.abs(x64['m']) + ge) + 4 * TINY32, unit_m)
    _note('mean-v', 'f32', np.abs(k64['v'] - v64),
          12 * U32 * (x64['v'] + (1.0 - b2) * ge * ge) + 4 * TINY32, unit_v)
    own = mc.adam_from_moments(one(x64['p']), one(k64['m']), one(k64['v']), t, lr, b1, b2, eps)['x']
    unit_p = U32 * np.abs(own)
    _note('mean-p-own', 'f32', np.abs(k64['p'] - own),
          12 * U32 * np.abs(own - x64['p']) + U32 * np.abs(own) + TINY32, np.maximum(unit_p, TINY32))
    if old_t is not None:
        t_old = old_t.astype(np.float64)
        own_t = mc.blend(one(t_old), one(k64['p']), tau)['x']
        _note('mean-t-own', 'f32', np.abs(k64['t'] - own_t),
              4 * U32 * abs(tau) * (np.abs(k64['p']) + np.abs(t_old)) + U32 * np.abs(own_t) + TINY32,
              np.maximum(U32 * np.abs(own_t), TINY32))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('per', [1, 255, 256, 257, 1023, 1024, 1025, 4097])
@dtypes
def test_elements_per_instance(torch_cuda, name, per):
    """Around one workgroup (256), one chunk (1024: two chunks from 1025 on) and 4097, where the
    strided loop of the four chunks' first threads takes another round; three instances at step
    counts 1, 2 and 1000, weight decay, target."""
    x = draw(1000 + per, 3, per, name)
    check(torch_cuda, name, x, [1.0, 2.0, 1000.0], dict(HYPER, weight_decay=1e-3), where=per)


@pytest.mark.parametrize('n', [1, 2, 37, 70000])
@dtypes
def test_instances_and_their_step_counts(torch_cuda, name, n):
    """1, 2, 37 instances of 33 elements and 70 000 of one (grid.x beyond 65 535), step counts 1,
    2, 10, 1000 and 1e6 mixed in one launch: with `active` NULL, and with an `active` that has
    zeros, under which NaN gradients change nothing."""
    per = 1 if n == 70000 else 33
    x = draw(2000 + n, n, per, name)
    steps = np.resize(STEPS, n)
    check(torch_cuda, name, x, steps, where=(n, 'all'))
    active = (np.arange(n) % 3 != 1).astype(np.uint8)
    x['g'][active == 0] = np.nan
    check(torch_cuda, name, x, steps, active=active, where=(n, 'some'))
    if n == 2:
        check(torch_cuda, name, x, steps, active=np.zeros(n, dtype=np.uint8), where=(n, 'none'))


@pytest.mark.parametrize('tau', [0.0, 0.05, 1.0])
@pytest.mark.parametrize('weight_decay', [0.0, 1e-3])
@dtypes
def test_weight_decay_target_and_tau(torch_cuda, name, weight_decay, tau):
    """Both weight decays, target NULL and given, tau 0 (the target keeps its bits), 0.05 and 1."""
    hyper = dict(HYPER, weight_decay=weight_decay, tau=tau)
    x = draw(3000, 5, 300, name)
    for target in (True, False):
        got = check(torch_cuda, name, x, STEPS, hyper, target=target, where=(weight_decay, tau, target))
        if target and tau == 0.0:
            assert _same_bits(got['t'], x['t'])


@dtypes
def test_zero_gradient_from_zero_moments_at_step_one(torch_cuda, name):
    """0 / (sqrt(0) / c + eps) is 0: the parameters keep their bits, both moments stay zero, and
    the target moves by its blend towards the UNCHANGED parameters only."""
    x = draw(4000, 3, 70, name, moments=False)
    x['g'][:] = 0.0
    got = check(torch_cuda, name, x, [1.0, 1.0, 1.0], where='zero')
    assert _same_bits(got['p'], x['p']) and not got['m'].any() and not got['v'].any()
    assert _same_bits(got['t'], x['t'] + _np(name)(HYPER['tau']) * (x['p'] - x['t']))
    assert not _same_bits(got['t'], x['t'])


@pytest.mark.parametrize('moments', [False, True])
def test_float32_gradients_whose_square_underflows(torch_cuda, moments):
    """Gradients of 1e-20 .. 1e-30 in float32: (1 - beta2) g^2 is subnormal or zero.  The moments
    are still the restatement's bit for bit (no flush to zero), and the bounds against float64
    Adam hold with their absolute term."""
    x = draw(5000, 4, 129, 'f32', moments=moments)
    rng = np.random.default_rng(5001)
    x['g'] = (rng.choice([-1.0, 1.0], size=x['g'].shape) *
              10.0 ** rng.uniform(-30, -20, size=x['g'].shape)).astype(np.float32)
    sq = (np.float32(1.0 - HYPER['beta2']) * x['g']) * x['g']
    assert (sq == 0).any() and ((sq != 0) & (sq < 2.0 ** -126)).any()
    check(torch_cuda, 'f32', x, [1.0, 2.0, 10.0, 1000.0], where=('underflow', moments))


@dtypes
def test_refusals_and_the_empty_launch(torch_cuda, name):
    """A NULL tensor, per_instance = 0 and n_instances = -1 are refused before any launch;
    n_instances = 0 is served and does nothing."""
    x = draw(6000, 2, 40, name)
    steps = np.array([1.0, 2.0])
    for what, code, kw in [(k, E_ARG, dict(nulls=(k,))) for k in ('p', 'g', 'm', 'v', 'steps')] + [
            ('per_instance', E_RANGE, dict(per=0)), ('n_instances', E_RANGE, dict(n=-1)),
            ('empty', 0, dict(n=0))]:
        rc, got, fr = launch(torch_cuda, name, x, steps, HYPER, **kw)
        assert rc == code, what
        assert all(f.intact() for f in fr.values()), what
        for k, a in x.items():
            assert _same_bits(got[k], a), (what, k)
