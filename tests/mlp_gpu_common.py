"""What the GPU edge tests of the stacked-network kernels share (tests/test_gpu_mlp_edges.py,
tests/test_gpu_dqn_replay_edges.py): outputs framed by sentinels, torch's float32 on the CPU as the
yardstick of the float32 kernels, and the comparison that records the worst figures."""
import ctypes as C

import numpy as np

import mlp_common as mc

DEV = 'cuda'
PAD = 96                   # sentinel elements in front of and behind every output
SENTINEL, SENTINEL_U8 = -777.25, 0xA5
# What torch's float32 may differ from the float64 reference by before the comparison is void (a
# wrong reference would otherwise widen the kernel's bound with it).  Forward passes and gradients
# are sums of at most 64 products: 1e-4 is 100x the largest figure measured (1e-6, D = O = 1).
# After an Adam step a gradient's error is divided by sqrt(v) + eps — at most lr / eps = 3e5 times
# a gradient error of ~1e-8 absolute for a network that starts from zero moments, measured 5e-5 —
# and everything later follows the parameters: 1e-2.
YARD_CAP, YARD_CAP_FIT = 1e-4, 1e-2


def _np(name):
    return np.float64 if name == 'f64' else np.float32


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _stack_dev(torch, stack):
    return {k: _dev(torch, a) for k, a in stack.items()}


def _launch(name, run):
    from cobel_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(C.byref(run), None))


class Framed:
    """An output tensor in the middle of a buffer of sentinels."""

    def __init__(self, torch, shape, dtype, fill=SENTINEL):
        count = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((count + 2 * PAD,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + count].view(shape)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all() and (self.buf[-PAD:] == self.fill).all())

    def untouched(self, j):
        return bool((self.view[j] == self.fill).all())


def _torch_dtype(torch, name):
    return torch.float64 if name == 'f64' else torch.float32


# ---------------------------------------------------------------------------------------------
# torch's float32 on the CPU: the yardstick of the float32 kernels
def _t32_forward(torch, p, x):
    h = torch.relu(x @ p['w1'].T + p['b1'])
    h = torch.relu(h @ p['w2'].T + p['b2'])
    return h @ p['w3'].T + p['b3']


def _t32_loss(torch, p, x, y, mask):
    q = _t32_forward(torch, p, x)
    on = torch.ones(x.shape[0]) if mask is None else torch.from_numpy((mask != 0).astype(np.float32))
    return (((q - y) ** 2) * on[:, None]).sum() / (max(float(on.sum()), 1.0) * q.shape[1])


def _t32_grads(torch, p, x, y, mask):
    leaf = {k: a.clone().requires_grad_() for k, a in p.items()}
    _t32_loss(torch, leaf, x, y, mask).backward()
    return {k: a.grad for k, a in leaf.items()}


def _t32_fit_step(torch, net, x, y, mask, train, hyper):
    out = dict(net)
    if train:
        leaf = {k: a.clone().requires_grad_() for k, a in net['p'].items()}
        opt = torch.optim.Adam([leaf[k] for k in mc.KEYS], lr=hyper['lr'], eps=hyper['eps'],
                               betas=(hyper['beta1'], hyper['beta2']),
                               weight_decay=hyper['weight_decay'])
        for k in mc.KEYS:
            opt.state[leaf[k]] = {'step': torch.tensor(float(net['steps'])),
                                  'exp_avg': net['m'][k].clone(), 'exp_avg_sq': net['v'][k].clone()}
        _t32_loss(torch, leaf, x, y, mask).backward()
        opt.step()
        out['p'] = {k: leaf[k].detach() for k in mc.KEYS}
        out['m'] = {k: opt.state[leaf[k]]['exp_avg'] for k in mc.KEYS}
        out['v'] = {k: opt.state[leaf[k]]['exp_avg_sq'] for k in mc.KEYS}
        out['steps'] = net['steps'] + 1.0
    if hyper['tau'] != 0.0 and net.get('t') is not None:
        out['t'] = {k: torch.lerp(net['t'][k], out['p'][k], hyper['tau']) for k in mc.KEYS}
    return out


def agree(figures, key, name, got, ref, t32=None, grad=False, where=None, after_adam=False,
          t32_ref=None):
    """The kernel's ``got`` against the float64 ``ref``; float32: measured against torch's, the
    worst (kernel, torch) pair kept in ``figures[key]``.  ``after_adam``: the yardstick's cap is
    YARD_CAP_FIT.  ``t32_ref``: what torch's result is held against where ``ref`` was formed from
    the kernel's own intermediate results (the same float64 operation on torch's own)."""
    if name == 'f64':
        if grad:
            err = mc.rel_err(got, ref)
            assert err <= 1e-12, (key, where, err)
        else:
            assert np.allclose(got, ref, rtol=1e-9, atol=1e-12), \
                (key, where, float(np.abs(got - ref).max()))
        return
    kernel, yard = mc.rel_err(got, ref), mc.rel_err(_host(t32), ref if t32_ref is None else t32_ref)
    # (the yardstick has to be one: torch's float32 and the reference compute the same thing)
    assert yard <= (YARD_CAP_FIT if after_adam else YARD_CAP), (key, where, yard)
    if key not in figures or kernel > figures[key][0]:
        figures[key] = (kernel, yard)
    assert kernel <= mc.f32_bound(yard), (key, where, 'kernel %.3e torch %.3e' % (kernel, yard))


def _stack_host(stack):
    return {k: _host(a) for k, a in stack.items()}
