"""cobel_adqn_store / cobel_adqn_sample and the ADQNMemory class on the device against the NumPy
restatement of tests/adqn_common.py (``RefMemory``: the device's summation order), np.array_equal on
every array, at the counts where a chunk or the wavefront ends, with sentinels around every array."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adqn_common as ac  # noqa: E402
from mlp_gpu_common import DEV, SENTINEL, Framed, _dev, _host  # noqa: E402
from oracle.philox import TapeRNG  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

D = 3
SEAMS = [1, 2, 63, 64, 65, 128, 129, 300]      # chunks of 1 | 2 | 3 | 5 entries, a full wavefront
BASE = 40                                      # instance numbers BASE + j


def experiences(count, j, zero=False):
    rng = np.random.default_rng([count, j])
    states = rng.random((count, D))
    rewards = rng.integers(-1, 2, count).astype(np.float64)
    actions = rewards.copy() if zero else rng.standard_normal(count)
    return states, actions, rewards


_BUILT = {}


def built(count, j, decay, rpe, zero=False, upto=None):
    """The restated memory of instance j after ``upto`` (default: all) of its experiences; shared,
    not to be written to (``fresh`` hands out copies with a tape of their own)."""
    upto = count if upto is None else upto
    key = (count, j, decay, rpe, zero, upto)
    if key not in _BUILT:
        s, a, r = experiences(count, j, zero)
        mem = ac.RefMemory(D, decay, rpe)
        for k in range(upto):
            mem.store(s[k], a[k], r[k])
        _BUILT[key] = mem
    return _BUILT[key]


def fresh(mem, j, start=0):
    out = ac.RefMemory(D, mem.decay, mem.rpe, TapeRNG(ac.SEED, BASE + j, ac.STREAM_ADQN_MEMORY, start))
    for k, v in ac.memory_arrays(mem).items():
        setattr(out, k, v.copy())
    return out


class DeviceMemory:
    """Caller-owned arrays of N instances of capacity cap, every one framed by sentinels."""

    def __init__(self, N, cap):
        self.N, self.cap = N, cap
        f = torch.float64
        self.f = {'states': Framed(torch, (N, cap, D), f), 'reinforcements': Framed(torch, (N, cap), f),
                  'errors': Framed(torch, (N, cap), f), 'priorities': Framed(torch, (N, cap), f),
                  'scratch': Framed(torch, (N, cap), f),
                  'count': Framed(torch, (N,), torch.int32, -7),
                  'draw_ctr': Framed(torch, (N,), torch.int32, -7)}
        self.f['count'].view.zero_()
        self.f['draw_ctr'].view.zero_()
        self.t = {k: v.view for k, v in self.f.items()}
        self.h_count = np.zeros(N, dtype=np.int64)

    def load(self, j, mem):
        n = len(mem.priorities)
        for k, v in ac.memory_arrays(mem).items():
            self.t[k][j, :n] = _dev(torch, v)
        self.t['count'][j] = n
        self.h_count[j] = n

    def struct(self, decay, rpe):
        from cobel_amd import _lib
        return ac.fill_mem(_lib, self.t, self.N, D, self.cap, int(self.h_count.min()),
                           int(self.h_count.max()), decay, rpe, instance_base=BASE)

    def store(self, decay, rpe, states, actions, rewards):
        from cobel_amd import _lib
        K = states.shape[1]
        s, a, r = (_dev(torch, v) for v in (states, actions, rewards))
        m = self.struct(decay, rpe)
        _lib.check(_lib.lib().cobel_adqn_store(C.byref(m), K, _lib.ptr(s), _lib.ptr(a), _lib.ptr(r),
                                               None))
        self.h_count += K

    def sample(self, decay, rpe, B, f64=True):
        from cobel_amd import _lib
        out = {'idx': Framed(torch, (self.N, B), torch.int32, -7),
               'in_index': Framed(torch, (self.N, B), torch.int32, -7),
               'targets': Framed(torch, (self.N, B), torch.float64 if f64 else torch.float32)}
        m = self.struct(decay, rpe)
        _lib.check(_lib.lib().cobel_adqn_sample(C.byref(m), B, int(f64), _lib.ptr(out['idx'].view),
                                                _lib.ptr(out['in_index'].view),
                                                _lib.ptr(out['targets'].view), None))
        torch.cuda.synchronize()
        assert all(v.intact() for v in out.values())
        return {k: _host(v.view) for k, v in out.items()}

    def check(self, mems, what=''):
        """Every array equals the restated memories, nothing behind a count was written, and the
        sentinels stand."""
        torch.cuda.synchronize()
        for k, fr in self.f.items():
            assert fr.intact(), (what, k)
        assert _host(self.t['count']).tolist() == [len(m.priorities) for m in mems], what
        for j, mem in enumerate(mems):
            n = len(mem.priorities)
            for k, v in ac.memory_arrays(mem).items():
                got = _host(self.t[k][j])
                assert np.array_equal(got[:n], v), (what, j, k)
                assert (got[n:] == SENTINEL).all(), (what, j, k, 'written behind the count')


def check_draw(got, mems, cap, B, what=''):
    for j, mem in enumerate(mems):
        idx = mem.sample(B)
        assert np.array_equal(got['idx'][j], idx), (what, j, got['idx'][j], idx)
        assert np.array_equal(got['in_index'][j], j * cap + idx), (what, j)
        assert np.array_equal(got['targets'][j], mem.reinforcements[idx].astype(got['targets'].dtype)), \
            (what, j)


@pytest.mark.parametrize('B', [1, 32, 33, 100])
@pytest.mark.parametrize('decay,rpe', [(1.0, True), (0.9, True), (0.0, True), (0.9, False)])
def test_store_and_draw_at_the_seams(B, decay, rpe):
    """Eight instances with the counts 1, 2, 63, 64, 65, 128, 129 and 300 in one launch — the last
    fills its memory exactly to cap: the launch stores every instance's LAST experience on top of
    count - 1 loaded ones, then two draws follow (the second continues the stream)."""
    N, cap = len(SEAMS), max(SEAMS)
    dm = DeviceMemory(N, cap)
    last = [experiences(c, j) for j, c in enumerate(SEAMS)]
    for j, c in enumerate(SEAMS):
        dm.load(j, built(c, j, decay, rpe, upto=c - 1))
    dm.store(decay, rpe, np.stack([s[-1:] for s, _, _ in last]), np.stack([a[-1:] for _, a, _ in last]),
             np.stack([r[-1:] for _, _, r in last]))
    mems = [fresh(built(c, j, decay, rpe), j) for j, c in enumerate(SEAMS)]
    dm.check(mems, 'store')
    if decay == 0.0:        # only the newest priority survives
        pr = _host(dm.t['priorities'])
        assert all(not pr[j, :c - 1].any() for j, c in enumerate(SEAMS))
    for call in range(2):
        check_draw(dm.sample(decay, rpe, B), mems, cap, B, 'draw %d' % call)
    assert _host(dm.t['draw_ctr']).tolist() == [2] * N
    scratch = _host(dm.t['scratch'])
    for j, mem in enumerate(mems):
        assert np.array_equal(scratch[j, :SEAMS[j]], ac.device_cdf(mem.priorities)), j
    dm.check(mems, 'after the draws')
    from cobel_amd import _lib
    with pytest.raises(IndexError, match='1 experiences on top of 300 pass the capacity of 300'):
        dm.store(decay, rpe, np.zeros((N, 1, D)), np.zeros((N, 1)), np.zeros((N, 1)))
    assert isinstance(_lib.lib().cobel_last_error(), bytes)


@pytest.mark.parametrize('counts', [[129], [3, 64, 65, 1, 200]], ids=['n1', 'n5'])
def test_instance_counts_that_do_not_fill_a_workgroup(counts):
    """One instance, and five (a workgroup holds four): float32 targets, the uniform instance
    numbers of a launch at base 40."""
    N, cap = len(counts), max(counts) + 5
    dm = DeviceMemory(N, cap)
    for j, c in enumerate(counts):
        dm.load(j, built(c, j, 0.9, True))
    mems = [fresh(built(c, j, 0.9, True), j) for j, c in enumerate(counts)]
    check_draw(dm.sample(0.9, True, 32, f64=False), mems, cap, 32)
    dm.check(mems)


def test_k_stores_in_one_launch_from_empty():
    """70 experiences per instance in one launch: every priority is multiplied by decay once per
    later store, each product rounded."""
    N, K, cap = 5, 70, 70
    dm = DeviceMemory(N, cap)
    exps = [experiences(K, j) for j in range(N)]
    dm.store(0.9, True, *(np.stack([e[k] for e in exps]) for k in range(3)))
    mems = [fresh(built(K, j, 0.9, True), j) for j in range(N)]
    dm.check(mems)
    check_draw(dm.sample(0.9, True, 33), mems, cap, 33)


@pytest.mark.parametrize('counts', [[1, 5, 64, 65, 130]])
def test_all_priorities_zero_draws_uniformly(counts):
    """action == reward in every experience and rpe on: prob_sum == 0, 1 / n each."""
    N, cap = len(counts), max(counts)
    dm = DeviceMemory(N, cap)
    for j, c in enumerate(counts):
        dm.load(j, built(c, j, 1.0, True, zero=True, upto=c - 1))
    last = [experiences(c, j, zero=True) for j, c in enumerate(counts)]
    dm.store(1.0, True, *(np.stack([e[k][-1:] for e in last]) for k in range(3)))
    mems = [fresh(built(c, j, 1.0, True, zero=True), j) for j, c in enumerate(counts)]
    assert all(not m.priorities.any() for m in mems)
    dm.check(mems)
    got = dm.sample(1.0, True, 100)
    check_draw(got, mems, cap, 100)
    assert len(set(got['idx'][4].tolist())) > 30


def test_empty_memory_and_bad_arguments_are_refused_on_the_device_path():
    dm = DeviceMemory(2, 8)
    dm.load(1, built(2, 1, 1.0, True))
    with pytest.raises(IndexError, match='an empty memory has nothing to draw'):
        dm.sample(1.0, True, 4)
    with pytest.raises(AssertionError, match='decay = 1.5'):
        dm.sample(1.5, True, 4)
    torch.cuda.synchronize()
    assert all(fr.intact() for fr in dm.f.values()) and _host(dm.t['draw_ctr']).tolist() == [0, 0]


@pytest.mark.parametrize('n_envs', [1, 3])
def test_the_memory_class_grows_and_returns_what_the_reference_returns(n_envs):
    """ADQNMemory.store / sample_batch through a capacity growth (16 -> 32 -> 64), against the
    restatement: the reference's return values and attribute shapes for one instance, padded device
    tensors with ``count`` for three."""
    from cobel_amd.memory import ADQNMemory
    from cobel_amd.spaces import Box
    shape = (D, 1)
    mem = ADQNMemory(Box(0.0, 1.0, shape), 0.9, True, n_envs=n_envs, seed=ac.SEED, device=DEV,
                     instance_base=BASE)
    refs = [ac.RefMemory(D, 0.9, True, TapeRNG(ac.SEED, BASE + j, ac.STREAM_ADQN_MEMORY))
            for j in range(n_envs)]
    exps = [experiences(40, j) for j in range(n_envs)]
    with pytest.raises(ValueError):
        mem.sample_batch(4)
    for k in range(40):
        for j, ref in enumerate(refs):
            ref.store(exps[j][0][k], exps[j][1][k], exps[j][2][k])
        if n_envs == 1:
            mem.store({'state': exps[0][0][k].reshape(shape), 'action': float(exps[0][1][k]),
                       'reward': float(exps[0][2][k])})
        else:
            mem.store({'state': np.stack([e[0][k].reshape(shape) for e in exps]),
                       'action': np.array([e[1][k] for e in exps]),
                       'reward': torch.as_tensor(np.array([e[2][k] for e in exps]), device=DEV)})
        if k in (0, 15, 16, 39):
            obs, rew = mem.sample_batch(5)
            for j, ref in enumerate(refs):
                idx = ref.sample(5)
                o, r = (obs, rew) if n_envs == 1 else (_host(obs[j]), _host(rew[j]))
                assert o.shape == (5,) + shape and r.shape == (5,)
                assert np.array_equal(o.reshape(5, D), ref.states[idx]), (k, j)
                assert np.array_equal(r, ref.reinforcements[idx]), (k, j)
    assert mem.cap == 64
    for j, ref in enumerate(refs):
        for key, want in ac.memory_arrays(ref).items():
            got = getattr(mem, key)
            got = got if n_envs == 1 else _host(got[j])
            assert np.array_equal(got.reshape(want.shape), want), (j, key)
    if n_envs == 1:
        assert mem.count == 40 and type(mem.states) is np.ndarray and mem.states.shape == (40,) + shape
    else:
        assert _host(mem.count).tolist() == [40] * n_envs
