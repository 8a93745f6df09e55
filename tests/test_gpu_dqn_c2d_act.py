"""cobel_dqn_act_c2d alone, with given Q arrays, over 12 consecutive calls on the state the
kernel left in device memory: after every call every array — the arena's state and env_ctr, the
policy and memory counters, the five ring arrays with size and head, trial, step, trial_reward,
active, adam_steps, the three monitors, stepped, batch_slots, obs, reward / done / wall and the
fallback counter — is compared bit for bit (np.array_equal) with the restatement of
tests/dqn_c2d_common.py, whose cases tests/test_host_dqn_c2d.py holds to their conditions.  Every
array sits in a sentinel frame (c2d_common.framed), checked after every call.

The step robot (the restatement is exact for it), 70 instances — across a wavefront and, at four
lanes per instance, across a workgroup — batch 3, a ring of 5 slots, 5 steps per trial, 3 trials,
instance_base 10; the open field, the eight-maze and the wedge (every reset takes the fallback);
every lane count 0 (the planner's), 1, 4, 16, 64 against the SAME reference, so all give the same
bits; both dtypes of the ring."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c2d_common as cc  # noqa: E402
import dqn_c2d_common as dc  # noqa: E402

pytestmark = pytest.mark.gpu

LANES = (0, 1, 4, 16, 64)
SCALARS = ('slots', 'batch', 'steps_per_trial', 'trials_target', 'trial_cap', 'mon_stripes',
           'epsilon', 'policy_stream', 'is_float64')


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def _torch_dtype(torch, a):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
            np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32}[a.dtype]


class DeviceCase:
    """The state of a case on the device, every array framed, and the arena's tables."""

    def __init__(self, torch, case, lanes):
        from cobel_amd import _lib
        self.torch, self.case, self._lib = torch, case, _lib
        arena, par = case['arena'], case['par']
        self.views, self.checks = {}, []
        for k, a in case['state'].items():
            dt = _torch_dtype(torch, a)
            fill = -777.25 if dt.is_floating_point else (0x5A if dt == torch.uint8 else -777)
            view, check = cc.framed(torch, a.shape, dt, fill)
            signed = a.view(np.int32) if a.dtype == np.uint32 else a
            view.copy_(torch.from_numpy(np.ascontiguousarray(signed)).to('cuda'))
            self.views[k] = view
            self.checks.append(check)
        self.tables = [torch.as_tensor(np.ascontiguousarray(t), device='cuda')
                       for t in (arena['T'], arena['S'], np.asarray(arena['R'], dtype=np.float64))]
        run = _lib.DQNActC2D()
        run.arena = cc.fill(_lib, _lib.ptr(self.tables[0]), _lib.ptr(self.tables[1]),
                            _lib.ptr(self.tables[2]), _lib.ptr(self.views['state']),
                            _lib.ptr(self.views['env_ctr']), par['n'], arena['T'].shape[1],
                            arena['S'].shape[1], len(arena['R']), arena['box'], arena['fallback'],
                            robot=arena['robot'], seed=par['seed'], base=par['instance_base'],
                            lanes=lanes, **arena['params'])
        for k in dc.ARRAYS[2:]:
            setattr(run, k, _lib.ptr(self.views[k]))
        for k in SCALARS:
            setattr(run, k, par[k])
        self.run = run

    def call(self, q):
        self.views['q'].copy_(self.torch.from_numpy(np.ascontiguousarray(q)).to('cuda'))
        self._lib.check(self._lib.lib().cobel_dqn_act_c2d(C.byref(self.run), None))
        self.torch.cuda.synchronize()
        for check in self.checks:
            check()
        out = {}
        for k, v in self.views.items():
            a = v.detach().cpu().numpy()
            out[k] = a.view(np.uint32) if self.case['state'][k].dtype == np.uint32 else a
        return out


def replay(torch, case, lanes):
    """The case's calls on the device, each against the restatement's state after that call."""
    dev = DeviceCase(torch, case, lanes)
    for k, (q, ref) in enumerate(case['steps']):
        got = dev.call(q)
        assert dc.same(got, dict(ref, q=q)) == [], (case['name'], lanes, k)
    return got


@pytest.mark.parametrize('f64', [True, False], ids=['f64', 'f32'])
@pytest.mark.parametrize('name', sorted(dc.NEEDS))
def test_twelve_calls_match_the_restatement_for_every_lane_count(torch_cuda, name, f64):
    case = dc.make_case(name, f64)
    for lanes in LANES:
        got = replay(torch_cuda, case, lanes)
    assert (got['active'] == 0).any() and got['ring_size'].max() == 5


def test_one_instance_alone(torch_cuda):
    """n = 1 (instance_base 10): one group in one workgroup, every other lane walks along."""
    case = dc.make_case('open_field', True, n=1, trials_target=40)
    for lanes in LANES:
        replay(torch_cuda, case, lanes)


def test_all_instances_frozen(torch_cuda):
    """Nothing is written and no counter moves: every array keeps its bytes, stepped becomes 0."""
    case = dc.make_case('eight', True)
    for lanes in (0, 64):
        dev = DeviceCase(torch_cuda, case, lanes)
        dev.views['active'].zero_()
        before = {k: v.detach().cpu().numpy().copy() for k, v in dev.views.items()}
        q = np.full_like(case['qs'][0], np.nan)
        got = dev.call(q)
        assert not got['stepped'].any()
        for k, v in dev.views.items():
            if k not in ('stepped', 'q'):
                assert v.detach().cpu().numpy().tobytes() == before[k].tobytes(), k


@pytest.mark.parametrize('mode,epsilon', [('ties', 0.3), ('mixed', 1.0), ('mixed', 0.0)],
                         ids=['all-ties', 'eps1', 'eps0'])
def test_selections_at_their_edges(torch_cuda, mode, epsilon):
    """Four equal Q-values in every instance; epsilon = 1 (uniform whatever Q holds) and 0."""
    case = dc.make_case('open_field', False, mode=mode, epsilon=epsilon)
    for lanes in (0, 16):
        replay(torch_cuda, case, lanes)
