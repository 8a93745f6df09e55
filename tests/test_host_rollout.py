"""Host side of ``rollout`` (no GPU): the restatement of a test session against trajectories recorded
from the reference, the new exports and the struct layout, every refusal of ``cobel_tab_rollout``
before a device is asked for, and the consumers of a record on a hand-made one."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rollout_common as rc
from conftest import GOLDEN, ROOT

NEW = ('cobel_tab_rollout', 'cobel_tab_rollout_plan', 'cobel_rollout_visits')


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'rollout_traces.npz'))


# -- the fixture and the restatement ---------------------------------------------------------------------
def test_fixture_covers_the_cases_and_is_small(Z):
    assert sorted({k.split('/')[0] for k in Z.files}) == sorted(rc.CASES)
    assert os.path.getsize(os.path.join(GOLDEN, 'rollout_traces.npz')) < 256 * 1024
    tables = {rc.case(n)['table'] for n in rc.CASES}
    worlds = {rc.case(n)['world'] for n in rc.CASES}
    assert tables == {'zeros', 'plateau', 'trained'} and worlds == {'open5', 'walls8', 'track4'}
    for name in rc.CASES:
        c = rc.case(name)
        q = Z[name + '/Q']
        assert q.dtype == np.float32
        want = rc.planted_table(c['table'], *q.shape)
        if want is not None:
            assert q.tobytes() == want.tobytes(), name
        else:
            assert np.count_nonzero(q) > 0, name + ': the reference learnt nothing'
        assert np.array_equal(Z[name + '/length'], Z[name + '/steps_log'] + 1), name
        assert len(Z[name + '/positions']) == int(Z[name + '/length'].sum()), name
    # zeros: four-way ties everywhere, the walks run into the step limit; plateau: two-way ties
    assert int(Z['open5_dynaq_zeros/length'].max()) == rc.case('open5_dynaq_zeros')['steps']
    plateau = rc.plateau_table(25, 4)
    assert ((plateau == plateau.max(axis=1, keepdims=True)).sum(axis=1) == 2).all()


@pytest.mark.parametrize('name', sorted(rc.CASES))
def test_restatement_equals_the_reference(Z, name):
    c = rc.case(name)
    tabs = {k: Z['%s/world/%s' % (name, k)] for k in ('next', 'reward', 'terminal', 'starts')}
    mask = Z[name + '/action_mask'] if c['mask'] else None
    got = rc.restate(tabs, Z[name + '/Q'], c['inst'], c['eps'], c['trials'], c['steps'],
                     c['test_policy'], mask)[0]
    for k in ('start', 'states', 'actions', 'length'):
        want = Z['%s/%s' % (name, k)]
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), (name, k)
    # the monitor's positions are the coordinates of the states entered
    coords = Z[name + '/world/coordinates']
    entered = np.concatenate([got['states'][t, :got['length'][t]] for t in range(c['trials'])])
    assert np.array_equal(coords[entered], Z[name + '/positions']), name
    if c['mask']:       # masked actions never appear
        prev = np.concatenate([np.concatenate(([got['start'][t]], got['states'][t, :n - 1]))
                               for t, n in enumerate(got['length'])])
        acts = np.concatenate([got['actions'][t, :n] for t, n in enumerate(got['length'])])
        assert mask[prev, acts].all(), name


def test_generator_reruns_bit_identically(Z, tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_rollout.py')],
                          env=env)
    fresh = np.load(tmp_path / 'rollout_traces.npz')
    assert sorted(fresh.files) == sorted(Z.files)
    for k in Z.files:
        assert fresh[k].dtype == Z[k].dtype and fresh[k].tobytes() == Z[k].tobytes(), k


# -- the C ABI ---------------------------------------------------------------------------------------------
def test_exports_and_struct_layout(tmp_path):
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for name in NEW:
        m = re.search(r'COBEL_API\s+int\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert name in _lib.EXPORTS and re.search(r'\bT %s\b' % name, out), name
        assert getattr(lib, name).restype is C.c_int
        assert len(m.group(1).split(',')) == len(_lib._SIGNATURES[name][1]), name
    P, ro = C.c_void_p, C.POINTER(_lib.TabRollout)
    assert lib.cobel_tab_rollout.argtypes == [P, ro, P]
    assert lib.cobel_tab_rollout_plan.argtypes == [P, ro, C.POINTER(C.c_int32 * 4)]
    assert re.search(r'#define COBEL_ROLLOUT_ELEMENT_STORES %du\b' % _lib.ROLLOUT_ELEMENT_STORES,
                     header)
    fields = ('run', 'start', 'states', 'actions', 'length', 'trials', 'steps', 'record_flags')
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu", sizeof(cobel_tab_rollout_t), sizeof(cobel_tab_run_t));\n'
           + ''.join('printf(" %zu", offsetof(cobel_tab_rollout_t, ' + f + '));\n' for f in fields)
           + 'printf("\\n");return 0;}')
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc is not None, 'no C compiler'
    exe = str(tmp_path / 'rollout_sizeof')
    subprocess.run([cc, '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_lib.TabRollout), C.sizeof(_lib.TabRun)] + \
        [getattr(_lib.TabRollout, f).offset for f in fields]
    assert _lib.TabRollout.run.offset == 0      # (a run struct's fillers fill the head in place)


REFUSALS = [
    # changes, status, a piece of the message
    (dict(start=None), 'E_ARG', 'the record needs start, states, actions and length'),
    (dict(states=None), 'E_ARG', 'the record needs'),
    (dict(actions=None), 'E_ARG', 'the record needs'),
    (dict(length=None), 'E_ARG', 'the record needs'),
    (dict(run__q=None), 'E_ARG', 'q and inst are required'),
    (dict(run__flags=1), 'E_ARG', 'COBEL_F_LEARN is set'),
    (dict(run__step_budget=1), 'E_ARG', 'step_budget = 1'),
    (dict(trials=0), 'E_RANGE', 'trials = 0'),
    (dict(steps=0, run__steps_per_trial=0), 'E_RANGE', 'steps = 0'),
    (dict(run__steps_per_trial=4), 'E_ARG', 'the record keeps 5 steps per trial'),
    (dict(run__trial_cap=1), 'E_RANGE', 'trial_cap 1 is too small for trials_target 2'),
    (dict(run__trials_target=1), 'E_RANGE', 'trials_target 1 is below'),
]


@pytest.mark.parametrize('changes,status,message', REFUSALS,
                         ids=['-'.join(c[0]) for c in REFUSALS])
def test_refusals_come_before_any_device_call(changes, status, message):
    """Both entry points, a world handle that names no device: the status and the message are the
    argument checks' (a check that reached the runtime would answer COBEL_E_HIP here)."""
    from cobel_amd import _lib
    lib, arrays, world = _lib.lib(), rc.HostArrays(), rc.fake_world()
    ro = rc.fill_rollout(_lib, arrays, **changes)
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    for call in (lambda: lib.cobel_tab_rollout(C.addressof(world), C.byref(ro), None),
                 lambda: lib.cobel_tab_rollout_plan(C.addressof(world), C.byref(ro), C.byref(out))):
        assert call() == getattr(_lib, status)
        assert message in lib.cobel_last_error().decode()
    assert list(out) == [0, 0, 0, 0]
    with pytest.raises({'E_ARG': AssertionError, 'E_RANGE': IndexError}[status], match=message):
        _lib.check(lib.cobel_tab_rollout(C.addressof(world), C.byref(ro), None))


def test_refusals_that_read_the_world_handle():
    from cobel_amd import _lib
    lib, arrays = _lib.lib(), rc.HostArrays()
    ro = rc.fill_rollout(_lib, arrays)
    world = rc.fake_world(n_actions=33)
    assert lib.cobel_tab_rollout(C.addressof(world), C.byref(ro), None) == _lib.E_UNSUPPORTED
    assert '33 actions (1..32 are served)' in lib.cobel_last_error().decode()
    with pytest.raises(NotImplementedError, match='33 actions'):
        _lib.check(lib.cobel_tab_rollout(C.addressof(world), C.byref(ro), None))
    # q: rows of four values are read as one 16-byte load; other rows value by value
    four, six = rc.fake_world(n_actions=4), rc.fake_world(n_actions=6)
    ro = rc.fill_rollout(_lib, arrays, run__q=arrays.q.ctypes.data + 4)
    assert lib.cobel_tab_rollout(C.addressof(four), C.byref(ro), None) == _lib.E_ARG
    assert 'q is misaligned' in lib.cobel_last_error().decode()
    # (the plan entry point: nothing is launched where a device answers the last check)
    out = (C.c_int32 * 4)()
    assert lib.cobel_tab_rollout_plan(C.addressof(six), C.byref(ro), C.byref(out)) != _lib.E_ARG
    ro = rc.fill_rollout(_lib, arrays, run__q=arrays.q.ctypes.data + 2)
    assert lib.cobel_tab_rollout(C.addressof(six), C.byref(ro), None) == _lib.E_ARG
    assert 'q is misaligned' in lib.cobel_last_error().decode()
    ro = rc.fill_rollout(_lib, arrays, states=arrays.states.ctypes.data + 2)
    assert lib.cobel_tab_rollout(C.addressof(four), C.byref(ro), None) == _lib.E_ARG
    assert 'the record is misaligned' in lib.cobel_last_error().decode()
    # NULL arguments
    assert lib.cobel_tab_rollout(None, C.byref(ro), None) == _lib.E_ARG
    assert lib.cobel_tab_rollout(C.addressof(four), None, None) == _lib.E_ARG
    assert lib.cobel_tab_rollout_plan(C.addressof(four), C.byref(ro), None) == _lib.E_ARG
    assert lib.cobel_rollout_visits(None, 1, 1, 25, 1, 0, None, None) == _lib.E_ARG
    assert lib.cobel_rollout_visits(arrays.states.ctypes.data, 1, 0, 25, 1, 0,
                                    arrays.length.ctypes.data, None) == _lib.E_RANGE


# -- the Python surface ----------------------------------------------------------------------------------------
def test_sfma_refuses_and_the_other_agents_have_no_rollout():
    from cobel_amd import agent as agents
    from cobel_amd.agent.sfma import SFMA
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    ag = SFMA(Discrete(25), Discrete(4), EpsilonGreedy(0.1), None)
    with pytest.raises(NotImplementedError, match='QAgent and DynaQ'):
        ag.rollout(None, 2, 5)
    assert hasattr(agents.QAgent, 'rollout') and hasattr(agents.DynaQ, 'rollout')
    from cobel_amd.agent.sr import SR
    assert not hasattr(SR, 'rollout')


class _Env:
    """Two stacked 2x2 worlds with coordinates of their own, no device."""
    instance_base = 1
    device = 'cpu'
    _coords = [np.array([[0., 0.], [1., 0.], [0., 1.], [1., 1.]]),
               np.array([[5., 5.], [6., 5.], [5., 6.], [6., 6.]])]


def hand_made_record():
    import torch
    from cobel_amd.monitor import TrajectoryRecord
    rec = TrajectoryRecord(_Env(), 2, 2, 3, device='cpu')
    rec.start.copy_(torch.tensor([[0, 3], [2, 1]], dtype=torch.int16))
    rec.states.copy_(torch.tensor([[[1, 3, 2], [2, -1, -1]], [[0, 0, -1], [3, 1, 0]]],
                                  dtype=torch.int16))
    rec.actions.copy_(torch.tensor([[[2, 3, 0], [1, 255, 255]], [[1, 1, 255], [3, 1, 0]]],
                                   dtype=torch.uint8))
    rec.length.copy_(torch.tensor([[3, 1], [2, 3]], dtype=torch.int32))
    return rec


def test_trajectory_and_the_monitor_on_a_hand_made_record():
    from cobel_amd.analysis.behavior_spatial import get_occupancy_map
    from cobel_amd.monitor import TrajectoryMonitor
    rec = hand_made_record()
    a, b = _Env._coords
    # instance 0 has global id 1: the second world; instance 1 the first
    assert [rec.world_of(0), rec.world_of(1)] == [1, 0]
    assert np.array_equal(rec.trajectory(0, 0), b[[1, 3, 2]])
    assert np.array_equal(rec.trajectory(0, 1), b[[2]])
    assert np.array_equal(rec.trajectory(1, 0), a[[0, 0]])
    assert np.array_equal(rec.trajectory(1, 1), a[[3, 1, 0]])
    mon = TrajectoryMonitor(2, _Env())
    mon.trajectory_trace.append(['kept'])
    mon.update_from_device(rec)
    trace = mon.get_trace()
    assert trace[0] == ['kept'] and len(trace) == 5
    want = [b[[1, 3, 2]], b[[2]], a[[0, 0]], a[[3, 1, 0]]]      # instance-major
    for got, exp in zip(trace[1:], want):
        assert isinstance(got, list) and np.array_equal(got, exp)
    mon.update_from_device(rec, instances=[1])
    assert len(mon.get_trace()) == 7 and np.array_equal(mon.get_trace()[5], a[[0, 0]])
    # the lists are what get_occupancy_map takes
    occ = get_occupancy_map(rec.trajectories([1]), 2.0, 2.0, 1.0)
    assert occ.sum() == 5


def test_a_record_names_its_size_when_it_cannot_fit(monkeypatch):
    import torch
    from cobel_amd.monitor import trajectory
    assert trajectory.record_bytes(65536, 20, 50) == 65536 * 20 * 156
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda device=None: (1000, 2000))
    env = _Env()
    env.device = 'cuda:0'
    with pytest.raises(MemoryError, match='takes 4992 bytes .* 1000 bytes of device memory'):
        trajectory.TrajectoryRecord(env, 4, 8, 50)
