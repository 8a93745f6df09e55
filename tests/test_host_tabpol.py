"""Host side of the Softmax / ExclusiveEpsilonGreedy / RandomDiscrete runs of QAgent and DynaQ (no
GPU): the restatement against traces recorded from the reference, the restated probabilities against
the reference's on random rows, the margins the comparisons on the device rest on, the new exports and
the struct layout, and every refusal of ``cobel_tab_policy_run`` that needs no device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import tabpol_common as tc
from conftest import GOLDEN, ROOT

NEW = ('cobel_tab_policy_run', 'cobel_tab_policy_plan', 'cobel_policy_select_n')


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'tabpol_traces.npz'))


@pytest.fixture(scope='module')
def tools():
    from cobel_amd.misc import gridworld_tools, topology_tools
    return gridworld_tools, topology_tools


# -- the fixture and the restatement ---------------------------------------------------------------------
def test_fixture_covers_the_cases_and_is_small(Z):
    assert sorted({k.split('/')[0] for k in Z.files} - {'rows'}) == sorted(tc.CASES)
    assert os.path.getsize(os.path.join(GOLDEN, 'tabpol_traces.npz')) < 256 * 1024
    for name in tc.CASES:
        c = tc.case(name)
        assert Z[name + '/Q'].dtype == np.float32 and np.count_nonzero(Z[name + '/Q']) > 0, name
        assert len(Z[name + '/steps']) == tc.TRIALS * (2 if c['opt'].get('test') else 1), name
        assert int(Z[name + '/steps'].min()) < tc.STEPS - 1, name + ': no trial reached the goal'
    assert Z['q_soft_hex/world/next'].shape[1] == 6
    # the mask of its case removes two actions in some states, and they are never taken
    m = Z['dynaq_soft_mask/action_mask']
    assert set(m.sum(axis=1)) == {2, 4}
    assert m[Z['dynaq_soft_mask/state'], Z['dynaq_soft_mask/action']].all()


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_margin_of_every_case(Z, name):
    """Every uniform draw of the reference's run lies at least 1e-9 from every edge of its CDF."""
    assert float(Z[name + '/margin']) >= tc.MARGIN, name


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_restatement_equals_the_reference(Z, tools, name):
    """Steps, per-trial tables, model / log, counters: bit for bit.  (td of a QAgent step: the
    reference's logs carry the td of the LAST update of the step's experience, which a replay of it
    in the same step overwrites; the restatement and the kernels report the online one.)"""
    c = tc.case(name)
    tabs = tc.case_tables(c, *tools)
    for k in ('next', 'reward', 'terminal', 'starts'):
        assert np.array_equal(tabs[k], Z['%s/world/%s' % (name, k)]), (name, k)
    got = tc.restate_case(name, tabs)
    for k in tc.EXACT:
        if k not in got or (k == 'td' and c['agent'] == 'q'):
            continue
        want = Z['%s/%s' % (name, k)]
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), (name, k)
    assert got['margin'] >= tc.MARGIN


def test_restated_probabilities_equal_the_references(Z):
    """Random rows of one to eight values, float64 input, some masked: ExclusiveEpsilonGreedy bit for
    bit; Softmax bit for bit up to seven summed values — eight NumPy adds pairwise, the device and
    the restatement in action order: one rounding of the sum apart (2**-52 relative, bounded by
    2**-51 here)."""
    R = {k[5:]: Z[k] for k in Z.files if k.startswith('rows/')}
    eights = 0
    for k in range(len(R['A'])):
        a = int(R['A'][k])
        m = np.array([(int(R['bits'][k]) >> j) & 1 for j in range(a)], dtype=bool)
        e = tc.exclusive_probs(R['vq'][k, :a], R['eps'][k], m)
        assert e.tobytes() == R['excl'][k, :a].tobytes(), k
        s, want = tc.softmax_probs(R['v'][k, :a], R['beta'][k], m), R['soft'][k, :a]
        if m.sum() < 8:
            assert s.tobytes() == want.tobytes(), k
        else:
            eights += 1
            assert np.all(np.abs(s - want) <= 2.0 ** -51 * want), k
    assert eights >= 10 and len(R['A']) >= 200
    # RandomDiscrete: full(A, 1 / A), one bounded draw whatever the row
    from oracle.philox import STREAM_POLICY, TapeRNG, draw_bounded
    p = tc.RefPolicy(tc.RANDOM, None, TapeRNG(tc.SEED, 3, STREAM_POLICY), 6)
    assert np.array_equal(p.get_action_probs(np.zeros(6)), np.full(6, 1.0 / 6))
    acts = [p.select_action(np.zeros(6)) for _ in range(9)]
    assert acts == [int(draw_bounded(tc.SEED, 3, c, 0, STREAM_POLICY, 6)) for c in range(9)]


@pytest.mark.parametrize('name', sorted(tc.SWEEPS))
def test_margins_of_the_device_sweeps(tools, name):
    """A condition of tests/test_gpu_tabpol.py: in its sweeps no draw of the restatement lies within
    1e-12 of an edge of its CDF, so equality on the device cannot hinge on exp's last bit."""
    R = tc.restate_sweep(name, tools[0])
    s = tc.sweep(name)
    assert len(R) == (s['n'] if s['check'] is None else len(s['check']))
    assert min(r.margin() for r in R.values()) >= tc.SWEEP_MARGIN, name


def test_generator_reruns_bit_identically(Z, tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_tabpol.py')],
                          env=env)
    fresh = np.load(tmp_path / 'tabpol_traces.npz')
    assert sorted(fresh.files) == sorted(Z.files)
    for k in Z.files:
        assert fresh[k].dtype == Z[k].dtype and fresh[k].tobytes() == Z[k].tobytes(), k


# -- the C ABI ---------------------------------------------------------------------------------------------
def test_exports_and_struct_layout(tmp_path):
    from cobel_amd import _lib
    from cobel_amd import policy
    assert policy.ExclusiveEpsilonGreedy.__mro__[1] is policy.EpsilonGreedy
    assert hasattr(policy, 'RandomDiscrete') and hasattr(policy.ExclusiveEpsilonGreedy, 'parameter_column')
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    assert lib.cobel_abi_version() == 1017
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for name in NEW:
        m = re.search(r'COBEL_API\s+int\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert name in _lib.EXPORTS and re.search(r'\bT %s\b' % name, out), name
        assert getattr(lib, name).restype is C.c_int
        assert len(m.group(1).split(',')) == len(_lib._SIGNATURES[name][1]), name
    for name, value in (('SOFTMAX', _lib.POLICY_SOFTMAX), ('EXCLUSIVE', _lib.POLICY_EXCLUSIVE),
                        ('RANDOM', _lib.POLICY_RANDOM)):
        assert re.search(r'COBEL_POLICY_%s = %d\b' % (name, value), header)
    fields = ('run', 'policy', 'policy_param', 'policy_params')
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu", sizeof(cobel_tab_policy_run_t), sizeof(cobel_tab_run_t));\n'
           + ''.join('printf(" %zu", offsetof(cobel_tab_policy_run_t, ' + f + '));\n' for f in fields)
           + 'printf("\\n");return 0;}')
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc is not None, 'no C compiler'
    exe = str(tmp_path / 'tabpol_sizeof')
    subprocess.run([cc, '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_lib.TabPolicyRun), C.sizeof(_lib.TabRun)] + \
        [getattr(_lib.TabPolicyRun, f).offset for f in fields]
    assert _lib.TabPolicyRun.run.offset == 0      # (a run struct's fillers fill the head in place)


A, W = tc.HostArrays(), None
REFUSALS = [
    # world (states, actions, distributions), changes, status, a piece of the message
    ((16, 4, False), dict(run__q=None), 'E_ARG', 'q and inst are required'),
    ((16, 4, False), dict(run__inst=None), 'E_ARG', 'q and inst are required'),
    ((16, 4, False), dict(run__model=None), 'E_ARG', 'Dyna-Q needs the model table'),
    ((16, 4, False), dict(policy=0), 'E_ARG', 'unknown policy 0'),
    ((16, 4, False), dict(policy=4), 'E_ARG', 'unknown policy 4'),
    ((16, 4, False), dict(policy_param=0.0), 'E_ARG', 'beta 0 is not positive'),
    ((16, 4, False), dict(policy_param=-1.0), 'E_ARG', 'beta -1 is not positive'),
    ((16, 4, False), dict(policy=2, policy_param=1.5), 'E_ARG', 'epsilon 1.5 outside'),
    ((16, 4, False), dict(policy=2, policy_param=-0.1), 'E_ARG', 'epsilon -0.1 outside'),
    ((16, 4, False), dict(policy_params=A.params.ctypes.data), 'E_ARG',
     'policy_params given without param_index'),
    ((16, 4, False), dict(run__param_index=A.index.ctypes.data), 'E_ARG',
     'param_index given without parameter sets'),
    ((16, 4, False), dict(run__flags=1 | 8), 'E_ARG', 'mask_actions set without an action mask'),
    ((16, 9, False), dict(run__agent=0), 'E_UNSUPPORTED', '9 actions (a Softmax run serves 1 to 8)'),
    ((1025, 4, False), {}, 'E_UNSUPPORTED', '1025 states (a Softmax run serves 1 to 1024)'),
    ((16, 4, False), dict(run__batch=63), 'E_UNSUPPORTED', 'batch 63 (a Softmax run serves 0 to 62)'),
    ((16, 4, False), dict(run__flags=1 | 4), 'E_UNSUPPORTED', 'episodic replay'),
    ((16, 4, True), {}, 'E_UNSUPPORTED', 'rows are distributions'),
    ((16385, 4, False), dict(run__agent=0, run__replay_log=A.log.ctypes.data, run__log_cap=8),
     'E_UNSUPPORTED', 'two words per entry'),
]


@pytest.mark.parametrize('world,changes,status,message', REFUSALS,
                         ids=['%d-%s' % (k, '-'.join(r[1]) or 'world') for k, r in enumerate(REFUSALS)])
def test_refusals_come_before_any_device_call(world, changes, status, message):
    """Both entry points, a world handle that names no device: the status and the message are the
    argument checks' (a check that reached the runtime would answer COBEL_E_HIP here)."""
    from cobel_amd import _lib
    lib = _lib.lib()
    fake = tc.fake_world(world[0], world[1], A.index.ctypes.data if world[2] else None)
    pr = tc.fill_policy_run(_lib, A, **changes)
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    for call in (lambda: lib.cobel_tab_policy_run(C.addressof(fake), C.byref(pr), None),
                 lambda: lib.cobel_tab_policy_plan(C.addressof(fake), C.byref(pr), C.byref(out))):
        assert call() == getattr(_lib, status)
        assert message in lib.cobel_last_error().decode()
    assert list(out) == [0, 0, 0, 0]
    want = {'E_ARG': AssertionError, 'E_UNSUPPORTED': NotImplementedError}[status]
    with pytest.raises(want):
        _lib.check(lib.cobel_tab_policy_run(C.addressof(fake), C.byref(pr), None))


def test_refusals_of_the_single_call_form():
    from cobel_amd import _lib
    lib = _lib.lib()
    v, u, par, k = A.q.ctypes.data, A.params.ctypes.data, A.params.ctypes.data, A.model.ctypes.data
    sel = lib.cobel_policy_select_n
    assert sel(0, v, None, u, None, par, 1, None, None, 4, 4, None) == _lib.E_ARG
    assert 'unknown policy 0' in lib.cobel_last_error().decode()
    assert sel(_lib.POLICY_SOFTMAX, v, None, u, None, par, 1, None, None, 4, 9, None) == _lib.E_UNSUPPORTED
    assert '9 actions (1 to 8)' in lib.cobel_last_error().decode()
    assert sel(_lib.POLICY_SOFTMAX, v, None, u, None, par, 1, None, None, -1, 4, None) == _lib.E_RANGE
    assert sel(_lib.POLICY_SOFTMAX, None, None, u, None, par, 1, None, None, 4, 4, None) == _lib.E_ARG
    assert sel(_lib.POLICY_EXCLUSIVE, v, None, None, None, par, 1, None, None, 4, 4, None) == _lib.E_ARG
    assert sel(_lib.POLICY_RANDOM, None, None, None, None, None, 0, None, None, 4, 4, None) == _lib.E_ARG
    assert 'RandomDiscrete takes the draws k' in lib.cobel_last_error().decode()
    assert sel(_lib.POLICY_SOFTMAX, v, None, u, None, par, 3, None, None, 4, 4, None) == _lib.E_ARG
    assert 'n_param = 3' in lib.cobel_last_error().decode()
    assert sel(_lib.POLICY_RANDOM, None, None, None, k + 4, None, 0, None, None, 4, 4, None) == _lib.E_ARG
    assert sel(_lib.POLICY_RANDOM, None, None, None, None, None, 0, None, None, 0, 4, None) == _lib.OK


# -- the Python surface ----------------------------------------------------------------------------------------
def test_policy_classes_keep_the_references_assertions():
    from cobel_amd.policy import ExclusiveEpsilonGreedy, RandomDiscrete, Softmax
    with pytest.raises(AssertionError, match='at least one action'):
        RandomDiscrete(0)
    with pytest.raises(AssertionError):
        ExclusiveEpsilonGreedy(1.5)
    with pytest.raises(AssertionError):
        Softmax(0.0)
    assert np.array_equal(RandomDiscrete(5).get_action_probs(np.zeros(5)), np.full(5, 0.2))
    e = ExclusiveEpsilonGreedy(np.array([0.1, 0.2]))
    assert np.array_equal(e.parameter_column(2), [0.1, 0.2])
    with pytest.raises(AssertionError, match='one value per instance'):
        e.parameter_column(3)


def test_other_policy_types_are_refused_by_name():
    from cobel_amd.agent import QAgent
    from cobel_amd.agent.tabular import TabularAgent
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete

    class Other(EpsilonGreedy):
        pass
    ag = QAgent(Discrete(16), Discrete(4), Other(0.1))
    with pytest.raises(NotImplementedError, match='EpsilonGreedy, Softmax, ExclusiveEpsilonGreedy or '
                                                  'RandomDiscrete; got Other'):
        TabularAgent._launch(ag, None, ag.policy, 0, 1, 1, 0, 0)
    with pytest.raises(NotImplementedError, match='rollout records sessions that select with '
                                                  'EpsilonGreedy'):
        ag.rollout(type('Env', (), {})(), 2, 5)
