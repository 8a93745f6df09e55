"""Host logic of the Rescorla-Wagner feature: constructors and attributes, the policies'
probabilities, the compilation of schedules into tables, the refusals, and the agreement of
header, ctypes and library on the new exports."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rw_common as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_rw_plan', 'cobel_rw_run', 'cobel_rw_predict', 'cobel_seq_step', 'cobel_seq_reset')
E = inspect.Parameter.empty


def params(fn):
    return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def host_sequence(trials, obs, nb_actions=1, overwrite=False, **kw):
    from cobel_amd.interface import Sequence
    from cobel_amd.spaces import Box
    shape = np.asarray(next(iter(obs.values()))).shape
    return Sequence(trials, obs, Box(0.0, 1.0, shape), nb_actions, overwrite, device='cpu', seed=1,
                    **kw)


# -- constructors -----------------------------------------------------------------------------------
def test_policy_constructors_assertions_and_attributes():
    """policy/scalar.py:42-50, 131-149, 238-254."""
    from cobel_amd.policy import Proportional, Sigmoid, Threshold
    assert params(Proportional.__init__) == [('value_max', 1.0), ('code_reverse', True), ('rng', None)]
    assert params(Threshold.__init__) == [('threshold', 0.5), ('window', 0.0), ('value_max', 1.0),
                                          ('code_reverse', True), ('rng', None)]
    assert params(Sigmoid.__init__) == [('threshold', 0.5), ('scale', 10.0), ('value_max', 1.0),
                                        ('code_reverse', True), ('rng', None)]
    t = Threshold(0.4, 0.2, 2.0, False)
    assert (t.threshold, t.window, t.value_max, t.code_reverse) == (0.4, 0.1, 2.0, False)
    s = Sigmoid(0.3, 2.0)
    assert (s.threshold, s.scale, s.value_max, s.code_reverse) == (0.3, 2.0, 1.0, True)
    with pytest.raises(AssertionError, match='Threshold must lie within'):
        Threshold(1.5)
    with pytest.raises(AssertionError, match='window for random actions'):
        Threshold(0.1, 0.4)
    with pytest.raises(AssertionError, match='Threshold must lie within'):
        Sigmoid(-0.1)
    with pytest.raises(AssertionError, match='non-negative'):
        Sigmoid(0.5, -1.0)
    # sweeps: a float parameter per instance, one row each for the kernel
    rows = Sigmoid(np.array([0.2, 0.4, 0.6]), 2.0).parameter_rows(3)
    assert rows.shape == (3, 4) and rows[:, 0].tolist() == [0.2, 0.4, 0.6] and (rows[:, 2] == 2.0).all()
    assert Threshold(0.4, 0.2).parameter_rows(7).tolist() == [[0.4, 0.1, 0.0, 1.0]]
    with pytest.raises(AssertionError, match='one entry per environment instance'):
        Sigmoid(np.array([0.2, 0.4])).parameter_rows(3)


def test_action_probabilities_are_the_reference_s(golden):
    from cobel_amd.policy import Proportional, Sigmoid, Threshold
    Z = golden('rw_traces')
    values = Z['probs/values']
    for name, make in (('proportional', lambda cr: Proportional(1.5, cr)),
                       ('threshold', lambda cr: Threshold(0.5, 0.2, 1.25, cr)),
                       ('sigmoid', lambda cr: Sigmoid(0.4, 3.0, 1.25, cr))):
        for cr in (True, False):
            pol = make(cr)
            got = np.array([pol.get_action_probs(np.float64(v)) for v in values])
            assert np.array_equal(got, Z['probs/%s_%d' % (name, cr)]), (name, cr)


def test_agent_constructors_and_attributes():
    """agent/rw.py:56-74, 253-265."""
    from cobel_amd.agent import BinaryRescorlaWagner, RescorlaWagner
    from cobel_amd.policy import EpsilonGreedy, Sigmoid
    from cobel_amd.spaces import Box, Discrete
    assert params(RescorlaWagner.__init__) == [('observation_space', E), ('learning_rate', 0.9),
                                               ('custom_callbacks', None)]
    assert params(BinaryRescorlaWagner.__init__) == [
        ('observation_space', E), ('policy', E), ('policy_test', None), ('learning_rate', 0.9),
        ('custom_callbacks', None)]
    for cls in (RescorlaWagner, BinaryRescorlaWagner):
        for name in ('train', 'test'):
            assert params(getattr(cls, name)) == [('interface', E), ('trials', E), ('steps', 32)]
    ag = RescorlaWagner(Box(0.0, 1.0, (4,)))
    assert ag.W.shape == (4,) and not ag.W.any() and ag.learning_rate == 0.9
    assert ag.current_trial == 0 and ag.stop is False
    ag.W.fill(0.5)
    assert ag.W.tolist() == [0.5] * 4
    assert np.array_equal(RescorlaWagner(Box(0.0, 1.0, (3,)), (0.5, 0.1, 0.9)).learning_rate,
                          np.array((0.5, 0.1, 0.9)))
    pol = Sigmoid()
    b = BinaryRescorlaWagner(Box(0.0, 1.0, (4,)), pol)
    assert b.policy is pol and b.policy_test is pol and int(b.action_space.n) == 2
    with pytest.raises(AssertionError, match='Wrong observation space!'):
        RescorlaWagner(Discrete(4))
    with pytest.raises(AssertionError, match='scalar policies'):
        BinaryRescorlaWagner(Box(0.0, 1.0, (4,)), EpsilonGreedy(0.1))


def test_weights_tensor_takes_numpy_s_fill():
    import torch
    from cobel_amd.agent.rw import Weights
    w = torch.zeros((3, 4), dtype=torch.float64).as_subclass(Weights)
    w.fill(0.5)
    assert w.tolist() == [[0.5] * 4] * 3 and w.data_ptr() != 0


def test_typing_names():
    from cobel_amd.typing import Trial, TrialStep
    step: TrialStep = {'observation': 'A', 'reward': 1.0, 'action': None}
    trial: Trial = [step]
    assert set(TrialStep.__annotations__) == {'observation', 'reward', 'action'} and trial


# -- schedules ----------------------------------------------------------------------------------
def test_schedules_compile_to_tables():
    obs = {'A': np.array([[1.0, 0.0], [0.0, 0.0]]), 'B': np.array([[0.0, 0.5], [0.0, 2.0]])}
    st = rc._step
    s0 = [[st('A', 1.0), st('B', np.array([0.25, 0.75]), 1)], [st('B', 0.0)]]
    s1 = [[st('B', -1.0)], [st('A', 0.5), st('A', 0.5), st('B', np.array([1.0, 2.0]), 0)]]
    env = host_sequence([s0, s1], obs, 2, True, n_envs=5)
    t = env.tables
    assert t['obs_table'].dtype == np.float64 and t['obs_table'].tolist() == [
        [0.0] * 4, [1.0, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 2.0]]
    assert t['step_obs'].tolist() == [1, 2, 2, 2, 1, 1, 2]
    assert t['step_action'].tolist() == [-1, 1, -1, -1, -1, -1, 0]
    assert t['step_scalar'].tolist() == [1, 0, 1, 1, 1, 1, 0]
    assert t['step_reward'].tolist() == [[1.0, 0.0], [0.25, 0.75], [0.0, 0.0], [-1.0, 0.0],
                                         [0.5, 0.0], [0.5, 0.0], [1.0, 2.0]]
    assert t['trial_off'].tolist() == [[0, 2, 3], [3, 4, 7]]
    assert env.schedule_of.tolist() == [0, 1, 0, 1, 0] and env.has_array_rewards
    assert (env.dim, env.n_trials, int(env.action_space.n)) == (4, 2, 2)
    assert env.current_observation.shape == (5, 2, 2) and not env.current_observation.any()
    assert host_sequence(s0, obs, 2, True).current_observation.shape == (2, 2)
    assert host_sequence([s0, s1], obs, 2, True, n_envs=3, schedule_of=[1, 1, 0]).schedule_of.tolist() \
        == [1, 1, 0]
    with pytest.raises(AssertionError, match='same number of trials'):
        host_sequence([s0, s1[:1]], obs, 2, True)
    with pytest.raises(AssertionError, match='needs its action'):
        host_sequence([[st('A', np.array([0.0, 1.0]))]], obs, 2, True)
    with pytest.raises(ValueError, match='one entry per action'):
        host_sequence([[st('A', np.array([0.0, 1.0, 2.0]))]], obs, 2)
    with pytest.raises(KeyError):
        host_sequence([[st('C', 1.0)]], obs)


def test_index_error_before_a_launch():
    """The position depends on the schedules and the caps alone: the host follows it and raises
    what the reference raises at the reset past the last trial — before anything is launched
    (the Sequence here lives on the host: a launch would fail differently)."""
    from cobel_amd.agent import RescorlaWagner
    obs = {n: np.eye(3)[i] for i, n in enumerate('ABC')}
    st = rc._step
    short = [[st('A', 1.0)], [st('B', 0.0), st('C', 1.0)], [st('A', 0.0)]]
    long = [[st('A', 1.0), st('A', 1.0), st('B', 1.0)], [st('B', 0.0)], [st('A', 0.0)]]
    env = host_sequence([short, long], obs, n_envs=4)
    tr, cs = env.plan_session(3, 2)
    assert tr.tolist() == [3, 0, 3, 0] and cs.tolist() == [1, 2, 1, 2]     # `long` is cut and replayed
    tr, cs = env.plan_session(3, 3)
    assert tr.tolist() == [3, 3, 3, 3]
    with pytest.raises(IndexError, match='past the last of the 3 trials'):
        env.plan_session(4, 3)
    env.plan_session(4, 1)      # trial 1 of `short` has two steps: the cap holds instance 0 back
    ag = RescorlaWagner(env.observation_space)
    with pytest.raises(IndexError, match='list index out of range'):
        ag.train(env, 4, 3)
    assert ag.n_envs is None and ag.current_trial == 0 and not env._h_trial.any()
    env.commit_session(2, 3)
    assert env._h_trial.tolist() == [2, 2, 2, 2] and env._h_step.tolist() == [2, 1, 2, 1]
    with pytest.raises(IndexError):
        ag.test(env, 2, 3)


def test_refusals_name_the_limit():
    from cobel_amd import _lib
    from cobel_amd.agent import BinaryRescorlaWagner, RescorlaWagner
    from cobel_amd.interface import Sequence
    from cobel_amd.policy import Sigmoid
    from cobel_amd.spaces import Box, Dict, Discrete
    st = rc._step
    assert _lib.RW_MAX_DIM == 64
    big = {'A': np.zeros((5, 13))}
    with pytest.raises(NotImplementedError, match='65 components — this version serves Box '
                                                  'observations of 1 to 64 components'):
        Sequence([[st('A', 1.0)]], big, Box(0.0, 1.0, (5, 13)), device='cpu')
    with pytest.raises(NotImplementedError, match='Sequence: Dict observation spaces — this version '
                                                  'serves Box observation spaces'):
        Sequence([[st('A', 1.0)]], {'A': {'x': np.zeros(2)}}, Dict({'x': Box(0.0, 1.0, (2,))}),
                 device='cpu')
    with pytest.raises(NotImplementedError, match='Sequence: Discrete observation spaces'):
        Sequence([[st('A', 1.0)]], {'A': 0}, Discrete(3), device='cpu')
    with pytest.raises(NotImplementedError, match='RescorlaWagner: observations of 65 components — '
                                                  'this version serves 1 to 64 components'):
        RescorlaWagner(Box(0.0, 1.0, (65,)))
    with pytest.raises(NotImplementedError, match='BinaryRescorlaWagner: observations of 80'):
        BinaryRescorlaWagner(Box(0.0, 1.0, (8, 10)), Sigmoid())
    obs = {n: np.eye(2)[i] for i, n in enumerate('AB')}
    arr = [[st('A', np.array([0.0, 1.0]), 1)], [st('B', 1.0)]]
    with pytest.raises(NotImplementedError, match=r'array rewards and overwrite=False — the '
                                                  r'reference would index the reward with int\(value\)'):
        RescorlaWagner(Box(0.0, 1.0, (2,))).train(host_sequence(arr, obs, 2, False), 1)
    with pytest.raises(NotImplementedError, match=r'BinaryRescorlaWagner: the Sequence has array '
                                                  r'rewards — the reference asserts type\(reward\) is float'):
        BinaryRescorlaWagner(Box(0.0, 1.0, (2,)), Sigmoid()).train(host_sequence(arr, obs, 2, True), 1)
    with pytest.raises(NotImplementedError, match='the selection happens inside the kernel'):
        Sigmoid().select_action(0.5)
    with pytest.raises(_lib.CobelHipError, match='built on the host'):
        host_sequence(arr, obs, 2, True).reset()


def test_library_refuses_before_touching_the_device():
    from cobel_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 4)()
    with pytest.raises(NotImplementedError, match='65 components'):
        _lib.check(lib.cobel_rw_plan(65, 10, C.byref(out)))
    for dim, n, want in ((1, 1, [1, 64, 256, 1]), (3, 7, [4, 16, 64, 1]), (5, 65, [8, 8, 32, 3]),
                         (33, 65, [64, 1, 4, 17]), (64, 1, [64, 1, 4, 1]), (4, 65536, [4, 16, 64, 1024]),
                         (4, 0, [4, 16, 64, 0])):
        _lib.check(lib.cobel_rw_plan(dim, n, C.byref(out)))
        assert list(out) == want, (dim, n)
    dummy = np.zeros(8)
    with pytest.raises(NotImplementedError, match='65 components'):
        _lib.check(lib.cobel_rw_predict(_lib.ptr(dummy), 1, 65, _lib.ptr(dummy), 1, _lib.ptr(dummy), None))
    seq = _lib.Seq()
    for k in ('obs_table', 'step_obs', 'step_action', 'step_scalar', 'step_reward', 'trial_off',
              'cur_trial', 'cur_step'):
        setattr(seq, k, _lib.ptr(dummy))
    seq.n, seq.dim, seq.n_obs, seq.n_actions, seq.n_schedules, seq.n_trials, seq.n_steps = 1, 65, 2, 1, 1, 1, 1
    with pytest.raises(NotImplementedError, match='a Sequence serves 1 to 64'):
        _lib.check(lib.cobel_seq_reset(C.byref(seq), _lib.ptr(dummy), None))
    seq.dim = 4
    run = _lib.RWRun()
    with pytest.raises(AssertionError, match='W, lr, mid and trew are required'):
        _lib.check(lib.cobel_rw_run(C.byref(seq), C.byref(run), None))


def test_exports_agree(tmp_path):
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    assert lib.cobel_abi_version() == 1017
    for name in NEW:
        m = re.search(r'COBEL_API\s+int\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert name in _lib.EXPORTS
        getattr(lib, name)
        assert len(m.group(1).split(',')) == len(_lib._SIGNATURES[name][1]), name
    assert re.search(r'#define COBEL_RW_MAX_DIM %d\b' % _lib.RW_MAX_DIM, header)
    for k, name in enumerate(('NONE', 'PROPORTIONAL', 'THRESHOLD', 'SIGMOID')):
        assert re.search(r'#define COBEL_RW_POLICY_%s %d\b' % (name, k), header)
        assert getattr(_lib, 'RW_POLICY_' + name) == k
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc is not None, 'no C compiler'
    fields = [('cobel_seq_t', 'Seq', f) for f, _ in _lib.Seq._fields_] + \
        [('cobel_rw_run_t', 'RWRun', f) for f, _ in _lib.RWRun._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(cobel_seq_t), sizeof(cobel_rw_run_t));\n'
                   + ''.join('printf("%%zu\\n", offsetof(%s, %s));\n' % (t, f) for t, _, f in fields)
                   + 'return 0; }\n')
    exe = tmp_path / 's'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [C.sizeof(_lib.Seq), C.sizeof(_lib.RWRun)]
    assert got[2:] == [getattr(getattr(_lib, cls), f).offset for _, cls, f in fields]
