"""Host logic of the AssociativeNetwork feature: constructor and attributes, the refusals, the
test()-uses-policy convention, the agreement of header, ctypes and library on the new exports, and
the argument checks of the entry points."""
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
import anet_common as ac  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_anet_plan', 'cobel_anet_run', 'cobel_anet_predict', 'cobel_anet_update')
E = inspect.Parameter.empty


def params(fn):
    return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def make(dim=2, actions=3, **kw):
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    return AssociativeNetwork(Box(0.0, 1.0, (dim,)), Discrete(actions), EpsilonGreedy(0.1), **kw)


def test_constructor_and_attributes():
    """agent/anet.py:99-179."""
    from cobel_amd.agent import Agent, AssociativeNetwork
    from cobel_amd.agent.agent import FusedAgent
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    assert params(AssociativeNetwork.__init__) == [
        ('observation_space', E), ('action_space', E), ('policy', E), ('policy_test', None),
        ('saturation', 20.0), ('learning_rate', 0.01), ('noise', 1.0), ('linear_update', False),
        ('custom_callbacks', None), ('rng', None)]
    for name in ('train', 'test'):
        assert params(getattr(AssociativeNetwork, name)) == [('interface', E), ('trials', E),
                                                             ('steps', 32)]
    for name in ('rescale_weights', 'retrieve_q', 'update_q', 'predict_on_batch'):
        assert callable(getattr(AssociativeNetwork, name))
    assert issubclass(AssociativeNetwork, Agent) and not issubclass(AssociativeNetwork, FusedAgent)
    pol, pol_t = EpsilonGreedy(0.1), EpsilonGreedy(0.0)
    ag = AssociativeNetwork(Box(0.0, 1.0, (2, 3)), Discrete(4), pol, pol_t)
    assert ag.policy is pol and ag.policy_test is pol_t
    for d in (ag.weights, ag.saturation, ag.learning_rate):
        assert sorted(d) == ['excitatory', 'inhibitory']
        assert all(type(v) is np.ndarray and v.shape == (6, 3) for v in d.values())
    assert not ag.weights['excitatory'].any() and not ag.weights['inhibitory'].any()
    assert (ag.saturation['inhibitory'] == 20.0).all() and (ag.learning_rate['excitatory'] == 0.01).all()
    assert (ag.noise_amplitude, ag.linear_update, ag.alpha, ag.d_alpha) == (1.0, False, 1.0, 0.0)
    assert ag.current_trial == 0 and ag.stop is False
    same = make()
    assert same.policy_test is same.policy
    sat = {'excitatory': np.full((2, 2), 7.0), 'inhibitory': np.full((2, 2), 3.0)}
    ag = make(saturation=sat, learning_rate=0.5, noise=0.25, linear_update=True)
    assert ag.saturation is sat and (ag.learning_rate['inhibitory'] == 0.5).all()
    assert ag.noise_amplitude == 0.25 and ag.linear_update is True
    ag.rescale_weights({'excitatory': 2.0, 'inhibitory': 0.5})      # NumPy arrays until bound
    with pytest.raises(AssertionError, match='Wrong observation space!'):
        AssociativeNetwork(Discrete(4), Discrete(3), pol)
    with pytest.raises(AssertionError, match='Wrong action space!'):
        AssociativeNetwork(Box(0.0, 1.0, (2,)), Box(0.0, 1.0, (2,)), pol)


def test_refusals_name_the_limit():
    from cobel_amd import _lib
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.policy import EpsilonGreedy, Sigmoid
    from cobel_amd.spaces import Box, Discrete
    assert _lib.ANET_MAX_ACTIONS == 9
    with pytest.raises(NotImplementedError, match='AssociativeNetwork: observations of 65 components '
                                                  '— this version serves 1 to 64 components'):
        make(dim=65)
    for actions in (1, 10):
        with pytest.raises(NotImplementedError, match='AssociativeNetwork: %d actions — this version '
                                                      'serves 2 to 9 actions' % actions):
            make(actions=actions)
    make(dim=64, actions=9), make(dim=1, actions=2)
    with pytest.raises(NotImplementedError, match='a Sigmoid policy — this version serves '
                                                  'EpsilonGreedy'):
        AssociativeNetwork(Box(0.0, 1.0, (2,)), Discrete(3), Sigmoid())

    class Other(EpsilonGreedy):
        pass

    with pytest.raises(NotImplementedError, match='a Other policy'):
        AssociativeNetwork(Box(0.0, 1.0, (2,)), Discrete(3), Other(0.1))

    class NoSequence:
        pass

    with pytest.raises(NotImplementedError, match='AssociativeNetwork runs on a Sequence'):
        make().train(NoSequence(), 1)
    with pytest.raises(NotImplementedError, match='AssociativeNetwork runs on a Sequence'):
        make().test(NoSequence(), 1)


def host_sequence(trials, obs, nb_actions=1, overwrite=False, **kw):
    from cobel_amd.interface import Sequence
    from cobel_amd.spaces import Box
    shape = np.asarray(next(iter(obs.values()))).shape
    return Sequence(trials, obs, Box(0.0, 1.0, shape), nb_actions, overwrite, device='cpu', seed=1,
                    **kw)


def test_errors_before_a_launch():
    """What the reference raises — the IndexError of a reset past the last trial, of an array
    reward shorter than the agent's choice — comes before anything is launched (the Sequence here
    lives on the host: a launch would fail differently)."""
    schedule, obs, seq_actions = ac.CASES['unit']['design']()
    ag = make()
    with pytest.raises(IndexError, match='list index out of range'):
        ag.train(host_sequence(schedule, obs, seq_actions), 21, 10)
    assert ag.n_envs is None and ag.current_trial == 0
    with pytest.raises(AssertionError, match='observations of 2 components, the agent 3'):
        make(dim=3).train(host_sequence(schedule, obs, seq_actions), 1)
    with pytest.raises(IndexError, match='index 3 is out of bounds for axis 0 with size 3'):
        make(actions=5).train(host_sequence(schedule, obs, seq_actions), 1)


def test_test_selects_with_policy(monkeypatch):
    """agent/anet.py:272: test() selects with `policy`; `policy_test` is stored only."""
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    pol, pol_t = EpsilonGreedy(0.1), EpsilonGreedy(0.0)
    ag = AssociativeNetwork(Box(0.0, 1.0, (2,)), Discrete(3), pol, pol_t)
    seen = []
    monkeypatch.setattr(AssociativeNetwork, '_bind_to', lambda self, n, d: setattr(self, 'n_envs', n))
    monkeypatch.setattr(AssociativeNetwork, '_policy_in', lambda self, p, i: None)
    monkeypatch.setattr(AssociativeNetwork, '_reserve', lambda self, t: None)
    monkeypatch.setattr(AssociativeNetwork, '_launch',
                        lambda self, interface, p, learn, *a: seen.append((p, learn)))
    schedule, obs, seq_actions = ac.CASES['unit']['design']()
    env = host_sequence(schedule, obs, seq_actions, n_envs=2)
    monkeypatch.setattr(env, '_on_device', lambda: None)
    ag.train(env, 2, 10)
    ag.test(env, 2, 10)
    assert seen == [(pol, True), (pol, False)] and ag.current_trial == 4
    assert pol_t.counter is None and pol_t.stream is None


def test_library_refuses_before_touching_the_device():
    from cobel_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 4)()
    with pytest.raises(NotImplementedError, match='65 components'):
        _lib.check(lib.cobel_anet_plan(65, 3, 10, C.byref(out)))
    for actions in (1, 10):
        with pytest.raises(NotImplementedError, match='%d actions' % actions):
            _lib.check(lib.cobel_anet_plan(4, actions, 10, C.byref(out)))
    with pytest.raises(IndexError, match='n = -1'):
        _lib.check(lib.cobel_anet_plan(4, 3, -1, C.byref(out)))
    for dim, n, want in ((1, 1, [1, 64, 256, 1]), (2, 37, [2, 32, 128, 1]), (3, 7, [4, 16, 64, 1]),
                         (5, 65, [8, 8, 32, 3]), (33, 65, [64, 1, 4, 17]), (64, 3, [64, 1, 4, 1]),
                         (2, 65536, [2, 32, 128, 512]), (4, 0, [4, 16, 64, 0])):
        _lib.check(lib.cobel_anet_plan(dim, 9, n, C.byref(out)))
        assert list(out) == want, (dim, n)
    dummy = np.zeros(64)
    seq = _lib.Seq()
    for k in ('obs_table', 'step_obs', 'step_action', 'step_scalar', 'step_reward', 'trial_off',
              'cur_trial', 'cur_step'):
        setattr(seq, k, _lib.ptr(dummy))
    seq.n, seq.dim, seq.n_obs, seq.n_actions, seq.n_schedules, seq.n_trials, seq.n_steps = 2, 4, 2, 3, 1, 1, 1

    def run_of(**kw):
        run = _lib.ANetRun()
        for k in ('We', 'Wi', 'sat_e', 'sat_i', 'lr_e', 'lr_i', 'eps', 'pol_ctr', 'agent_ctr', 'mid',
                  'trew'):
            setattr(run, k, _lib.ptr(dummy))
        run.n, run.n_actions, run.sat_rows, run.lr_rows, run.eps_rows = 2, 3, 1, 2, 1
        run.steps_per_trial, run.trials = 10, 1
        for k, v in kw.items():
            setattr(run, k, v)
        return run

    def refused(exc, match, run, s=seq):
        with pytest.raises(exc, match=match):
            _lib.check(lib.cobel_anet_run(C.byref(s), C.byref(run), None))

    with pytest.raises(AssertionError, match='NULL sequence'):
        _lib.check(lib.cobel_anet_run(None, C.byref(run_of()), None))
    with pytest.raises(AssertionError, match='run, We and Wi are required'):
        _lib.check(lib.cobel_anet_run(C.byref(seq), None, None))
    refused(AssertionError, 'run, We and Wi are required', run_of(Wi=None))
    refused(AssertionError, r'run->n = 3, seq->n = 2', run_of(n=3))
    refused(NotImplementedError, '10 actions', run_of(n_actions=10))
    refused(NotImplementedError, '1 actions', run_of(n_actions=1))
    refused(AssertionError, 'sat_e, sat_i, lr_e and lr_i are required', run_of(lr_i=None))
    refused(AssertionError, r'sat_rows = 3, lr_rows = 2 \(1 or n = 2\)', run_of(sat_rows=3))
    refused(AssertionError, r'lr_rows = 0', run_of(lr_rows=0))
    refused(AssertionError, 'eps, pol_ctr, agent_ctr, mid and trew are required', run_of(agent_ctr=None))
    refused(AssertionError, r'eps_rows = 3', run_of(eps_rows=3))
    refused(IndexError, 'steps_per_trial = 0', run_of(steps_per_trial=0))
    refused(IndexError, 'trials = -1', run_of(trials=-1))
    refused(AssertionError, 'trace and trace_len go together', run_of(trace=_lib.ptr(dummy)))
    refused(AssertionError, 'misaligned weights', run_of(We=_lib.ptr(dummy) + 4))
    refused(AssertionError, 'misaligned saturation or learning rate', run_of(sat_i=_lib.ptr(dummy) + 4))
    refused(AssertionError, 'misaligned argument', run_of(trew=_lib.ptr(dummy) + 4))
    refused(AssertionError, 'misaligned argument', run_of(pol_ctr=_lib.ptr(dummy) + 2))
    wide = _lib.Seq.from_buffer_copy(seq)
    wide.dim = 65
    refused(NotImplementedError, 'a Sequence serves 1 to 64', run_of(), wide)
    # predict and update
    with pytest.raises(NotImplementedError, match='65 components'):
        _lib.check(lib.cobel_anet_predict(C.byref(run_of()), 65, _lib.ptr(dummy), 1, _lib.ptr(dummy), None))
    with pytest.raises(IndexError, match='batch of -1'):
        _lib.check(lib.cobel_anet_predict(C.byref(run_of()), 4, _lib.ptr(dummy), -1, _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match='agent_ctr must be given'):
        _lib.check(lib.cobel_anet_predict(C.byref(run_of(agent_ctr=None)), 4, _lib.ptr(dummy), 1,
                                          _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match='cobel_anet_predict: NULL argument'):
        _lib.check(lib.cobel_anet_predict(C.byref(run_of()), 4, None, 1, _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match='cobel_anet_predict: misaligned argument'):
        _lib.check(lib.cobel_anet_predict(C.byref(run_of()), 4, _lib.ptr(dummy) + 4, 1, _lib.ptr(dummy), None))
    with pytest.raises(NotImplementedError, match='0 components'):
        _lib.check(lib.cobel_anet_update(C.byref(run_of()), 0, _lib.ptr(dummy), _lib.ptr(dummy),
                                         _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match=r'lr_rows = 3'):
        _lib.check(lib.cobel_anet_update(C.byref(run_of(lr_rows=3)), 4, _lib.ptr(dummy), _lib.ptr(dummy),
                                         _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match='cobel_anet_update: NULL argument'):
        _lib.check(lib.cobel_anet_update(C.byref(run_of()), 4, _lib.ptr(dummy), None, _lib.ptr(dummy), None))
    with pytest.raises(AssertionError, match='cobel_anet_update: misaligned argument'):
        _lib.check(lib.cobel_anet_update(C.byref(run_of()), 4, _lib.ptr(dummy), _lib.ptr(dummy) + 2,
                                         _lib.ptr(dummy), None))
    # nothing to do is no error, and needs no device
    _lib.check(lib.cobel_anet_run(C.byref(seq), C.byref(run_of(trials=0)), None))
    _lib.check(lib.cobel_anet_predict(C.byref(run_of()), 4, None, 0, None, None))


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
        comment = header[:m.start()].rsplit('/*', 1)[1]
        # (the plan call replaces nothing in the reference, and its comment says so)
        cites = r'No line of the\s+\*?\s*reference corresponds' if name == 'cobel_anet_plan' \
            else r'anet\.py:\d+'
        assert re.search(cites, comment), '%s must cite the reference lines it replaces' % name
    assert re.search(r'#define COBEL_ANET_MAX_ACTIONS %d\b' % _lib.ANET_MAX_ACTIONS, header)
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc is not None, 'no C compiler'
    fields = [f for f, _ in _lib.ANetRun._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(cobel_anet_run_t));\n'
                   + ''.join('printf("%%zu\\n", offsetof(cobel_anet_run_t, %s));\n' % f for f in fields)
                   + 'return 0; }\n')
    exe = tmp_path / 's'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.ANetRun)
    assert got[1:] == [getattr(_lib.ANetRun, f).offset for f in fields]
    # every field of the header's struct is one of the ctypes struct's
    body = re.search(r'typedef struct \{((?:(?!typedef).)*)\} cobel_anet_run_t;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'(\w+)\s*[,;]', body) == fields
