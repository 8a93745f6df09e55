"""Host logic of the MFEC feature: the constructor, the limits, the agreement of header, ctypes and
library on the new exports, and the feature table."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_mfec_pairs', 'cobel_mfec_run', 'cobel_mfec_estimate')


def spaces():
    from cobel_amd.spaces import Box, Discrete
    return Box(0.0, 1.0, (20,)), Discrete(4)


def test_constructor_signature_and_defaults_are_the_reference_s():
    """agent/mfec.py:324-337."""
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    sig = inspect.signature(MFEC.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('observation_space', inspect.Parameter.empty), ('action_space', inspect.Parameter.empty),
        ('policy', inspect.Parameter.empty), ('policy_test', None), ('capacity', 2000), ('k', 3),
        ('gamma', 0.97), ('model', None), ('projection_size', 256), ('custom_callbacks', None),
        ('rng', None)]
    for name in ('train', 'test'):
        s = inspect.signature(getattr(MFEC, name))
        assert [(p.name, p.default) for p in list(s.parameters.values())[1:]] == [
            ('interface', inspect.Parameter.empty), ('trials', inspect.Parameter.empty), ('steps', 32)]
    box, act = spaces()
    pol = EpsilonGreedy(0.1)
    ag = MFEC(box, act, pol, rng=np.random.default_rng(3))
    assert (ag.capacity, ag.k, ag.gamma, ag.projection_size, ag.nb_actions) == (2000, 3, 0.97, 256, 4)
    assert ag.policy is pol and ag.policy_test is pol and ag.model is None
    assert np.array_equal(ag.projection, np.random.default_rng(3).random((20, 256)))
    assert len(ag.Q.buffers) == 4 and all(len(b) == 0 for b in ag.Q.buffers) and ag.Q.k == 3
    with pytest.raises(AssertionError):
        MFEC(box, box, pol)


def test_dict_spaces_take_the_sum_of_their_components():
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Dict, Discrete
    space = Dict({'1': Box(0.0, 1.0, (6,)), '2': Box(0.0, 1.0, (2, 3))})
    ag = MFEC(space, Discrete(6), EpsilonGreedy(0.1), projection_size=16, rng=np.random.default_rng(0))
    assert ag.projection.shape == (12, 16)
    obs = {'1': np.arange(6.0), '2': np.arange(6.0) + 1}
    assert np.array_equal(ag.process_observation(obs),
                          np.dot(np.array(list(obs.values())).flatten(), ag.projection))


def test_limits_raise_not_implemented_naming_the_limit():
    from cobel_amd import _lib
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    box, act = spaces()
    pol = EpsilonGreedy(0.1)
    with pytest.raises(NotImplementedError, match='capacity of 1 to %d' % _lib.MFEC_MAX_CAPACITY):
        MFEC(box, act, pol, capacity=_lib.MFEC_MAX_CAPACITY + 1)
    with pytest.raises(NotImplementedError, match='capacity'):
        MFEC(box, act, pol, capacity=0)
    with pytest.raises(NotImplementedError, match='k of 1 to %d' % _lib.MFEC_MAX_K):
        MFEC(box, act, pol, k=_lib.MFEC_MAX_K + 1)
    with pytest.raises(NotImplementedError, match='1 to %d actions' % _lib.MFEC_MAX_ACTIONS):
        MFEC(box, Discrete(_lib.MFEC_MAX_ACTIONS + 1), pol)
    MFEC(box, Discrete(_lib.MFEC_MAX_ACTIONS), pol, capacity=_lib.MFEC_MAX_CAPACITY,
         k=_lib.MFEC_MAX_K)
    assert _lib.MFEC_MAX_CAPACITY >= 2000 and _lib.MFEC_MAX_STATES >= 1024


def test_library_limits_raise_without_a_device():
    """The entry points refuse what they do not serve before touching the device."""
    from cobel_amd import _lib
    lib = _lib.lib()
    dummy = np.zeros(8)
    for S, D, what in ((_lib.MFEC_MAX_STATES + 1, 4, 'states'), (4, _lib.MFEC_MAX_FEATURES + 1, 'features')):
        with pytest.raises(NotImplementedError, match=what):
            _lib.check(lib.cobel_mfec_pairs(_lib.ptr(dummy), S, D, _lib.ptr(dummy), _lib.ptr(dummy),
                                            None))
    mem = _lib.MFECMem()
    for p in ('rdist', 'same', 'ids', 'values', 'times', 'len', 'clock'):
        setattr(mem, p, _lib.ptr(dummy))
    mem.n, mem.n_states, mem.n_actions, mem.capacity, mem.k = 1, 4, 4, 10, 3
    for field, value, what in (('n_states', _lib.MFEC_MAX_STATES + 1, 'states'),
                               ('n_actions', _lib.MFEC_MAX_ACTIONS + 1, 'actions'),
                               ('capacity', _lib.MFEC_MAX_CAPACITY + 1, 'capacity'),
                               ('k', _lib.MFEC_MAX_K + 1, 'k = ')):
        keep = getattr(mem, field)
        setattr(mem, field, value)
        with pytest.raises(NotImplementedError, match=what):
            _lib.check(lib.cobel_mfec_estimate(C.byref(mem), _lib.ptr(dummy), 1, _lib.ptr(dummy), None))
        setattr(mem, field, keep)


def test_exports_agree(tmp_path):
    from cobel_amd import _lib
    import shutil
    import subprocess
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS
        getattr(lib, name)
    for macro, value in (('STATES', _lib.MFEC_MAX_STATES), ('ACTIONS', _lib.MFEC_MAX_ACTIONS),
                         ('CAPACITY', _lib.MFEC_MAX_CAPACITY), ('K', _lib.MFEC_MAX_K),
                         ('FEATURES', _lib.MFEC_MAX_FEATURES)):
        assert re.search(r'#define COBEL_MFEC_MAX_%s %d\b' % (macro, value), header), macro
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc is not None, 'no C compiler'
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(cobel_mfec_mem_t), sizeof(cobel_mfec_run_t), '
                   'offsetof(cobel_mfec_run_t, gamma), offsetof(cobel_mfec_mem_t, n));\nreturn 0; }\n')
    exe = tmp_path / 's'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.MFECMem), C.sizeof(_lib.MFECRun), _lib.MFECRun.gamma.offset,
                     _lib.MFECMem.n.offset]


class _Graph:
    """What feature_table reads of a Topology."""

    def __init__(self, observations=None):
        from cobel_amd.interface.simulator.offline import OfflineSimulator
        from cobel_amd.misc.topology_tools import linear_track
        self.nodes, _ = linear_track(5, 2, 1.0, 20.0, 'right')
        self.ids = list(self.nodes)
        self.pose = np.array([self.nodes[k]['pose'] for k in self.ids], dtype=np.float64)
        self.simulator = None
        if observations is not None:
            obs = {tuple(self.nodes[k]['pose']): observations(i, self.nodes[k]['pose'])
                   for i, k in enumerate(self.ids)}
            self.simulator = OfflineSimulator(obs, None)


@pytest.mark.parametrize('kind', ['pose', 'onehot', 'dict', 'float32'])
def test_feature_table_is_np_dot_row_by_row(kind):
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Dict, Discrete
    S = 10
    if kind == 'pose':
        g, space = _Graph(), Box(0.0, 1.0, (6,))
    elif kind == 'onehot':
        g, space = _Graph(lambda i, p: np.eye(S)[i]), Box(0.0, 1.0, (S,))
    elif kind == 'float32':
        g = _Graph(lambda i, p: (np.arange(12).reshape(3, 4) * 0.37 + i).astype(np.float32))
        space = Box(0.0, 1.0, (3, 4))
    else:
        g = _Graph(lambda i, p: {'1': np.array(p), '2': np.array(p) * 0.5})
        space = Dict({'1': Box(0.0, 1.0, (6,)), '2': Box(0.0, 1.0, (6,))})
    ag = MFEC(space, Discrete(4), EpsilonGreedy(0.1), projection_size=16,
              rng=np.random.default_rng(7))
    F = ag.feature_table(g)
    assert F.shape == (S, 16) and F.dtype == np.float64
    for i, o in enumerate(ag.node_observations(g)):
        flat = np.array(list(o.values())).flatten() if kind == 'dict' else o.flatten()
        assert np.array_equal(F[i], np.dot(flat, ag.projection))


def test_feature_table_from_a_model_is_one_prediction_per_node():
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete

    class Model:
        calls = 0

        def predict_on_batch(self, batch):
            Model.calls += 1
            assert batch.shape == (1, 6)
            return np.tanh(batch * 0.1) + 1.0

    g = _Graph()
    ag = MFEC(Box(0.0, 1.0, (6,)), Discrete(4), EpsilonGreedy(0.1), model=Model())
    F = ag.feature_table(g)
    assert Model.calls == 10 and np.array_equal(F, np.tanh(g.pose * 0.1) + 1.0)
