"""Host side of the Dyna-Q calls between sessions (no GPU): the new exports are declared in the
header, bound with the documented signatures and exported by the library; the rule by which
``DynaQ.update_q`` picks its arithmetic."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ('cobel_dynaq_replay', 'cobel_dynaq_replay_plan', 'cobel_dynaq_update', 'cobel_model_store')


def test_new_exports_are_declared_bound_and_exported():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS and re.search(r'\bT %s\b' % name, out), name
        assert getattr(lib, name).restype is C.c_int
    P, run = C.c_void_p, C.POINTER(_lib.TabRun)
    assert lib.cobel_dynaq_replay.argtypes == [P, run, C.c_int32, P]
    assert lib.cobel_dynaq_replay_plan.argtypes == [P, run, C.c_int32, C.POINTER(C.c_int32 * 4)]
    assert lib.cobel_dynaq_update.argtypes == [P, run, P, C.c_uint32, P, P]
    assert lib.cobel_model_store.argtypes == [P, P, C.c_int32, C.c_int32, P, C.c_double, P]
    # the constants and the experience record are the header's
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %u %d %d %d %d\\n", sizeof(cobel_tab_exp_t), '
           'offsetof(cobel_tab_exp_t, reward), COBEL_F_REPLAY_LANE, COBEL_REPLAY_WAVE, '
           'COBEL_REPLAY_LANE, COBEL_UPDATE_ONLINE, COBEL_UPDATE_PLANNING);}')
    exe = '/tmp/cobel_replay_sizeof_%d' % os.getpid()
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    os.remove(exe)
    assert got == [C.sizeof(_lib.TabExp), _lib.TabExp.reward.offset, _lib.F_REPLAY_LANE,
                   _lib.REPLAY_WAVE, _lib.REPLAY_LANE, _lib.UPDATE_ONLINE, _lib.UPDATE_PLANNING]
    assert C.sizeof(_lib.TabExp) == 24
    # bad arguments are refused before any HIP call
    out4 = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.cobel_dynaq_replay(None, None, 1, None) == _lib.E_ARG
    assert lib.cobel_dynaq_replay_plan(None, None, 1, C.byref(out4)) == _lib.E_ARG
    assert list(out4) == [0, 0, 0, 0]
    assert lib.cobel_dynaq_replay_plan(None, None, 1, None) == _lib.E_ARG
    assert lib.cobel_dynaq_update(None, None, None, 0, None, None) == _lib.E_ARG
    assert lib.cobel_model_store(None, None, 1, 25, None, 0.9, None) == _lib.E_ARG


def test_update_q_infers_its_arithmetic_from_the_types():
    """Plain Python numbers for reward and terminal: online float32; anything NumPy-typed in
    either: planning; array-valued experiences: online (unless the caller says planning=True)."""
    from cobel_amd.agent.dyna_q import infer_planning

    def exp(r, t, s=3):
        return {'state': s, 'action': 1, 'reward': r, 'next_state': 4, 'terminal': t}
    for r, t in ((0.5, 1), (1, 0), (0.0, True), (2, 1.0)):
        assert infer_planning(exp(r, t)) is False, (r, t)
    for r, t in ((np.float32(0.5), 1), (np.float64(0.5), 1), (0.5, np.int64(1)),
                 (np.float32(0.5), np.int64(0)), (0.5, np.bool_(True)), (np.array(0.5), 1)):
        assert infer_planning(exp(r, t)) is True, (type(r), type(t))
    assert infer_planning(exp(np.zeros(4), np.ones(4, dtype=np.int64), np.arange(4))) is False
    assert infer_planning(exp(np.zeros(4, dtype=np.float32), 1)) is False
    assert infer_planning(exp(0.5, 1, np.arange(4))) is False
    import torch
    assert infer_planning(exp(torch.zeros(4), torch.ones(4, dtype=torch.int64))) is False


def test_experiences_are_packed_and_range_checked_on_the_host():
    import torch
    from cobel_amd.memory.dyna_q import pack_experiences
    cpu = torch.device('cpu')
    e = pack_experiences({'state': np.array([3, -1, 0]), 'action': 2, 'reward': 0.1,
                          'next_state': np.array([24, 99, 1]), 'terminal': np.array([1, 0, 5])},
                         3, 25, cpu).numpy()
    assert e.shape == (3, 6) and e.dtype == np.int32
    assert e[:, 0].tolist() == [3, -1, 0] and e[:, 1].tolist() == [2, 2, 2]
    assert e[:, 2].tolist() == [24, 99, 1] and e[:, 3].tolist() == [1, 0, 1]
    assert np.array_equal(e[:, 4].view(np.float32), np.full(3, np.float32(0.1)))
    t = pack_experiences({'state': torch.tensor([3, -1, 0]), 'action': 2, 'reward': 0.1,
                          'next_state': torch.tensor([24, 99, 1]),
                          'terminal': torch.tensor([1, 0, 5])}, 3, 25, cpu).numpy()
    assert np.array_equal(t, e)
    for bad in ({'state': 25}, {'action': 4}, {'action': -1}, {'next_state': 25},
                {'next_state': -1}):
        exp = {'state': 0, 'action': 0, 'reward': 0.0, 'next_state': 0, 'terminal': 1}
        exp.update(bad)
        with pytest.raises(IndexError):
            pack_experiences(exp, 2, 25, cpu)
    with pytest.raises(AssertionError):
        pack_experiences({'state': np.arange(3), 'action': 0, 'reward': 0.0, 'next_state': 0,
                          'terminal': 1}, 2, 25, cpu)
