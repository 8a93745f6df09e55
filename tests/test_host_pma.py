"""Host logic of the PMA feature: construction, the limits, attribute round trips before a device
is bound, and the agreement of header, ctypes and library on the new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pma_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_pma_plan', 'cobel_pma_replay', 'cobel_pma_trial', 'cobel_pma_store',
       'cobel_pma_update_sr')


def test_import_from_the_package_roots():
    from cobel_amd.agent import PMA
    from cobel_amd.memory import PMAMemory
    assert PMA.__name__ == 'PMA' and PMAMemory.__name__ == 'PMAMemory'


def test_exports_agree():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.cobel_abi_version() == 1017
    assert re.search(r'#define COBEL_STREAM_PMA_MEMORY %du' % _lib.STREAM_PMA_MEMORY, header)
    assert re.search(r'#define COBEL_STREAM_PMA_POLICY %du' % _lib.STREAM_PMA_POLICY, header)
    assert re.search(r'#define COBEL_PMA_MAX_STATES %d\b' % _lib.PMA_MAX_STATES, header)
    assert re.search(r'#define COBEL_PMA_MAX_ACTIONS %d\b' % _lib.PMA_MAX_ACTIONS, header)
    assert (pc.STREAM_PMA_MEMORY, pc.STREAM_PMA_POLICY) == (_lib.STREAM_PMA_MEMORY,
                                                          _lib.STREAM_PMA_POLICY)


def test_struct_sizes_match_the_header(tmp_path):
    """sizeof of the three structs as a C compiler lays out the header."""
    from cobel_amd import _lib
    import shutil
    import subprocess
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\nint main(void) {\n'
                   'printf("%zu %zu %zu\\n", sizeof(cobel_pma_mem_t), sizeof(cobel_pma_run_t), '
                   'sizeof(cobel_pma_rec_t));\nreturn 0; }\n')
    exe = tmp_path / 's'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(_lib.PMAMem), C.sizeof(_lib.PMARun), 24]


def test_plan_and_limits():
    from cobel_amd import _lib
    out = (C.c_int32 * 4)()
    assert _lib.lib().cobel_pma_plan(128, 8, 32, C.byref(out)) == _lib.OK
    assert 0 < out[0] <= 64 * 1024 and out[1] == 64 and out[3] == 256
    assert out[2] == 8 * (128 * 128 + 2 * 128)
    for S, A in ((129, 4), (25, 9)):
        assert _lib.lib().cobel_pma_plan(S, A, 32, C.byref(out)) == _lib.E_UNSUPPORTED
        msg = _lib.lib().cobel_last_error().decode()
        assert '128 states' in msg and '8 actions' in msg


def test_construction_matches_the_reference_expressions():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = pc.demo_world()
    tabs, sas = pc.tables_of(world)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99)
    ref = pc.RefPMAMemory(sas, None, gamma_q=0.99)
    assert np.array_equal(mem.T, ref.T) and np.array_equal(mem.SR, ref.SR)
    assert np.array_equal(mem.update_mask, ref.update_mask)
    assert mem.update_mask.sum() == 100 - 4            # the quirk: only state 0's entries
    assert (mem.nb_states, mem.nb_actions, mem.learning_rate_T) == (25, 4, 0.9)
    assert (mem.min_gain, mem.min_gain_mode) == (10 ** -6, 'original')
    assert mem.ignore_barriers and not (mem.equal_need or mem.equal_gain or mem.allow_loops)
    assert mem.states.dtype == np.int64 and mem.rewards.shape == (25, 4)
    # attribute round trips before a device is bound
    mem.SR = np.eye(25)
    assert np.array_equal(mem.SR, np.eye(25))
    mem.states = np.arange(100).reshape(25, 4) % 25
    mem.compute_update_mask()
    ref.states = np.arange(100).reshape(25, 4) % 25
    ref.compute_update_mask()
    assert np.array_equal(mem.update_mask, ref.update_mask)
    assert mem.flags() == 4 | 16


def test_refusal_above_the_limits_names_them():
    from cobel_amd.agent import PMA
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    with pytest.raises(NotImplementedError, match='128 states and 8 actions'):
        PMAMemory(np.zeros((129, 4, 129)), EpsilonGreedy(0.1))
    with pytest.raises(NotImplementedError, match='128 states and 8 actions'):
        PMAMemory(np.zeros((16, 9, 16)), EpsilonGreedy(0.1))
    world = pc.demo_world()
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1))
    agent = PMA(Discrete(25), Discrete(4), EpsilonGreedy(0.1), mem)
    assert agent.Q.shape == (25, 4) and agent.Q.dtype == np.float64
    assert agent.M is mem and agent.learning_rate == 0.9 and agent.gamma == 0.99
    assert not agent.mask_actions and agent.action_mask.all()
    assert np.array_equal(agent.predict_on_batch([3, 4]), np.zeros((2, 4)))
    with pytest.raises(NotImplementedError, match='128 states and 8 actions'):
        PMA(Discrete(129), Discrete(4), EpsilonGreedy(0.1), mem)
