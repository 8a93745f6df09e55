"""SFMAMemory's own methods, without a GPU: the NumPy restatement (oracle/sfma_loop.RefSFMAMemory,
completed by tests/sfma_memory_common.RefMemory for error modulation and ``current_action``)
reproduces the reference's recorded store / replay / random-batch scripts
(tests/golden/sfma_memory_traces.npz) bit for bit; the ABI additions keep their layout; the early
end the GPU tests rely on is what the restatement does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sfma_memory_common as mc
from conftest import SEED
from oracle.philox import STREAM_MEMORY, TapeRNG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('w55_dr_error_local', 'w67_sr_error_mod')


@pytest.fixture(scope='module')
def Z(golden):
    return golden('sfma_memory_traces')


def case(z, name):
    g = lambda k: z['%s/%s' % (name, k)]          # noqa: E731
    inst, S = [int(x) for x in g('cfg')]
    return g, inst, S, mc.loads(g('ops'))


def oracle_memory(D, S, inst, start=0):
    return mc.RefMemory(D, S, 4, TapeRNG(SEED, inst, STREAM_MEMORY, start=start, double_sub=1),
                        dtype=np.float32)


def test_fixture_covers_what_it_should(Z):
    assert sorted({k.split('/')[0] for k in Z.files}) == sorted(CASES)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'sfma_memory_traces.npz')) < 100_000
    modes, kinds = set(), set()
    for name in CASES:
        g, inst, S, ops = case(Z, name)
        stores = [tuple(op[1:3]) for op in ops if op[0] == 'store']
        assert 55 <= len(stores) <= 70
        assert max(stores.count(x) for x in stores) >= 4                 # one (s, a) repeated
        modes |= {op[2] for op in ops if op[:2] == ['set', 'mode']}
        kinds |= {(op[2] is None, op[3] is None) for op in ops if op[0] == 'replay'}
        sets = {op[1] for op in ops if op[0] == 'set'}
        assert {'deterministic', 'recency', 'decay_strength'} <= sets
        assert sets & {'error_mod', 'error_mod_local'}
        assert any(op[0] == 'random' for op in ops)
        assert len(g('replayed')) > 200
    assert len(modes) == 7 and len(kinds) == 4


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_recorded_scripts(Z, name):
    g, inst, S, ops = case(Z, name)
    got = mc.run_script(mc.OracleMemory(oracle_memory(g('D'), S, inst)), ops)
    mc.assert_same_record(got, {k: g(k) for k in mc.RECORD_KEYS}, what=name)


class PlainMemory(mc.OracleMemory):
    def store(self, s, a, r, ns, nt, td):
        self.mem.store(s, a, r, ns, nt)

    def replay(self, length, state, action):
        assert action is None
        return [[float(x) for x in e] for e in self.mem.replay(length, state)]


@pytest.mark.parametrize('name', CASES)
def test_plain_restatement_where_it_restates_the_feature(Z, name):
    """oracle/sfma_loop.RefSFMAMemory as it stands covers every call up to the first replay with
    ``current_action`` given: the first half of the stores and two replays under each mode."""
    from oracle.sfma_loop import RefSFMAMemory
    g, inst, S, ops = case(Z, name)
    cut = next(k for k, op in enumerate(ops) if op[0] == 'replay' and op[3] is not None)
    assert cut > 40 and sum(op[0] == 'replay' for op in ops[:cut]) == 14
    plain = RefSFMAMemory(g('D'), S, 4, TapeRNG(SEED, inst, STREAM_MEMORY, double_sub=1),
                          dtype=np.float32)
    got = mc.run_script(PlainMemory(plain), ops[:cut])
    want = {k: g(k)[:cut] for k in ('C', 'T', 'I', 'index')}
    want['replayed'] = g('replayed')[g('replayed')[:, 0] < cut]
    mc.assert_same_record(got, want, keys=tuple(want), what=name)


def test_generator_reruns_bit_identically(Z, tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden',
                                                        'gen_sfma_memory.py')], env=env)
    fresh = np.load(tmp_path / 'sfma_memory_traces.npz')
    assert sorted(fresh.files) == sorted(Z.files)
    for k in Z.files:
        assert fresh[k].dtype == Z[k].dtype and fresh[k].tobytes() == Z[k].tobytes(), k


def test_replay_of_a_one_state_memory_ends_after_one_reactivation():
    """Every stored experience sits at state 7: the first reactivation inhibits the state fully
    (I_step 1), every rating is zero from then on, so a replay of length 8 returns one experience."""
    from oracle import sfma_loop
    D = sfma_loop.metric_euclidean(5, 5)
    for start in (7, None):
        mem = oracle_memory(D, 25, 3)
        for a, ns in ((0, 6), (1, 2), (2, 8), (3, 12), (0, 6)):
            mem.store(7, a, 0.0, ns, 1)
        out = mem.replay(8, start)
        assert len(out) == 1 and out[0][0] == 7
        assert mem.I[7] == 1.0 and np.count_nonzero(mem.I) == 1


def test_empty_memory_raises_and_weak_memory_returns_nothing():
    from oracle import sfma_loop
    mem = oracle_memory(sfma_loop.metric_euclidean(5, 5), 25, 0)
    with pytest.raises(ValueError):
        with np.errstate(invalid='ignore'):
            mem.replay(4, None)
    mem.C_step = 1e-9
    mem.store(3, 1, 0.0, 4, 1)
    assert mem.replay(4, 3) == []


def test_memory_struct_layouts_match_the_header():
    from cobel_amd import _lib
    from cobel_amd.memory.sfma import EVENT, EXPERIENCE
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(cobel_sfma_mem_t), '
           'offsetof(cobel_sfma_mem_t, model_lr), offsetof(cobel_sfma_mem_t, seed), '
           'sizeof(cobel_sfma_exp_t), offsetof(cobel_sfma_exp_t, reward), '
           'sizeof(cobel_sfma_event_t));}')
    exe = '/tmp/cobel_sizeof_mem_%d' % os.getpid()
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    a, b, c, d, e, f = [int(x) for x in subprocess.check_output([exe]).split()]
    os.remove(exe)
    assert a == C.sizeof(_lib.SFMAMem) and b == _lib.SFMAMem.model_lr.offset
    assert c == _lib.SFMAMem.seed.offset
    assert d == C.sizeof(_lib.SFMAExp) == EXPERIENCE.itemsize == 32
    assert e == _lib.SFMAExp.reward.offset == EXPERIENCE.fields['reward'][1]
    assert f == EVENT.itemsize == _lib.SFMA_EVENT_BYTES


def test_memory_plan_follows_the_agents_plan():
    from cobel_amd import _lib
    lib = _lib.lib()
    out, ref = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    for S, flags in ((25, 0), (42, 0), (225, 0), (225, _lib.F_NO_PREFETCH), (42, _lib.F_SFMA_STREAM),
                     (1274, 0), (1275, 0), (5089, 0), (6785, 0), (16383, 0)):
        _lib.check(lib.cobel_sfma_mem_plan(S, flags, C.byref(out)))
        _lib.check(lib.cobel_sfma_plan(S, flags, C.byref(ref)))
        assert list(out)[:2] == list(ref)[:2]
        assert out[2] == (ref[2] if ref[0] == 0 else (256 if ref[2] == 256 else 1024))
    _lib.check(lib.cobel_sfma_mem_plan(5088, 0, C.byref(out)))
    assert out[3] == 3
    _lib.check(lib.cobel_sfma_mem_plan(5089, 0, C.byref(out)))
    assert out[3] == 2
    _lib.check(lib.cobel_sfma_mem_plan(6785, 0, C.byref(out)))
    assert out[3] == 0
    assert lib.cobel_sfma_mem_plan(16384, 0, C.byref(out)) == _lib.E_UNSUPPORTED
