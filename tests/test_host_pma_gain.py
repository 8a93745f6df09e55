"""CPU tests of PMAMemory's observables (csrc/pma_gain.hip): the NumPy restatement
(``RefPMAMemory.compute_gain_batch / compute_gain / update_q / _probs_batch`` of
tests/pma_common.py) against the real reference's recorded values, bit for bit; the exports; and
every refusal of the four entry points and of the Python methods that comes before a launch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pma_gain_common as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_pma_gain_batch', 'cobel_pma_gain_seq', 'cobel_pma_action_probs', 'cobel_pma_update_q')
FAKE = 0x10000           # an aligned address nobody dereferences


@pytest.fixture(scope='module')
def Z(golden):
    return golden('pma_gain')


# -- the restatement against the reference ---------------------------------------------------------
@pytest.mark.parametrize('name', list(gc.WORLDS))
def test_restatement_equals_the_reference(Z, name):
    want = {k[len(name) + 1:]: Z[k] for k in Z.files if k.startswith(name + '/')}
    gc.assert_same(gc.expected(name), want, name)


def test_action_probs_restated(Z):
    for rows in gc.PROB_ROWS:
        for A in gc.PROB_ACTIONS:
            for masked in (False, True):
                q, mask = gc.prob_case(rows, A, masked)
                want = Z['probs/%dx%d/%s' % (rows, A, gc.MASKS[masked])]
                assert want.shape == (rows, A)
                assert np.array_equal(gc.probs_restated(q, mask), want), (rows, A, masked)
                if mask is not None:
                    assert (want[~mask] == 0).all() and mask.any(axis=1).all()


def test_fixture_holds_what_the_cases_promise(Z):
    mg = 10 ** -6
    for name in gc.WORLDS:
        case = gc.build(name)
        S, A = case['S'], case['A']
        assert Z[name + '/gain_batch/plain/zero'].shape == (gc.N, A * S)
        assert (Z[name + '/gain_batch/plain/stay'] == mg).all(), 'a gain that is not clipped'
        if A > 1:
            flip = Z[name + '/gain_batch/plain/flip']
            assert (flip > 1000 * mg).any() and (flip == mg).any()
            rnd = Z[name + '/gain_batch/masked/random']
            assert not np.array_equal(rnd[0], rnd[1]) and not np.array_equal(rnd[1], rnd[2])
            assert not np.array_equal(rnd, Z[name + '/gain_batch/plain/random'])
            a, b = (Z['%s/gain_seq/%s/plain/random' % (name, m)] for m in gc.MODES)
            assert not np.array_equal(a, b), 'the two gain modes agree everywhere'
        assert Z[name + '/gain_seq/original/plain/random'].shape == (gc.N, len(gc.GAIN_SEQS))
        Q = case['Q']['random']
        for sname in ('break', 'terminal'):     # (step 0 looks ahead to the end: memory/pma.py:476-489)
            assert np.array_equal(Z['%s/update_q/%s' % (name, sname)], Q), 'a terminal step must break'
        for sname in ('len1', 'len32', 'lenmax', 'twice', 'dead1'):
            got = Z['%s/update_q/%s' % (name, sname)]
            changed = {(int(e['state']), int(e['action'])) for e in case['seqs'][sname]}
            assert 1 <= int((got[0] != Q[0]).sum()) <= len(changed), (name, sname)
        assert len(case['seqs']['lenmax']) == gc.MAX_SEQ
        assert case['seqs']['terminal'][-1]['terminal'] == 0
        assert case['seqs']['break'][1]['terminal'] == 0
        assert case['mask'].any(axis=1).all() and (A == 1 or not case['mask'].all())
    assert [gc.build(n)['S'] * gc.build(n)['A'] for n in gc.WORLDS] == [48, 100, 72, 6, 528]
    assert gc.build('wide_132')['S'] == 132 and gc.build('eight_9x8')['A'] == 8


def test_fixture_regenerates(tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_pma_gain.py')],
                          env=env)
    fresh, held = np.load(tmp_path / 'pma_gain.npz'), np.load(
        os.path.join(ROOT, 'tests', 'golden', 'pma_gain.npz'))
    assert sorted(fresh.files) == sorted(held.files)
    for k in held.files:
        assert np.array_equal(fresh[k], held[k]), k


# -- the C ABI ---------------------------------------------------------------------------------------
def test_exports_agree():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS
        getattr(lib, name)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert set(NEW) <= set(re.findall(r'\bT (cobel_\w+)', out))
    m = re.search(r'#define\s+COBEL_PMA_MAX_SEQ\s+(\d+)', header)
    assert m and int(m.group(1)) == _lib.PMA_MAX_SEQ == gc.MAX_SEQ and _lib.PMA_MAX_SEQ >= 64
    assert lib.cobel_abi_version() == 1017


def fake_mem(S=25, A=4, n=3, pow_len=300, **fields):
    from cobel_amd import _lib
    m = _lib.PMAMem()
    m.rewards = m.states = m.terminals = m.gamma_pow = m.gamma_q_pow = FAKE
    m.n, m.n_states, m.n_actions, m.pow_len = n, S, A, pow_len
    m.epsilon, m.min_gain = 0.1, 1e-6
    for k, v in fields.items():
        setattr(m, k, v)
    return m


def lengths(*values):
    return np.ascontiguousarray(values, dtype=np.int32)


def err():
    from cobel_amd import _lib
    return _lib.lib().cobel_last_error().decode()


def test_gain_batch_refuses_before_any_launch():
    """Every refusal comes before the launch: this host has no GPU, the addresses are fakes."""
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_gain_batch
    m = fake_mem()
    assert call(None, FAKE, 0, FAKE, None) == _lib.E_ARG and 'NULL mem' in err()
    assert call(C.byref(m), None, 0, FAKE, None) == _lib.E_ARG and 'NULL q' in err()
    assert call(C.byref(m), FAKE, 0, None, None) == _lib.E_ARG and 'NULL gain' in err()
    for A in (0, 9):
        bad = fake_mem(A=A)
        assert call(C.byref(bad), FAKE, 0, FAKE, None) == _lib.E_UNSUPPORTED
        assert '%d actions' % A in err() and '1 .. 8 actions' in err()
    for S in (0, 1025):
        bad = fake_mem(S=S)
        assert call(C.byref(bad), FAKE, 0, FAKE, None) == _lib.E_UNSUPPORTED
        assert '%d states' % S in err() and '1 .. 1024 states' in err()
    for stride in (1, 99, 101, -100, 200):
        assert call(C.byref(m), FAKE, stride, FAKE, None) == _lib.E_ARG
        assert 'q_stride = %d' % stride in err() and '100' in err()
    assert call(C.byref(fake_mem(n=-1)), FAKE, 0, FAKE, None) == _lib.E_RANGE and 'n = -1' in err()
    assert call(C.byref(fake_mem(rewards=None)), FAKE, 0, FAKE, None) == _lib.E_ARG
    assert 'rewards, states and terminals' in err()
    assert call(C.byref(m), FAKE + 4, 0, FAKE, None) == _lib.E_ARG and 'misaligned' in err()
    assert call(C.byref(fake_mem(epsilon=1.5)), FAKE, 0, FAKE, None) == _lib.E_ARG
    assert 'epsilon' in err()
    # nothing to do is no launch either
    assert call(C.byref(fake_mem(n=0)), FAKE, 100, FAKE, None) == _lib.OK


def test_gain_seq_refuses_before_any_launch():
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_gain_seq
    m = fake_mem()
    one = lengths(1)

    def go(mem=m, q=FAKE, stride=0, steps=FAKE, lens=one, n_seq=1, max_len=4, inst=0, gain=FAKE):
        return call(C.byref(mem) if mem is not None else None, q, stride, steps,
                    None if lens is None else lens.ctypes.data, n_seq, max_len, inst, gain, None)

    assert go(mem=None) == _lib.E_ARG and 'NULL mem' in err()
    assert go(q=None) == _lib.E_ARG and 'NULL q' in err()
    assert go(gain=None) == _lib.E_ARG and 'NULL gain' in err()
    assert go(steps=None) == _lib.E_ARG and 'steps' in err()
    assert go(lens=None) == _lib.E_ARG and 'NULL lengths' in err()
    for A in (0, 9):
        assert go(mem=fake_mem(A=A)) == _lib.E_UNSUPPORTED and '1 .. 8 actions' in err()
    for S in (0, 1025):
        assert go(mem=fake_mem(S=S)) == _lib.E_UNSUPPORTED and '1 .. 1024 states' in err()
    assert go(n_seq=-1) == _lib.E_RANGE and 'n_seq = -1' in err()
    assert go(stride=7) == _lib.E_ARG and 'q_stride = 7' in err()
    assert go(lens=lengths(0)) == _lib.E_RANGE and 'lengths[0] = 0' in err()
    assert go(lens=lengths(5)) == _lib.E_RANGE and 'lengths[0] = 5' in err() and 'max_len = 4' in err()
    assert go(lens=lengths(2, 4, 5), n_seq=3) == _lib.E_RANGE and 'lengths[2] = 5' in err()
    # per-instance lists: [N][n_seq] lengths, all of them looked at
    assert go(lens=lengths(1, 1, 1, 1, 1, 9), n_seq=2, inst=8) == _lib.E_RANGE
    assert 'lengths[5] = 9' in err()
    assert go(n_seq=2, lens=lengths(1, 1), inst=5) == _lib.E_ARG and 'inst_stride = 5' in err()
    for bad in (0, -1, _lib.PMA_MAX_SEQ + 1):
        assert go(max_len=bad) == _lib.E_UNSUPPORTED
        assert 'max_len = %d' % bad in err() and '1 .. %d steps' % _lib.PMA_MAX_SEQ in err()
    # pow_len must exceed the longest sequence
    assert go(mem=fake_mem(pow_len=4), lens=lengths(4)) == _lib.E_ARG
    assert 'hold 4 entries, 5 are needed' in err()
    assert go(mem=fake_mem(pow_len=3), lens=lengths(1, 3, 2), n_seq=3) == _lib.E_ARG
    assert 'hold 3 entries, 4 are needed' in err()
    assert go(mem=fake_mem(gamma_pow=None)) == _lib.E_ARG and 'power tables' in err()
    assert go(steps=FAKE + 4) == _lib.E_ARG and '8-byte aligned' in err()
    assert go(n_seq=0) == _lib.OK and go(mem=fake_mem(n=0)) == _lib.OK


def test_action_probs_refuses_before_any_launch():
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_action_probs
    assert call(None, None, 3, 4, 0.1, FAKE, None) == _lib.E_ARG and 'NULL q' in err()
    assert call(FAKE, None, 3, 4, 0.1, None, None) == _lib.E_ARG and 'NULL probs' in err()
    for A in (0, 9):
        assert call(FAKE, None, 3, A, 0.1, FAKE, None) == _lib.E_UNSUPPORTED
        assert '%d actions' % A in err() and '1 .. 8 actions' in err()
    assert call(FAKE, None, -1, 4, 0.1, FAKE, None) == _lib.E_RANGE and 'rows = -1' in err()
    assert call(FAKE, None, 3, 4, -0.5, FAKE, None) == _lib.E_ARG and 'epsilon' in err()
    assert call(FAKE + 4, None, 3, 4, 0.1, FAKE, None) == _lib.E_ARG and 'misaligned' in err()
    assert call(FAKE, None, 0, 4, 0.1, FAKE, None) == _lib.OK


def test_update_q_refuses_before_any_launch():
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_update_q
    m = fake_mem()
    one = lengths(1)

    def go(mem=m, q=FAKE, steps=FAKE, lens=one, max_len=4, inst=0, pows=FAKE, pow_len=300):
        return call(C.byref(mem) if mem is not None else None, q, steps,
                    None if lens is None else lens.ctypes.data, max_len, inst, 0.9, pows, pow_len,
                    None)

    assert go(mem=None) == _lib.E_ARG and 'NULL mem' in err()
    assert go(q=None) == _lib.E_ARG and 'NULL q' in err()
    assert go(steps=None) == _lib.E_ARG and 'steps' in err()
    assert go(lens=None) == _lib.E_ARG and 'NULL lengths' in err()
    assert go(pows=None) == _lib.E_ARG and 'power table' in err()
    for A in (0, 9):
        assert go(mem=fake_mem(A=A)) == _lib.E_UNSUPPORTED and '1 .. 8 actions' in err()
    for S in (0, 1025):
        assert go(mem=fake_mem(S=S)) == _lib.E_UNSUPPORTED and '1 .. 1024 states' in err()
    assert go(mem=fake_mem(n=-2)) == _lib.E_RANGE and 'n = -2' in err()
    assert go(lens=lengths(0)) == _lib.E_RANGE and 'lengths[0] = 0' in err()
    assert go(lens=lengths(5)) == _lib.E_RANGE and 'lengths[0] = 5' in err()
    assert go(lens=lengths(1, 4, 6), inst=4) == _lib.E_RANGE and 'lengths[2] = 6' in err()
    assert go(inst=3) == _lib.E_ARG and 'inst_stride = 3' in err()
    for bad in (0, _lib.PMA_MAX_SEQ + 1):
        assert go(max_len=bad) == _lib.E_UNSUPPORTED and 'max_len = %d' % bad in err()
    assert go(lens=lengths(4), pow_len=4) == _lib.E_ARG and 'holds 4 entries, 5 are needed' in err()
    assert go(lens=lengths(1, 3, 2), inst=4, pow_len=3) == _lib.E_ARG and '4 are needed' in err()
    assert go(q=FAKE + 4) == _lib.E_ARG and '8-byte aligned' in err()
    assert go(mem=fake_mem(n=0)) == _lib.OK


# -- PMAMemory ---------------------------------------------------------------------------------------
def looks_bound(n=3):
    """A memory of ``n`` instances that has its counters and no device tables: every refusal below
    comes before anything touches a device."""
    import torch
    import pma_common as pc
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(pc.small_world()['sas'], EpsilonGreedy(0.1))
    mem.n_envs, mem.counter = n, torch.zeros(n, dtype=torch.int32)
    return mem


STEP = {'state': 1, 'action': 0, 'reward': 0.5, 'next_state': 2, 'terminal': 1}


def test_the_four_methods_exist():
    from cobel_amd.memory import PMAMemory
    for name in ('compute_gain_batch', 'compute_gain', 'action_probs_batch', 'update_q'):
        assert callable(getattr(PMAMemory, name)), name
    doc = sys.modules[PMAMemory.__module__].__doc__
    assert all(name in doc for name in ('compute_gain_batch', 'action_probs_batch', 'update_q'))


def test_python_refuses_bad_updates():
    from cobel_amd import _lib
    mem = looks_bound()
    Q = np.zeros((12, 4))
    with pytest.raises(IndexError, match='without steps'):
        mem.compute_gain(Q, None, [[STEP], []])
    with pytest.raises(IndexError, match='without steps'):
        mem.update_q(np.zeros((3, 12, 4)), [])
    with pytest.raises(NotImplementedError, match='up to %d steps' % _lib.PMA_MAX_SEQ):
        mem.compute_gain(Q, None, [[STEP] * (_lib.PMA_MAX_SEQ + 1)])
    with pytest.raises(NotImplementedError, match='up to %d steps' % _lib.PMA_MAX_SEQ):
        mem.update_q(np.zeros((3, 12, 4)), [STEP] * (_lib.PMA_MAX_SEQ + 1))
    with pytest.raises(IndexError, match='state outside'):
        mem.compute_gain(Q, None, [[dict(STEP, state=12)]])
    with pytest.raises(IndexError, match='first ones'):
        mem.compute_gain(Q, None, [[dict(STEP, state=[1, -1, 1]), dict(STEP, state=[1, 1, 1])]])
    with pytest.raises(IndexError, match='at least one'):
        mem.compute_gain(Q, None, [[dict(STEP, state=[1, None, 1])]])


def test_python_refuses_a_q_function_of_the_wrong_shape():
    mem = looks_bound()
    for shape in ((12,), (4, 12), (2, 12, 4), (3, 12, 5), (48,)):
        with pytest.raises(ValueError, match=r'\[12, 4\] or \[3, 12, 4\]'):
            mem.compute_gain_batch(np.zeros(shape), None)
        with pytest.raises(ValueError, match=r'\[12, 4\] or \[3, 12, 4\]'):
            mem.compute_gain(np.zeros(shape), None, [[STEP]])
        with pytest.raises(ValueError, match=r'\[3, 12, 4\] is expected'):
            mem.update_q(np.zeros(shape), [STEP])
    with pytest.raises(ValueError, match=r'\[3, 12, 4\] is expected'):
        mem.update_q(np.zeros((12, 4)), [STEP])           # which of the three instances?
    with pytest.raises(ValueError, match=r'\[1, 12, 4\] or \[12, 4\]'):
        looks_bound(1).update_q(np.zeros((2, 12, 4)), [STEP])


def test_sequences_as_the_kernels_take_them():
    """Scalars give one list for every instance, arrays one per instance; a state of None or < 0
    ends an instance's sequence early."""
    from cobel_amd.memory.pma import RECORD
    mem = looks_bound()
    steps, lens, max_len, per = mem._sequences([[STEP, STEP], [STEP]], 'compute_gain')
    assert not per and max_len == 2 and np.array_equal(lens, [[2, 1]]) and lens.dtype == np.int32
    rec = steps.numpy().view(RECORD).reshape(1, 2, 2)
    assert rec['state'][0].tolist() == [[1, 1], [1, 0]] and rec['reward'][0, 0, 1] == 0.5
    two = [dict(STEP, state=[1, 2, 3], reward=[0.0, 1.0, 2.0]), dict(STEP, state=[4, -1, None])]
    steps, lens, max_len, per = mem._sequences([two, [STEP]], 'compute_gain')
    assert per and max_len == 2 and np.array_equal(lens, [[2, 1], [1, 1], [1, 1]])
    rec = steps.numpy().view(RECORD).reshape(3, 2, 2)
    assert rec['state'][:, 0, 0].tolist() == [1, 2, 3] and rec['state'][:, 0, 1].tolist() == [4, -1, -1]
    assert rec['reward'][:, 0, 0].tolist() == [0.0, 1.0, 2.0]
