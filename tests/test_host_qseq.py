"""CPU tests of QAgent on a Sequence: the restatement of tests/qseq_common.py against the traces
recorded from the real reference (tests/golden/qseq_traces.npz), the C ABI of csrc/qseq.hip (exports,
struct layout, every refusal before a launch) and the host side of the Python surface."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qseq_common as qc  # noqa: E402

NEW = ('cobel_qseq_plan', 'cobel_qseq_run', 'cobel_softmax_n')


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'qseq_traces.npz'))


# -- the restatement against the reference ----------------------------------------------------------
def test_the_fixture_holds_every_case_and_keeps_the_margin(Z):
    """No case and no instance is left out; every recorded draw lies at least 1e-9 away from every
    edge of the normalised CDF it was compared with."""
    assert sorted({k.split('/')[0] for k in Z.files} - {'probs'}) == sorted(qc.CASES)
    for name in qc.CASES:
        assert float(Z[name + '/margin']) > qc.MARGIN, name
    assert sorted(k.split('/')[1] for k in Z.files if k.startswith('probs/')) == sorted(qc.KAT_ROWS)


@pytest.mark.parametrize('name', sorted(qc.CASES))
def test_restatement_equals_the_reference_exactly(Z, name):
    out = qc.restate_case(name)
    assert out['margin'] > qc.MARGIN
    qc.assert_same_record(out, Z, name + '/', what=name)
    for k in qc.EXACT:
        assert name + '/' + k in Z.files and k in out, k


def test_cases_cover_what_they_are_meant_to(Z):
    assert Z['demo12/Q'].shape == (48, 5, 8) and int(Z['demo12/len_M']) == 48
    cut = Z['multistep_cut/end']
    assert cut.any() and not cut.all(), 'some trials must be cut by the cap, some must end'
    assert Z['one_action/Q'].shape[2] == 1 and Z['one_action/index'][0] == len(Z['one_action/action'])
    assert Z['three_actions/Q'].shape[2] == 3
    # B = 0 first: the log fills, the agent's generator moves by one call per step all the same
    assert Z['b0_then_b5/index'][2] == len(Z['b0_then_b5/action']) == int(Z['b0_then_b5/len_M'])
    # exact ties: the untouched zeros of the start, and equal values that were learned
    q = Z['eps_ties/Q'][-1]
    assert all(row.max() > 0 and (row == row.max()).sum() >= 2 for row in q[1:])
    # 'A' and 'A2' share a key, 'Z' shares the key of a trial's end: three keys for four names
    assert Z['shared_keys/Q'].shape[1] == 3
    assert (Z['shared_keys/M'][:, 0] == 0).any(), 'the zero observation must occur as a state'
    # test() draws from policy_test's own stream and learns nothing
    assert Z['train_test/index'][1] == 13 and int(Z['train_test/len_M']) == Z['train_test/index'][2]


def test_softmax_restatement_against_the_reference_probabilities(Z):
    """The restatement's sum runs in action order, NumPy's pairwise for eight values: equal up to the
    rounding of one sum (2^-52 relative), exact zeros and ones alike."""
    for name, (v, mask, beta) in qc.KAT_ROWS.items():
        want = Z['probs/' + name]
        got = qc.softmax_probs(v, beta, mask)
        assert got.shape == want.shape and not np.isnan(got).any(), name
        assert np.array_equal(got == 0, want == 0), name
        assert np.all(np.abs(got - want) <= 2.0 ** -52 * want), name
    hot = qc.softmax_probs(*[qc.KAT_ROWS['hot'][k] for k in (0, 2)])
    assert np.array_equal(hot == 0, [1, 1, 0, 1, 1, 0]), 'beta = 1e4 gives exact zeros'
    assert np.array_equal(qc.softmax_probs([0.7, -0.3, 0.7, 0.0], 1e4), [0.5, 0, 0.5, 0])
    assert np.array_equal(qc.softmax_probs([0.5] * 8, 1.0), [0.125] * 8)


def test_generator_reruns_bit_identically(Z, tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_qseq.py')],
                          env=env)
    fresh = np.load(tmp_path / 'qseq_traces.npz')
    assert sorted(fresh.files) == sorted(Z.files)
    for k in Z.files:
        assert fresh[k].dtype == Z[k].dtype and fresh[k].tobytes() == Z[k].tobytes(), k


# -- the C ABI --------------------------------------------------------------------------------------
def test_exports_and_struct_layout(tmp_path):
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
    for macro, value in (('MAX_ACTIONS', _lib.QSEQ_MAX_ACTIONS), ('MAX_KEYS', _lib.QSEQ_MAX_KEYS),
                         ('ROW', _lib.QSEQ_ROW), ('POLICY_SOFTMAX', _lib.QSEQ_POLICY_SOFTMAX),
                         ('POLICY_EPS_GREEDY', _lib.QSEQ_POLICY_EPS_GREEDY)):
        assert re.search(r'#define COBEL_QSEQ_%s %d\b' % (macro, value), header), macro
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc is not None, 'no C compiler'
    fields = [f for f, _ in _lib.QSeqRun._fields_]
    src = tmp_path / 'qseq.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\nprintf("%zu %zu\\n", sizeof(cobel_qseq_run_t), '
                   'sizeof(cobel_qseq_rec_t));\n'
                   + ''.join('printf("%%zu\\n", offsetof(cobel_qseq_run_t, %s));\n' % f for f in fields)
                   + 'printf("%zu\\n", offsetof(cobel_qseq_rec_t, meta));\nreturn 0; }\n')
    exe = tmp_path / 'qseq'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.QSeqRun) and got[1] == 16 and got[-1] == 8
    assert got[2:-1] == [getattr(_lib.QSeqRun, f).offset for f in fields]
    body = re.search(r'typedef struct \{((?:(?!typedef).)*)\} cobel_qseq_run_t;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'(\w+)\s*[,;]', body) == fields


def test_plan():
    from cobel_amd import _lib
    out = (C.c_int32 * 4)()
    assert _lib.lib().cobel_qseq_plan(5, 8, 2700, out) == _lib.OK
    assert list(out) == [8, 8, 32, 85]
    assert _lib.lib().cobel_qseq_plan(64, 1, 33, out) == _lib.OK and out[3] == 2
    assert _lib.lib().cobel_qseq_plan(1, 1, 0, out) == _lib.OK and out[3] == 0
    for keys, actions in ((0, 3), (65, 3), (4, 0), (4, 9)):
        assert _lib.lib().cobel_qseq_plan(keys, actions, 8, out) == _lib.E_UNSUPPORTED
    assert _lib.lib().cobel_qseq_plan(4, 3, -1, out) == _lib.E_RANGE
    assert _lib.lib().cobel_qseq_plan(4, 3, 8, None) == _lib.E_ARG


def test_every_refusal_comes_before_a_launch():
    """The structs hold made-up addresses: a call that got as far as a launch would not return one
    of these codes (trials = 0 returns OK without one)."""
    from cobel_amd import _lib
    seq, run = qc.fake_structs()
    assert qc.run_rc(seq, run) == _lib.OK
    for actions in (0, 9):
        seq, run = qc.fake_structs()
        seq.n_actions = run.n_actions = actions
        run.trials = 3
        assert qc.run_rc(seq, run) == _lib.E_UNSUPPORTED, actions
        assert b'actions' in _lib.lib().cobel_last_error()
    for keys in (0, 65):
        seq, run = qc.fake_structs()
        run.n_keys, run.trials = keys, 3
        assert qc.run_rc(seq, run) == _lib.E_UNSUPPORTED, keys
    for name in ('Q', 'key_of_row', 'par', 'pol_ctr', 'mid', 'trew', 'log', 'log_len', 'mem_ctr'):
        seq, run = qc.fake_structs()
        setattr(run, name, None)
        run.trials = 3
        assert qc.run_rc(seq, run) == _lib.E_ARG, name
    for name in ('obs_table', 'step_obs', 'step_reward', 'trial_off', 'cur_trial'):
        seq, run = qc.fake_structs()
        setattr(seq, name, None)
        run.trials = 3
        assert qc.run_rc(seq, run) == _lib.E_ARG, name
    # test() needs neither the log nor the agent's counter
    seq, run = qc.fake_structs(learn=False)
    run.log = run.log_len = run.mem_ctr = None
    assert qc.run_rc(seq, run) == _lib.OK
    for name, off in (('Q', 4), ('par', 4), ('log', 4), ('trew', 4), ('trace', 4), ('last', 4),
                      ('steps_done', 4), ('key_of_row', 2), ('pol_ctr', 2), ('log_len', 2),
                      ('mid', 1)):
        seq, run = qc.fake_structs()
        setattr(run, name, getattr(run, name) + off)
        run.trials = 3
        assert qc.run_rc(seq, run) == _lib.E_ARG, name
        assert b'misaligned' in _lib.lib().cobel_last_error()
    for name, value, code in (('policy', 2, _lib.E_ARG), ('par_rows', 3, _lib.E_ARG),
                              ('n', 5, _lib.E_ARG), ('batch_size', -1, _lib.E_RANGE),
                              ('steps_per_trial', 0, _lib.E_RANGE), ('log_cap', -1, _lib.E_RANGE),
                              ('trials', -1, _lib.E_RANGE)):
        seq, run = qc.fake_structs()
        run.trials = 3
        setattr(run, name, value)
        assert qc.run_rc(seq, run) == code, name
    assert _lib.lib().cobel_qseq_run(C.byref(seq), None, None) == _lib.E_ARG
    # cobel_softmax_n
    f = _lib.lib().cobel_softmax_n
    assert f(0x1000, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, 0, 3, None) == _lib.OK
    assert f(0x1000, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, 4, 0, None) == _lib.E_UNSUPPORTED
    assert f(0x1000, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, 4, 9, None) == _lib.E_UNSUPPORTED
    assert f(None, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, 4, 3, None) == _lib.E_ARG
    assert f(0x1000, None, 0x2000, 0x3000, 2, 0x4000, 0x5000, 4, 3, None) == _lib.E_ARG
    assert f(0x1004, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, 4, 3, None) == _lib.E_ARG
    assert f(0x1000, None, 0x2000, 0x3000, 1, 0x4000, 0x5000, -1, 3, None) == _lib.E_RANGE


# -- the Python surface, host side ------------------------------------------------------------------
def test_softmax_argument_checks():
    from cobel_amd.policy import Policy, Softmax
    assert isinstance(Softmax(), Policy) and Softmax().beta == 1.0
    assert Softmax(np.array([0.5, 2.0])).parameter_column(2).tolist() == [0.5, 2.0]
    assert Softmax(3).parameter_column(7).tolist() == [3.0]
    for bad in (0.0, -1.0, np.array([1.0, 0.0])):
        with pytest.raises(AssertionError):
            Softmax(bad)
    with pytest.raises(AssertionError):
        Softmax(np.array([1.0, 2.0])).parameter_column(3)


def test_key_deduplication():
    from cobel_amd.agent.q_seq import observation_keys
    table = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [-0.0, 1.0]])
    key_of_row, key_obs = observation_keys(table)
    # (-0.0 == 0.0, so the tuples are equal and hash alike: one dict key in the reference too)
    assert key_of_row.tolist() == [0, 1, 2, 1, 0, 2] and key_of_row.dtype == np.int32
    assert np.array_equal(key_obs, [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    for name, c in qc.CASES.items():
        schedule, obs = c['design']()
        key, tuples = qc.keys_of(obs)
        rows = np.stack([np.zeros(len(tuples[0]))] + [np.asarray(o, dtype=np.float64).reshape(-1)
                                                       for o in obs.values()])
        kr, ko = observation_keys(rows)
        assert kr.tolist() == [0] + [key[n] for n in obs], name
        assert [tuple(r) for r in ko.tolist()] == tuples, name


def test_qagent_refuses_what_a_sequence_session_does_not_serve():
    from cobel_amd.agent import QAgent
    from cobel_amd.agent.q_seq import QSequence
    from cobel_amd.policy import EpsilonGreedy, Softmax
    from cobel_amd.spaces import Box, Discrete
    ag = QAgent(Discrete(4), Discrete(3), Softmax())
    with pytest.raises(NotImplementedError, match='Discrete observation spaces'):
        QSequence(ag)
    ag = QAgent(Box(0.0, 1.0, (4,)), Discrete(3), EpsilonGreedy(0.1), Softmax(2.0))
    ag.current_trial = 5
    h = QSequence(ag)
    assert h.current_trial == 5 and h.policy is ag.policy and h.policy_test is ag.policy_test
    assert h._acting_policy(True) is ag.policy and h._acting_policy(False) is ag.policy_test
    h.current_trial = 7
    assert ag.current_trial == 7 and h.callbacks is ag.callbacks
    assert ag.trial_reward_trace is None and ag.trial_steps_trace is None
    assert not hasattr(ag, 'replay') and not hasattr(ag, 'update_q')
