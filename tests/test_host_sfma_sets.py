"""Per-instance parameter sets of SFMA / SFMAMemory, what needs no GPU: the host-side fill, the
layout of the new struct and fields, the Python plumbing on CPU tensors with every refusal, the
condition that every column of a set matters to some instance of the GPU cases (on the NumPy
restatement alone), and what the fixed slice of scripts/fuzz_sfma_sets.py contains."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sfma_sets_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


# ---------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------
def _fill(alpha, gamma, eps, mlr, memory):
    from cobel_amd import _lib
    ps = _lib.SFMAParamSet()
    rc = _lib.lib().cobel_sfma_param_set_fill(alpha, gamma, eps, mlr,
                                              C.byref((C.c_double * 10)(*memory)), C.byref(ps))
    return rc, ps


@pytest.mark.parametrize('eps', [0.0, 0.1, 1.0])
def test_fill_agent_part_is_param_set_fill_and_the_doubles_are_verbatim(eps):
    from cobel_amd import _lib
    memory = [0.9, 0.97, 0.5, 0.3, 1e-6, 20.0, 2.5, 0.1, 0.8, 1.0 / 3.0]
    rc, ps = _fill(0.7, 0.95, eps, 0.8, memory)
    assert rc == _lib.OK
    plain = _lib.ParamSet()
    _lib.check(_lib.lib().cobel_param_set_fill(0.7, 0.95, eps, 0.8, C.byref(plain)))
    assert bytes(ps.agent) == bytes(plain)
    assert [getattr(ps, k) for k in _lib.SFMA_SET_MEMORY] == memory
    assert bytes(ps)[C.sizeof(plain):] == np.array(memory, dtype='<f8').tobytes()


@pytest.mark.parametrize('eps', [-0.01, 1.5, float('nan')])
def test_fill_refuses_epsilon_outside_the_unit_interval(eps):
    from cobel_amd import _lib
    rc, _ = _fill(0.5, 0.5, eps, 0.9, [1.0] * 10)
    assert rc == _lib.E_ARG
    with pytest.raises(AssertionError):
        _lib.check(rc)


# ---------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------
def _header_offsets(ctype, cname, fields):
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){'
           'printf("%%zu", sizeof(%s));' % cname
           + ''.join('printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields)
           + 'printf("\\n");}')
    exe = '/tmp/cobel_sfma_sets_%d' % os.getpid()
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    os.remove(exe)
    return out[0], dict(zip(fields, out[1:]))


def test_layout_of_the_set_and_of_the_new_fields_header_against_ctypes():
    from cobel_amd import _lib
    new = ('param_sets', 'param_index', 'n_param_sets')
    for ctype, cname in ((_lib.SFMAParamSet, 'cobel_sfma_param_set_t'),
                         (_lib.SFMARun, 'cobel_sfma_run_t'), (_lib.SFMAMem, 'cobel_sfma_mem_t')):
        fields = [f[0] for f in ctype._fields_]
        size, off = _header_offsets(ctype, cname, fields)
        assert size == C.sizeof(ctype), cname
        assert off == {f: getattr(ctype, f).offset for f in fields}, cname
        if ctype is not _lib.SFMAParamSet:
            assert tuple(fields[-3:]) == new, cname
    assert C.sizeof(_lib.SFMAParamSet) == 592 and C.sizeof(_lib.SFMAParamSet) % 16 == 0
    assert _lib.SFMAParamSet.agent.offset == 0 and _lib.SFMAParamSet.decay_inhibition.offset == 512
    assert tuple(f[0] for f in _lib.SFMAParamSet._fields_[1:]) == _lib.SFMA_SET_MEMORY


def test_no_field_that_existed_before_has_moved():
    """The two launch structs as they were (their fields without the three appended ones) have
    the offsets they had: the new fields start where the old struct ended."""
    from cobel_amd import _lib
    for ctype, old_size, seed_at in ((_lib.SFMARun, 344, 336), (_lib.SFMAMem, 184, 176)):
        class Old(C.Structure):
            _fields_ = ctype._fields_[:-3]
        assert C.sizeof(Old) == old_size and Old.seed.offset == seed_at
        for name, _ in Old._fields_:
            assert getattr(ctype, name).offset == getattr(Old, name).offset, name
        assert ctype.param_sets.offset == old_size
        assert ctype.param_index.offset == old_size + 8
        assert ctype.n_param_sets.offset == old_size + 16
        assert C.sizeof(ctype) == old_size + 24
    assert _lib.lib().cobel_abi_version() == 1017


# ---------------------------------------------------------------------------------------------
# host plumbing on CPU tensors
# ---------------------------------------------------------------------------------------------
def cpu_memory(n, S=25, **attrs):
    """An SFMAMemory whose ``table`` is a CPU tensor of N instances — ``_fill_params`` reads its
    shape and its device only, so the sets and the index are built without a GPU."""
    import torch
    from cobel_amd.memory import SFMAMemory
    mem = SFMAMemory(np.eye(S), S, 4)
    mem.table = torch.empty((n, S, 4), dtype=torch.int64)
    for k, v in attrs.items():
        setattr(mem, k, v)
    return mem


def held_sets(mem, who):
    from cobel_amd import _lib
    h = mem._psets[who]
    raw = h['sets'].numpy().tobytes()
    sets = (_lib.SFMAParamSet * h['n']).from_buffer_copy(raw)
    return sets, h['index'].numpy().view(np.uint16), h


def test_distinct_rows_become_sets_with_the_right_index():
    from cobel_amd import _lib
    n = 12
    cols = sc.columns(sc.SETS4, sc.WHICH12)
    mem = cpu_memory(n, **{k: cols[k] for k in sc.MEMORY})
    mem.learning_rate = cols['model_lr']
    run = _lib.SFMARun()
    sf = mem._fill_params(run, (cols['alpha'], cols['gamma'], cols['epsilon']))
    assert sf == _lib.SF_R_NORMALIZE
    sets, index, held = held_sets(mem, 'agent')
    assert run.n_param_sets == held['n'] == 4
    assert run.param_sets == held['sets'].data_ptr() and run.param_index == held['index'].data_ptr()
    assert index.shape == (n,)
    names = dict(zip(sc.MEMORY, _lib.SFMA_SET_MEMORY))
    for i in range(n):
        ps, want = sets[int(index[i])], sc.SETS4[sc.WHICH12[i]]
        got = {k: getattr(ps.agent, k) for k in sc.AGENT}
        got.update({k: getattr(ps, names[k]) for k in sc.MEMORY})
        assert got == {k: want[k] for k in sc.PARAMETERS}, i
        rc, filled = _fill(*[want[k] for k in sc.AGENT], [want[k] for k in sc.MEMORY])
        assert rc == _lib.OK and bytes(ps) == bytes(filled)
    # the scalar fields: set 0's values as placeholders
    first = sets[0]
    assert (run.alpha, run.gamma, run.epsilon, run.model_lr) == (
        first.agent.alpha, first.agent.gamma, first.agent.epsilon, first.agent.model_lr)
    assert [getattr(run, k) for k in _lib.SFMA_SET_MEMORY] == \
        [getattr(first, k) for k in _lib.SFMA_SET_MEMORY]


def test_one_array_among_scalars_and_the_memory_s_own_table():
    """The memory's own calls: its ten columns and ``learning_rate``, the agent part at defaults."""
    from cobel_amd import _lib
    beta = np.array([5.0, 20.0, 5.0, 9.0, 20.0])
    mem = cpu_memory(5, beta=beta)
    m = _lib.SFMAMem()
    mem._fill_params(m)
    sets, index, held = held_sets(mem, 'memory')
    assert m.n_param_sets == 3 and m.param_index == held['index'].data_ptr()
    assert [sets[int(k)].beta for k in index] == list(beta)
    for ps in sets:
        assert (ps.agent.model_lr, ps.decay_inhibition, ps.decay_strength) == (0.9, 0.9, 1.0)
        assert (ps.c_step, ps.i_step, ps.r_threshold) == (1.0, 1.0, 10.0 ** -6)
        assert 0.0 <= ps.agent.epsilon <= 1.0
    assert m.beta == sets[0].beta and m.model_lr == 0.9


def test_the_cache_hits_on_equal_bytes():
    from cobel_amd import _lib
    mem = cpu_memory(6, decay_inhibition=np.array([0.5, 0.9, 0.5, 0.9, 0.7, 0.7]))
    mem._fill_params(_lib.SFMAMem())
    _, _, held = held_sets(mem, 'memory')
    first = (held['sets'], held['index'], held['key'])
    mem.decay_inhibition = np.array([0.5, 0.9, 0.5, 0.9, 0.7, 0.7])      # equal bytes, another array
    m = _lib.SFMAMem()
    mem._fill_params(m)
    assert held['sets'] is first[0] and held['index'] is first[1]
    assert m.param_sets == first[0].data_ptr() and m.n_param_sets == 3
    mem.decay_inhibition = np.array([0.5, 0.9, 0.5, 0.9, 0.7, 0.6])
    mem._fill_params(m)
    assert held['sets'] is not first[0] and held['key'] != first[2] and m.n_param_sets == 4
    # the agent's table is kept apart from the memory's
    mem._fill_params(_lib.SFMARun(), (0.9, 0.9, 0.1))
    assert set(mem._psets) == {'memory', 'agent'}


def test_scalars_only_give_a_null_index_and_the_scalar_fields_as_before():
    from cobel_amd import _lib
    mem = cpu_memory(4, beta=7, decay_strength=0.97, blend=0.25)
    run = _lib.SFMARun()
    mem._fill_params(run, (0.8, 0.95, 0.2))
    assert run.param_index is None and run.param_sets is None and run.n_param_sets == 0
    assert (run.alpha, run.gamma, run.epsilon, run.model_lr) == (0.8, 0.95, 0.2, 0.9)
    assert (run.decay_inhibition, run.decay_strength, run.c_step, run.i_step) == (0.9, 0.97, 1.0, 1.0)
    assert (run.r_threshold, run.beta, run.reward_modulation) == (10.0 ** -6, 7.0, 1.0)
    assert (run.blend, run.interp_fwd, run.interp_rev) == (0.25, 0.5, 0.5)
    assert mem._psets == {}
    m = _lib.SFMAMem()
    mem._fill_params(m)
    assert m.param_index is None and m.n_param_sets == 0 and m.beta == 7.0 and m.model_lr == 0.9


def test_a_wrong_shape_is_refused_with_hyper_s_message():
    from cobel_amd import _lib
    from cobel_amd.memory import _device
    for bad in (np.ones(5), np.ones((4, 1)), np.ones(0)):
        mem = cpu_memory(4, beta=bad)
        with pytest.raises(AssertionError) as e:
            mem._fill_params(_lib.SFMAMem())
        assert str(e.value) == _device.PER_INSTANCE_SHAPE
    mem = cpu_memory(4)
    with pytest.raises(AssertionError) as e:
        mem._fill_params(_lib.SFMARun(), (np.full(3, 0.9), 0.9, 0.1))
    assert str(e.value) == _device.PER_INSTANCE_SHAPE
    assert _device.PER_INSTANCE_SHAPE == \
        'per-instance hyper-parameters need one entry per environment instance'


def test_more_than_65535_distinct_rows_are_refused():
    from cobel_amd import _lib
    n = 65536
    mem = cpu_memory(n, S=1, beta=np.arange(n, dtype=np.float64))
    with pytest.raises(AssertionError) as e:
        mem._fill_params(_lib.SFMAMem())
    assert '65535' in str(e.value)
    mem.beta = np.minimum(np.arange(n), 65534).astype(np.float64)      # 65 535 distinct: served
    m = _lib.SFMAMem()
    mem._fill_params(m)
    assert m.n_param_sets == 65535


def test_an_epsilon_outside_the_unit_interval_is_refused_in_a_set():
    from cobel_amd import _lib
    mem = cpu_memory(3)
    with pytest.raises(AssertionError):
        mem._fill_params(_lib.SFMARun(), (0.9, 0.9, np.array([0.1, 1.5, 0.1])))


SWITCHES = ('deterministic', 'recency', 'C_normalize', 'D_normalize', 'R_normalize',
            'reward_mod_local', 'reward_mod', 'state_mod', 'error_mod_local', 'error_mod')


@pytest.mark.parametrize('name', SWITCHES + ('decay_recency',))
def test_an_array_in_a_launch_wide_attribute_of_the_memory_is_refused(name):
    from cobel_amd import _lib
    value = np.array([0.9, 0.8, 0.9]) if name == 'decay_recency' else np.array([True, False, True])
    mem = cpu_memory(3, **{name: value})
    for struct, agent in ((_lib.SFMAMem(), None), (_lib.SFMARun(), (0.9, 0.9, 0.1))):
        with pytest.raises(NotImplementedError) as e:
            mem._fill_params(struct, agent)
        assert name in str(e.value)
    with pytest.raises(NotImplementedError) as e:       # before the store looks at anything else
        mem.store({'state': 0, 'action': 0, 'reward': 0.0, 'next_state': 1, 'terminal': 1})
    assert name in str(e.value)


def _cpu_agent(mem):
    from cobel_amd.agent import SFMA
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    return SFMA(Discrete(mem.nb_states), Discrete(4), EpsilonGreedy(0.1), mem)


@pytest.mark.parametrize('name', ['nb_replays', 'random', 'dynamic', 'start_replay'])
def test_an_array_in_a_launch_wide_attribute_of_the_agent_is_refused(name):
    agent = _cpu_agent(cpu_memory(3))
    setattr(agent, name, np.array([1, 2, 1]) if name == 'nb_replays' else np.array([True, False, True]))
    with pytest.raises(NotImplementedError) as e:       # the first thing the launcher does
        agent._launch(None, agent.policy, 0, 1, 10, 0, 32)
    assert name in str(e.value)


def test_an_array_as_batch_size_or_a_memory_switch_is_refused_by_the_launcher():
    agent = _cpu_agent(cpu_memory(3))
    with pytest.raises(NotImplementedError) as e:
        agent._launch(None, agent.policy, 0, 1, 10, 0, np.array([8, 16, 8]))
    assert 'batch_size' in str(e.value)
    agent.M.recency = np.array([True, False, True])
    with pytest.raises(NotImplementedError) as e:
        agent._launch(None, agent.policy, 0, 1, 10, 0, 32)
    assert 'recency' in str(e.value)


# ---------------------------------------------------------------------------------------------
# sensitivity: every column of a set, and the mode, matters to an instance the GPU tests compare
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.PARAMETERS + ('mode',))
def test_every_parameter_matters_to_an_instance_the_restatement_reruns(name):
    """Among the instances of the oracle cases that test_gpu_sfma_sets.py re-runs with their own
    parameters there is one whose final Q, C or replayed rows change when this one parameter is
    put back to set 0's value — under a mode and switches for which it acts.  A kernel that
    ignored the column could then not pass."""
    base = sc.SETS8[0][name]
    acts = {'blend': ('blend_forward', 'blend_reverse'),
            'interpolation_fwd': ('interpolate',), 'interpolation_rev': ('interpolate',)}
    if name == 'reward_modulation':
        assert sc.ORACLE_OPTS['reward_mod_local']
    found = []
    for case, c in sc.ORACLE_CASES.items():
        for i in c['rerun']:
            own = sc.SETS8[sc.WHICH16[i]]
            if own[name] == base or (name in acts and own['mode'] not in acts[name]):
                continue
            if sc.outcome(sc.oracle_case_run(case, i)) != \
                    sc.outcome(sc.oracle_case_run(case, i, {name: base})):
                found.append((case, i))
    assert found, 'no re-run instance depends on ' + name


def test_the_sets_of_the_gpu_cases():
    assert len(sc.SETS8) == 8 and len(sc.WHICH16) == 16 and set(sc.WHICH16) == set(range(8))
    for name in sc.PARAMETERS + ('mode',):
        assert len({s[name] for s in sc.SETS8}) >= 2, name
    for c in sc.ORACLE_CASES.values():
        assert len(c['rerun']) == 6 and len({sc.WHICH16[i] for i in c['rerun']}) == 6
    assert {sc.WHICH16[i] for c in sc.ORACLE_CASES.values() for i in c['rerun']} == set(range(1, 8))
    rows = {tuple(sorted(s.items())) for s in sc.SETS4}
    assert len(rows) == 4 and sc.WHICH12 == sorted(sc.WHICH12)
    # three consecutive instances per set: a scalar launch of three can have the same global ids
    assert all(sc.WHICH12[3 * k:3 * k + 3] == [k] * 3 for k in range(4))
    # the scalar launch of set 0 on 5x5 is fast-eligible, those of the other sets are not all
    assert sc.SETS4[0]['decay_strength'] == 1.0 and sc.SETS4[2]['decay_strength'] != 1.0


# ---------------------------------------------------------------------------------------------
# what the fixed slice of scripts/fuzz_sfma_sets.py holds
# ---------------------------------------------------------------------------------------------
def _slice():
    import fuzz_sfma_sets as fz
    from test_gpu_fuzz_sfma_sets import CHUNK, FIRSTS
    seeds = [s for first in FIRSTS for s in range(first, first + CHUNK)]
    return fz, seeds, [fz.draw_case(s) for s in seeds]


def test_sweep_cases_are_drawn_alike_every_time():
    fz, seeds, _ = _slice()
    assert len(seeds) == 32 and len(set(seeds)) == 32
    a, b = fz.draw_case(17), fz.draw_case(17)
    assert a == b and fz.describe(a) == fz.describe(b)
    assert fz.describe(a) != fz.describe(fz.draw_case(18))
    assert len(fz.MODES) == 7
    assert set(fz.BASE_SET) == set(fz.CHOICES) == set(sc.PARAMETERS)


def test_what_the_sweep_slice_contains():
    fz, _, cases = _slice()
    assert {c['form'] for c in cases} == set(fz.FORMS)
    assert {len(c['sets']) for c in cases} >= {1, 2, 8}
    assert {c['n'] for c in cases} == {3, 12, 40}
    assert {s['mode'] for c in cases for s in c['sets']} == set(fz.MODES)
    for name in sc.PARAMETERS:          # every column takes a value other than the default's
        assert any(s[name] != fz.BASE_SET[name] for c in cases for s in c['sets']), name
    # an instance whose set is not set 0, and sets that several instances share
    assert any(len(set(c['which'])) > 1 for c in cases)
    assert any(len(c['which']) > len(set(c['which'])) for c in cases)
    assert all(0 <= k < len(c['sets']) for c in cases for k in c['which'])
    assert all(0.0 <= s['epsilon'] <= 1.0 for c in cases for s in c['sets'])
    switches = {k for c in cases for k in c['opts']}
    assert switches >= {'recency', 'deterministic', 'reward_mod_local', 'reward_mod', 'dynamic',
                        'start_replay', 'nb_replays'}
    sizes = [c['h'] * c['w'] for c in cases]
    assert min(sizes) <= 16 and max(sizes) > 64            # two experiences per lane ... the general kernel
    # the restatement serves a case of the slice with each instance's own parameters
    c = cases[0]
    world, D = fz.make_world(c)
    if world is not None:
        import test_gpu_sfma as T
        ag = sc.oracle_run(T._oracle_world(world), D, c['base'], c['sets'][c['which'][0]],
                           c['opts'], c['trials'], c['steps'], c['B'])
        assert len(ag.steps) == c['trials'] + c['opts'].get('noreplay_trials', 0) + \
            c['opts'].get('test_trials', 0)
