"""Per-instance parameter sets of PMA / PMAMemory, what needs no GPU: the exports, the layout of the
new structs (``cobel_pma_mem_t`` itself keeps its 192 bytes; the sets follow it in a
``cobel_pma_mem_sets_t``), the host-side fill with its refusals, every refusal
of the entry points before a device call (fake addresses), the Python plumbing on CPU tensors, the
condition that the sets of the GPU cases act differently (on the NumPy restatement alone), and
what the fixed slice of scripts/fuzz_pma_sets.py contains."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pma_common as pc
import pma_sets_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
NEW = ('cobel_pma_param_set_fill', 'cobel_pma_update_q_sets')
GOOD = [0.9, 0.8, 0.7, 0.6, 0.99, 1e-6, 0.1]       # the memory's seven


# ---------------------------------------------------------------------------------------------
# exports and layout
# ---------------------------------------------------------------------------------------------
def test_exports_agree():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    names = subprocess.check_output(['nm', '-D', '--defined-only', lib._name]).decode()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS
        getattr(lib, name)
        assert re.search(r'\bT %s\b' % name, names), name
    assert lib.cobel_abi_version() == 1017
    assert re.search(r'#define COBEL_PMA_Q_MEMORY %d\b' % _lib.PMA_Q_MEMORY, header)
    assert re.search(r'#define COBEL_PMA_Q_AGENT %d\b' % _lib.PMA_Q_AGENT, header)
    assert re.search(r'#define COBEL_PMA_SETS %du' % _lib.PMA_SETS, header) and _lib.PMA_SETS == 128


def _header_offsets(tmp_path, cname, fields):
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%%zu", sizeof(%s));' % cname
                   + ''.join('printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields)
                   + 'printf("\\n");return 0;}\n')
    exe = tmp_path / 's'
    subprocess.check_call(['cc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    return out[0], dict(zip(fields, out[1:]))


def test_layout_of_the_set_and_of_the_memory_struct_with_sets(tmp_path):
    from cobel_amd import _lib
    for ctype, cname in ((_lib.PMAParamSet, 'cobel_pma_param_set_t'),
                         (_lib.PMAMem, 'cobel_pma_mem_t'), (_lib.PMAMemSets, 'cobel_pma_mem_sets_t'),
                         (_lib.PMARun, 'cobel_pma_run_t')):
        fields = [f[0] for f in ctype._fields_]
        size, off = _header_offsets(tmp_path, cname, fields)
        assert size == C.sizeof(ctype), cname
        assert off == {f: getattr(ctype, f).offset for f in fields}, cname
    assert C.sizeof(_lib.PMAParamSet) == 80 and C.sizeof(_lib.PMAParamSet) % 16 == 0
    assert tuple(f[0] for f in _lib.PMAParamSet._fields_) == _lib.PMA_SET_MEMORY + _lib.PMA_SET_AGENT


def test_no_field_that_existed_before_has_moved():
    """``cobel_pma_mem_t`` is what it was (192 bytes, ``seed`` last) and is the head of
    ``cobel_pma_mem_sets_t``, whose three fields start where it ends; ``cobel_pma_run_t`` is as it
    was."""
    from cobel_amd import _lib
    assert C.sizeof(_lib.PMAMem) == 192 and _lib.PMAMem.seed.offset == 184
    assert _lib.PMAMem._fields_[-1][0] == 'seed'
    assert _lib.PMAMemSets.mem.offset == 0
    assert _lib.PMAMemSets.param_sets.offset == 192 and _lib.PMAMemSets.param_index.offset == 200
    assert _lib.PMAMemSets.n_param_sets.offset == 208 and C.sizeof(_lib.PMAMemSets) == 216
    x = _lib.PMAMemSets()
    m = x.mem                            # a view of the head: what the entry points are handed
    m.n = 7
    assert x.mem.n == 7 and C.addressof(m) == C.addressof(x)
    assert C.sizeof(_lib.PMARun) == 128
    assert _lib.lib().cobel_abi_version() == 1017


# ---------------------------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------------------------
def _fill(memory, alpha=0.5, gamma=0.95, eps=0.2):
    from cobel_amd import _lib
    ps = _lib.PMAParamSet()
    rc = _lib.lib().cobel_pma_param_set_fill(C.byref((C.c_double * 7)(*memory)), alpha, gamma, eps,
                                             C.byref(ps))
    return rc, ps, _lib.lib().cobel_last_error().decode()


def test_fill_round_trips_its_ten_values():
    from cobel_amd import _lib
    # (nothing but the epsilons and the memory's gamma has a range: the reference gives none)
    for memory, agent in ((GOOD, (0.5, 0.95, 0.2)), ([-2.0, 3.0, 1.5, 0.0, 7.0, -1.0, 0.0],
                                                     (-0.5, 2.0, 1.0))):
        rc, ps, _ = _fill(memory, *agent)
        assert rc == _lib.OK
        assert [getattr(ps, k) for k in _lib.PMA_SET_MEMORY] == memory
        assert tuple(getattr(ps, k) for k in _lib.PMA_SET_AGENT) == agent
        assert bytes(ps) == np.array(memory + list(agent), dtype='<f8').tobytes()


@pytest.mark.parametrize('what,value,text', [
    ('memory_epsilon', -0.01, "the memory's epsilon -0.01 outside [0, 1]"),
    ('memory_epsilon', 1.5, "the memory's epsilon 1.5 outside [0, 1]"),
    ('memory_epsilon', float('nan'), "the memory's epsilon nan outside [0, 1]"),
    ('epsilon', -0.25, "the acting policy's epsilon -0.25 outside [0, 1]"),
    ('epsilon', 2.0, "the acting policy's epsilon 2 outside [0, 1]"),
    ('gamma', 1.0, "the memory's gamma 1 outside [0, 1)"),
    ('gamma', -0.5, "the memory's gamma -0.5 outside [0, 1)"),
    ('gamma', float('nan'), "the memory's gamma nan outside [0, 1)"),
])
def test_fill_refuses_each_bad_value_with_its_message(what, value, text):
    from cobel_amd import _lib
    memory, eps = list(GOOD), 0.2
    if what == 'memory_epsilon':
        memory[6] = value
    elif what == 'gamma':
        memory[3] = value
    else:
        eps = value
    rc, _, msg = _fill(memory, eps=eps)
    assert rc == _lib.E_ARG and msg == 'cobel_pma_param_set_fill: ' + text
    with pytest.raises(AssertionError):
        _lib.check(rc)


# ---------------------------------------------------------------------------------------------
# the entry points refuse bad sets before any device call (every address below is fake)
# ---------------------------------------------------------------------------------------------
TAIL = ('param_sets', 'param_index', 'n_param_sets')


def fake_mem(**changes):
    """The head of a ``cobel_pma_mem_sets_t`` with fake addresses and three sets behind it
    (``flags`` carries ``PMA_SETS`` unless ``changes`` says otherwise)."""
    from cobel_amd import _lib
    x = _lib.PMAMemSets()
    m = x.mem
    for k, name in enumerate(('q', 'rewards', 'states', 'terminals', 'T', 'SR', 'update_mask',
                              'mem_ctr', 'pol_ctr', 'gamma_pow', 'gamma_q_pow')):
        setattr(m, name, 0x10000 * (k + 1))
    m.n, m.n_states, m.n_actions, m.pow_len = 7, 25, 4, 34
    m.epsilon, m.gamma = 0.1, 0.9
    m.flags = _lib.PMA_SETS
    x.param_sets, x.param_index, x.n_param_sets = 0x200000, 0x300000, 3
    for k, v in changes.items():
        setattr(x if k in TAIL else m, k, v)
    return m


def entry_points():
    """name -> call(mem): every entry point that takes sets, with arguments that pass its other
    checks as far as a check can be passed without a device."""
    from cobel_amd import _lib
    lib = _lib.lib()
    lengths = (C.c_int32 * 7)(*([3] * 7))
    return {
        'cobel_pma_replay': lambda m: lib.cobel_pma_replay(C.byref(m), 8, 0x500000, None, None,
                                                           0x600000, None),
        'cobel_pma_store': lambda m: lib.cobel_pma_store(C.byref(m), 0x500000, None),
        'cobel_pma_update_sr': lambda m: lib.cobel_pma_update_sr(C.byref(m), None),
        'cobel_pma_gain_batch': lambda m: lib.cobel_pma_gain_batch(C.byref(m), 0x500000, 100,
                                                                   0x600000, None),
        'cobel_pma_gain_seq': lambda m: lib.cobel_pma_gain_seq(
            C.byref(m), 0x500000, 100, 0x700000, C.byref(lengths), 1, 3, 0, 0x600000, None),
        'cobel_pma_update_q_sets': lambda m: lib.cobel_pma_update_q_sets(
            C.byref(m), 0x500000, 0x700000, C.byref(lengths), 3, 3, _lib.PMA_Q_AGENT, 0x800000,
            None),
    }, None


BAD_SETS = [
    ('index_without_sets', dict(param_sets=None), 'param_index given without parameter sets'),
    ('no_sets', dict(n_param_sets=0), '0 parameter sets (1 ... 65535)'),
    ('negative_sets', dict(n_param_sets=-1), '-1 parameter sets (1 ... 65535)'),
    ('too_many_sets', dict(n_param_sets=65536), '65536 parameter sets (1 ... 65535)'),
    ('sets_misaligned', dict(param_sets=0x200008),
     'param_sets must be 16-byte, param_index 2-byte aligned'),
    ('index_misaligned', dict(param_index=0x300001),
     'param_sets must be 16-byte, param_index 2-byte aligned'),
]


@pytest.mark.parametrize('case', BAD_SETS, ids=[c[0] for c in BAD_SETS])
def test_every_entry_point_refuses_bad_sets_before_any_launch(case):
    from cobel_amd import _lib
    _, changes, text = case
    calls, _ = entry_points()
    for name, call in calls.items():
        assert call(fake_mem(**changes)) == _lib.E_ARG, name
        assert _lib.lib().cobel_last_error().decode() == '%s: %s' % (name, text)


def test_cobel_pma_trial_checks_the_sets_too():
    """``cobel_pma_trial`` looks at its world first, and a world handle takes a device: without one
    only that order can be pinned here.  Its memory then goes through the ``check_mem`` that
    ``cobel_pma_replay``, ``_store`` and ``_update_sr`` share, whose refusals are the cases above;
    the trial's own refusal of bad sets is exercised on a device, in tests/test_gpu_pma_sets.py."""
    from cobel_amd import _lib
    run = _lib.PMARun()
    m = fake_mem(param_sets=None)
    assert _lib.lib().cobel_pma_trial(None, C.byref(m), C.byref(run), None) != _lib.OK
    assert 'cobel_pma_trial' in _lib.lib().cobel_last_error().decode()


def test_power_tables_not_above_the_length_are_refused():
    from cobel_amd import _lib
    calls, _ = entry_points()
    lib = _lib.lib()
    assert calls['cobel_pma_replay'](fake_mem(pow_len=8)) == _lib.E_ARG
    assert lib.cobel_last_error().decode() == \
        'cobel_pma_replay: the power tables hold 8 entries, 9 are needed'
    assert calls['cobel_pma_gain_seq'](fake_mem(pow_len=3)) == _lib.E_ARG
    assert lib.cobel_last_error().decode() == \
        'cobel_pma_gain_seq: the power tables hold 3 entries, 4 are needed'
    assert calls['cobel_pma_update_q_sets'](fake_mem(pow_len=3)) == _lib.E_ARG
    assert lib.cobel_last_error().decode() == \
        'cobel_pma_update_q_sets: the power table holds 3 entries, 4 are needed'


def test_update_q_sets_wants_an_index_a_table_and_a_known_pair():
    from cobel_amd import _lib
    lib = _lib.lib()
    lengths = (C.c_int32 * 7)(*([3] * 7))

    def call(m, which=_lib.PMA_Q_AGENT, table=0x800000):
        return lib.cobel_pma_update_q_sets(C.byref(m), 0x500000, 0x700000, C.byref(lengths), 3, 3,
                                           which, table, None)
    for without in (dict(param_index=None), dict(flags=0)):
        assert call(fake_mem(**without)) == _lib.E_ARG
        assert lib.cobel_last_error().decode() == \
            'cobel_pma_update_q_sets: the memory carries no param_index'
    assert call(fake_mem(), which=2) == _lib.E_ARG
    assert 'which = 2' in lib.cobel_last_error().decode()
    assert call(fake_mem(), table=None) == _lib.E_ARG
    assert 'the power table is required' in lib.cobel_last_error().decode()
    # the memory's pair reads mem->gamma_q_pow and does not look at the argument
    assert call(fake_mem(gamma_q_pow=None), which=_lib.PMA_Q_MEMORY) == _lib.E_ARG
    assert 'the power table is required' in lib.cobel_last_error().decode()


def test_a_zeroed_tail_passes_the_scalar_checks_unchanged():
    """Without an index the three new fields are not looked at — whatever they hold — and the
    scalar checks are the ones that were: the epsilon's range among them, which a launch with an
    index leaves to the fill."""
    from cobel_amd import _lib
    lib = _lib.lib()
    calls, _ = entry_points()
    plain = dict(param_sets=None, param_index=None, n_param_sets=0)
    # (a zeroed tail under the flag; no flag, and whatever lies behind the 192 bytes is not read)
    for junk in (plain, dict(plain, param_sets=0x200008, n_param_sets=-5),
                 dict(flags=0, param_sets=0x200008, param_index=0x300001, n_param_sets=-5)):
        # n = 0: every check passes, then nothing is launched
        for name in ('cobel_pma_replay', 'cobel_pma_store', 'cobel_pma_update_sr',
                     'cobel_pma_gain_batch'):
            assert calls[name](fake_mem(n=0, **junk)) == _lib.OK, (name, lib.cobel_last_error())
        assert calls['cobel_pma_replay'](fake_mem(n=0, epsilon=1.5, **junk)) == _lib.E_ARG
        assert lib.cobel_last_error().decode() == 'cobel_pma_replay: epsilon 1.5 outside [0, 1]'
        assert calls['cobel_pma_gain_batch'](fake_mem(n=0, epsilon=-1.0, **junk)) == _lib.E_ARG
    # with an index the scalar epsilon is a placeholder
    assert calls['cobel_pma_replay'](fake_mem(n=0, epsilon=1.5)) == _lib.OK
    assert calls['cobel_pma_gain_batch'](fake_mem(n=0, epsilon=1.5)) == _lib.OK
    assert calls['cobel_pma_update_q_sets'](fake_mem(n=0)) == _lib.OK


# ---------------------------------------------------------------------------------------------
# host plumbing on CPU tensors
# ---------------------------------------------------------------------------------------------
def cpu_memory(n, params=None, name='demo_5x5', **attrs):
    """A PMAMemory bound to CPU tensors: ``_fill_params`` builds sets, index and power tables
    without a GPU."""
    import torch
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    p = dict(sc.SETS3[0], **(params or {}))
    _, _, sas, _ = sc.world_of(name)
    mem = PMAMemory(sas, EpsilonGreedy(p['memory_epsilon']), learning_rate=p['learning_rate'],
                    learning_rate_q=p['learning_rate_q'], gamma=p['gamma'], gamma_q=p['gamma_q'])
    mem.learning_rate_T, mem.min_gain = p['learning_rate_T'], p['min_gain']
    for k, v in attrs.items():
        setattr(mem, k, v)
    mem._bind(n, torch.device('cpu'))
    mem._session(sc.SEED, sc.BASE)
    return mem


def held_sets(mem, who):
    from cobel_amd import _lib
    h = mem._psets[who]
    sets = (_lib.PMAParamSet * h['n']).from_buffer_copy(h['sets'].numpy().tobytes())
    return sets, h['index'].numpy().view(np.uint16), h


@pytest.mark.parametrize('which', [sc.WHICH7, sc.ONE7])
def test_distinct_rows_become_sets_with_the_expected_index(which):
    from cobel_amd import _lib
    from cobel_amd.memory.pma import AGENT_DEFAULTS
    cols = sc.columns(sc.SETS3, which)
    mem = cpu_memory(sc.N, cols)
    m = mem._mem()
    x = mem._tail
    sets, index, held = held_sets(mem, 'memory')
    used = sorted(set(which))
    # np.unique sorts the rows: by learning_rate first, 0.5 < 0.75 < 0.9
    order = sorted(used, key=lambda s: [sc.SETS3[s][k] for k in sc.PARAMETERS[:7]])
    assert held['n'] == len(used) == x.n_param_sets <= 65535 and m.flags & _lib.PMA_SETS
    assert [order[k] for k in index] == list(which)
    if which is sc.WHICH7:
        assert index.tolist() == [2, 1, 0, 2, 1, 1, 0]
    for k, s in enumerate(order):
        assert [getattr(sets[k], f) for f in _lib.PMA_SET_MEMORY] == \
            [sc.SETS3[s][f] for f in sc.PARAMETERS[:7]]
        # the memory on its own: the agent part at the agent's defaults
        assert tuple(getattr(sets[k], f) for f in _lib.PMA_SET_AGENT) == AGENT_DEFAULTS
    # placeholders: set 0's values
    assert [getattr(m, f) for f in _lib.PMA_SET_MEMORY] == \
        [getattr(sets[0], f) for f in _lib.PMA_SET_MEMORY]
    assert x.param_sets % 16 == 0 and x.param_index % 2 == 0 and C.addressof(m) == C.addressof(x)
    # the agent's launcher: its three values travel in the set
    agent = (cols['alpha'], cols['agent_gamma'], cols['epsilon'])
    m = mem._mem(agent=agent)
    sets, index, held = held_sets(mem, 'agent')
    assert [order[k] for k in index] == list(which)
    for k, s in enumerate(order):
        assert tuple(getattr(sets[k], f) for f in _lib.PMA_SET_AGENT) == \
            tuple(sc.SETS3[s][f] for f in sc.PARAMETERS[7:])
    assert mem._held is held and list(held['first']) == [sc.SETS3[order[0]][k] for k in sc.PARAMETERS]


def test_power_tables_per_set_and_their_regrowth():
    cols = sc.columns(sc.SETS3, sc.WHICH7)
    mem = cpu_memory(sc.N, cols)
    m = mem._mem(agent=(cols['alpha'], cols['agent_gamma'], cols['epsilon']))
    sets, _, held = held_sets(mem, 'agent')
    assert m.pow_len == 34

    def check(length):
        for name, field in (('gamma_pow', 'gamma'), ('gamma_q_pow', 'gamma_q'),
                            ('agent_pow', 'agent_gamma')):
            tab = held[name].numpy()
            assert tab.shape == (3, length) and tab.dtype == np.float64
            for k in range(3):
                g = getattr(sets[k], field)
                assert tab[k].tolist() == [g ** j for j in range(length)], (name, k)
    check(34)
    first = held['gamma_pow']
    m = mem._mem(length=33, agent=(cols['alpha'], cols['agent_gamma'], cols['epsilon']))
    assert held['gamma_pow'] is first                    # 34 rows serve a replay of 33
    m = mem._mem(length=40, agent=(cols['alpha'], cols['agent_gamma'], cols['epsilon']))
    assert m.pow_len == 41 and m.gamma_pow == held['gamma_pow'].data_ptr()
    assert m.gamma_q_pow == held['gamma_q_pow'].data_ptr()
    check(41)


def test_the_cache_hits_on_equal_bytes_and_one_array_among_scalars_makes_sets():
    mem = cpu_memory(5, learning_rate_q=np.array([0.5, 0.9, 0.5, 0.9, 0.7]))
    mem._mem()
    sets, index, held = held_sets(mem, 'memory')
    assert held['n'] == 3 and index.tolist() == [0, 2, 0, 2, 1]
    kept = held['sets']
    mem.learning_rate_q = np.array([0.5, 0.9, 0.5, 0.9, 0.7])       # another array, equal bytes
    mem._mem()
    assert mem._psets['memory']['sets'] is kept
    mem.learning_rate_q = np.array([0.5, 0.9, 0.5, 0.9, 0.9])
    mem._mem()
    assert mem._psets['memory']['sets'] is not kept and mem._psets['memory']['n'] == 2
    mem.learning_rate_q = 0.9                                        # scalars: the scalar launch
    m = mem._mem()
    x = mem._tail
    assert mem._held is None and not x.param_index and not x.param_sets and x.n_param_sets == 0
    assert not m.flags & 128
    assert m.learning_rate_q == 0.9 and m.pow_len == 34
    # the policy's epsilon is one of the columns
    mem.policy.epsilon = np.array([0.1, 0.1, 0.2, 0.1, 0.1])
    m = mem._mem()
    sets, index, held = held_sets(mem, 'memory')
    assert index.tolist() == [0, 0, 1, 0, 0] and [s.epsilon for s in sets] == [0.1, 0.2]


def test_array_shapes():
    from cobel_amd.memory import _device
    for bad in (np.array([0.5, 0.9]), np.full((4, 1), 0.5), np.full((1, 4), 0.5)):
        mem = cpu_memory(4, learning_rate_T=bad)
        with pytest.raises(AssertionError) as e:
            mem._mem()
        assert str(e.value) == _device.PER_INSTANCE_SHAPE
    mem = cpu_memory(4)
    with pytest.raises(AssertionError) as e:
        mem._mem(agent=(0.9, np.array([0.5, 0.9, 0.99]), 0.1))
    assert str(e.value) == _device.PER_INSTANCE_SHAPE
    mem.policy.epsilon = np.array([0.1, 0.2, 0.3])
    with pytest.raises(AssertionError) as e:
        mem._mem()
    assert str(e.value) == _device.PER_INSTANCE_SHAPE
    # a bad value in a set is the fill's refusal
    mem = cpu_memory(3, gamma_q=np.array([0.5, 0.9, 0.9]))
    mem.gamma = np.array([0.9, 1.0, 0.9])
    with pytest.raises(AssertionError, match=r"the memory's gamma 1 outside \[0, 1\)"):
        mem._mem()


def test_more_than_65535_distinct_rows_are_refused():
    import torch
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    n = 65536
    mem = PMAMemory(np.ones((1, 1, 1)), EpsilonGreedy(0.1))
    mem.min_gain = np.arange(n, dtype=np.float64)
    mem._bind(n, torch.device('cpu'))
    with pytest.raises(AssertionError, match='at most 65535 distinct parameter combinations'):
        mem._mem()


@pytest.mark.parametrize('name,value', [
    ('equal_need', np.array([True, False, True])), ('equal_gain', [True, False, True]),
    ('ignore_barriers', np.array([True, False, True])), ('allow_loops', np.array([0, 1, 0])),
    ('min_gain_mode', ['original', 'other', 'original']), ('wide', np.array([False, True, False])),
    ('need_workspace', np.array([0, 1, 2]))])
def test_an_array_in_a_launch_wide_attribute_is_refused_by_name(name, value):
    with pytest.raises(NotImplementedError) as e:      # (the two that shape the tables: at bind)
        cpu_memory(3, **{name: value})._mem()
    assert str(e.value) == 'PMAMemory.%s is launch-wide: one value for all instances, not an array' % name
    mem = cpu_memory(3)
    setattr(mem, name, value)
    with pytest.raises(NotImplementedError, match='PMAMemory.%s is launch-wide' % name):
        mem.store({'state': 1, 'action': 0, 'reward': 0.0, 'next_state': 2, 'terminal': 1})


def test_launch_wide_constructor_arguments_lengths_and_offline_need():
    from cobel_amd.agent import PMA
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    _, _, sas, _ = sc.world_of('demo_5x5')
    with pytest.raises(NotImplementedError, match='PMAMemory.wide is launch-wide'):
        PMAMemory(sas, EpsilonGreedy(0.1), wide=np.array([True, False]))
    with pytest.raises(NotImplementedError, match='PMAMemory.need_workspace is launch-wide'):
        PMAMemory(sas, EpsilonGreedy(0.1), wide=True, need_workspace=[1, 2])
    mem = cpu_memory(3)
    with pytest.raises(NotImplementedError, match='PMAMemory.offline_need is launch-wide'):
        mem.offline_need = ['host', 'device', 'host']
    assert mem.offline_need == 'host'
    with pytest.raises(NotImplementedError, match='PMAMemory.replay_length is launch-wide'):
        mem.replay(np.zeros((25, 4)), None, np.array([4, 8, 4]), 12)
    agent = PMA(Discrete(25), Discrete(4), EpsilonGreedy(0.1), mem)
    with pytest.raises(NotImplementedError, match='PMA.batch_size is launch-wide'):
        agent.train(None, 1, 10, np.array([8, 4, 8]))


def test_a_constructor_gamma_array_gives_an_sr_per_instance_and_later_ones_leave_it():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    _, _, sas, _ = sc.world_of('demo_5x5')
    gammas = np.array([0.9, 0.8, 0.95, 0.9, 0.8])
    mem = PMAMemory(sas, EpsilonGreedy(0.1), gamma=gammas)
    T = np.sum(sas, axis=1) / 4
    assert mem.SR.shape == (5, 25, 25) and mem.T.shape == (25, 25)
    for i, g in enumerate(gammas):
        assert np.array_equal(mem.SR[i], np.linalg.inv(np.eye(25) - g * T)), i
    assert np.array_equal(mem.SR[0], pc.RefPMAMemory(sas, None, gamma=0.9).SR)
    before = mem.SR.copy()
    mem.gamma = np.array([0.5, 0.5, 0.5, 0.5, 0.5])            # reaches update_sr() only
    assert np.array_equal(mem.SR, before)
    import torch
    mem._bind(5, torch.device('cpu'))
    assert np.array_equal(mem.SR, before) and mem._dev['SR'].shape == (5, 25, 25)
    mem.SR = np.eye(25)                                       # assigning broadcasts, as before
    assert np.array_equal(mem.SR[3], np.eye(25))
    # one entry: one instance, tables without an instance axis
    one = PMAMemory(sas, EpsilonGreedy(0.1), gamma=np.array([0.8]))
    assert one.SR.shape == (25, 25)
    assert np.array_equal(one.SR, np.linalg.inv(np.eye(25) - 0.8 * T))
    # a scalar is what it was, and a count that does not match the instances is refused at bind
    assert np.array_equal(PMAMemory(sas, EpsilonGreedy(0.1), gamma=0.8).SR, one.SR)
    with pytest.raises(AssertionError):
        PMAMemory(sas, EpsilonGreedy(0.1), gamma=gammas)._bind(4, torch.device('cpu'))


def test_update_q_of_the_agent_before_the_first_session_applies_each_instance_s_own():
    from cobel_amd.agent import PMA
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Discrete
    _, _, sas, _ = sc.world_of('demo_5x5')
    update = [{'state': 12, 'action': 1, 'reward': 0.5, 'next_state': 7, 'terminal': 1},
              {'state': 7, 'action': 2, 'reward': 0.0, 'next_state': 8, 'terminal': 1},
              {'state': 8, 'action': 1, 'reward': 10.0, 'next_state': 3, 'terminal': 1}]
    cols = sc.columns(sc.SETS3, sc.WHICH7)
    agent = PMA(Discrete(25), Discrete(4), EpsilonGreedy(0.1), PMAMemory(sas, EpsilonGreedy(0.1)),
                learning_rate=cols['alpha'], gamma=cols['agent_gamma'])
    agent.Q = sc.q_start('demo_5x5')
    agent.update_q(update)
    assert agent.Q.shape == (7, 25, 4)
    ref = pc.RefPMAMemory(sas, None)
    for i, s in enumerate(sc.WHICH7):
        want = ref.update_q(sc.q_start('demo_5x5').copy(), update, sc.SETS3[s]['alpha'],
                            sc.SETS3[s]['agent_gamma'])
        assert np.array_equal(agent.Q[i], want), i
    # scalars: one table, as before
    plain = PMA(Discrete(25), Discrete(4), EpsilonGreedy(0.1), PMAMemory(sas, EpsilonGreedy(0.1)))
    plain.update_q(update)
    assert plain.Q.shape == (25, 4)
    assert np.array_equal(plain.Q, ref.update_q(np.zeros((25, 4)), update, 0.9, 0.99))


def test_spread_over_instances_names_the_pma_attributes():
    from cobel_amd.optimizer.grid_search import spread_over_instances
    doc = spread_over_instances.__doc__
    for name in ('PMAMemory', 'learning_rate_q', 'learning_rate_T', 'gamma_q', 'min_gain', 'PMA'):
        assert name in doc, name
    cols, which = spread_over_instances([{'gamma_q': 0.9, 'epsilon': 0.1},
                                         {'gamma_q': 0.5, 'epsilon': 0.3}], 3)
    assert which.tolist() == [0, 0, 0, 1, 1, 1] and cols['gamma_q'].tolist() == [0.9] * 3 + [0.5] * 3


# ---------------------------------------------------------------------------------------------
# what the cases contain: on the restatement alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True], ids=['own_policy', 'shared_policy'])
@pytest.mark.parametrize('name', list(sc.WORLDS))
def test_the_sets_of_the_gpu_cases_act_differently(name, shared):
    """The condition under which the GPU cases say anything about sets: for every pair of the
    three sets, the restatement's final Q of two instances that differ ONLY in their set (one
    global instance, so the same streams) is different.  A kernel that gave everybody set 0 — or
    any one set — could not equal the scalar launches or the restatement.  (The need mode of a
    case changes where ``compute_need(None)`` runs, not what a set holds.)"""
    inst = sc.BASE + 1
    qs = [sc.ref_run(name, inst, s, shared)[1].Q for s in range(3)]
    for a in range(3):
        for b in range(a):
            assert not np.array_equal(qs[a], qs[b]), (a, b)
    assert all(len({s[k] for s in sc.SETS3}) == 3 for k in sc.PARAMETERS)
    assert len(sc.WHICH7) == sc.N == 7 and sorted(set(sc.WHICH7)) == [0, 1, 2] and sc.BASE == 5
    assert set(sc.ONE7) == {0}


# ---------------------------------------------------------------------------------------------
# what the fixed slice of scripts/fuzz_pma_sets.py holds
# ---------------------------------------------------------------------------------------------
def _slice():
    import fuzz_pma_sets as fz
    from test_gpu_fuzz_pma_sets import CHUNK, FIRSTS
    seeds = [s for first in FIRSTS for s in range(first, first + CHUNK)]
    return fz, seeds, [fz.draw_case(s) for s in seeds]


def test_sweep_cases_are_drawn_alike_every_time():
    fz, seeds, _ = _slice()
    assert len(seeds) == 16 and len(set(seeds)) == 16
    a, b = fz.draw_case(11), fz.draw_case(11)
    assert fz.describe(a) == fz.describe(b) and a['sets'] == b['sets'] and a['which'] == b['which']
    assert fz.describe(a) != fz.describe(fz.draw_case(12))
    assert set(fz.BASE_SET) == set(sc.PARAMETERS) == set(fz.CHOICES) | {'alpha'}


def test_what_the_sweep_slice_contains():
    fz, _, cases = _slice()
    assert {len(c['sets']) for c in cases} >= {1, 2, 3}
    assert {c['n'] for c in cases} == {3, 7, 12}
    assert {c['shared'] for c in cases} == {False, True}
    assert {c['masked'] for c in cases} == {False, True}
    for name in sc.PARAMETERS:          # every column takes a value other than the default's
        assert any(s[name] != fz.BASE_SET[name] for c in cases for s in c['sets']), name
    assert any(len(set(c['which'])) > 1 for c in cases)
    assert any(len(c['which']) > len(set(c['which'])) for c in cases)
    assert all(0 <= k < len(c['sets']) for c in cases for k in c['which'])
    assert all(c['which'][-1] == len(c['sets']) - 1 for c in cases)
    assert any(len(c['sessions']) == 2 for c in cases)
    assert any(s[3] for c in cases for s in c['sessions'])            # a session without replays
    assert min(c['S'] for c in cases) <= 12 and max(c['S'] for c in cases) > 25
    # every case with more than one set: its sets act differently on the restatement
    many = [c for c in cases if len(c['sets']) > 1]
    assert len(many) >= 8
    for c in many:
        assert fz.sets_act_differently(c), fz.describe(c)
