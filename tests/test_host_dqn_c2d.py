"""cobel_dqn_act_c2d without a GPU: the seeded cases of its restatement (tests/dqn_c2d_common.py)
hold the conditions the GPU test relies on, the export is declared, mirrored and present in the
library, the ctypes mirror of cobel_dqn_c2d_act_t agrees with the C compiler, and malformed
arguments are refused before any launch."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c2d_common as cc  # noqa: E402
import dqn_c2d_common as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000           # an aligned address nobody dereferences


@pytest.mark.parametrize('name', sorted(dc.NEEDS))
def test_seeded_cases_hold_their_conditions(name):
    """On the restatement alone, over the 12 calls of the case the GPU test replays: every action
    occurs; a trial ends by reaching the reward and another by the step limit; an instance freezes
    at trials_target while others go on; the ring of 5 slots wraps; a move ends at a wall; on the
    open field and in the eight-maze a reset takes more than one candidate; in the wedge, whose
    spawn ring lies outside the candidate box, every reset takes the fallback."""
    case = dc.make_case(name, True)
    met = dc.conditions(case, case['steps'], case['logs'])
    assert dc.NEEDS[name] <= met, sorted(dc.NEEDS[name] - met)
    assert ('fallback' in met) == (name == 'wedge')
    last = case['steps'][-1][1]
    assert int(last['fallbacks'][0]) == sum(e[4] and e[5] is None for log in case['logs'] for e in log)
    # the instance frozen from the start: nothing of its own ever moves
    first = case['state']
    for k in ('state', 'env_ctr', 'policy_ctr', 'memory_ctr', 'ring_states', 'ring_size', 'trial',
              'adam_steps', 'batch_slots', 'obs', 'reward_out'):
        assert np.array_equal(last[k][1], first[k][1], equal_nan=True), k
    assert last['stepped'][1] == 0
    # env_ctr stays even and advances by 2k + 4 per restart (2052 for a fallback)
    assert not (last['env_ctr'] & 1).any()
    # a stored transition is one c2d_common.step, and next_states is the observation BEFORE a reset
    arena, st = case['arena'], case['steps'][0][1]
    for e in case['logs'][0][:10]:
        i, a = e[0], e[1]
        slot = (int(st['ring_head'][i]) + int(st['ring_size'][i]) - 1) % case['par']['slots']
        s0 = case['state']['state'][i]
        ws, wr, wd, _ = cc.step(arena['T'], arena['R'], cc.STEP, s0, a, arena['params'])
        assert st['ring_states'][i, slot].tolist() == list(s0[:2])
        assert st['ring_next_states'][i, slot].tolist() == list(ws[:2])
        assert st['ring_rewards'][i, slot] == wr and st['ring_nonterminal'][i, slot] == 1.0 - wd


def test_the_wedge_reset_is_c2d_commons():
    """dqn_c2d_common.reset leaves out the draws of the wedge's 1 024 refused candidates: the same
    result as c2d_common.reset with all of them."""
    arena = dc.arenas()['wedge']
    for g, c in ((10, 0), (79, 4106)):
        assert dc.reset(arena, 77, g, c) == cc.reset(arena['T'], arena['S'], arena['box'],
                                                     arena['fallback'], cc.STEP, 77, g, c)
    assert dc.reset(dc.arenas()['eight'], 77, 3, 0)[2] is False


def test_both_dtypes_walk_the_same_path():
    """The ring's dtype changes what is stored, not what happens: float32 rows are the float64
    rows rounded, every integer array is the same (the Q-values are a handful of numbers both
    dtypes hold exactly)."""
    a, b = dc.make_case('open_field', True), dc.make_case('open_field', False)
    assert a['seed'] == b['seed']
    x, y = a['steps'][-1][1], b['steps'][-1][1]
    for k in ('state', 'env_ctr', 'policy_ctr', 'memory_ctr', 'ring_actions', 'ring_size', 'trial',
              'batch_slots', 'lat_sum', 'obs'):
        assert np.array_equal(x[k], y[k]), k
    assert y['ring_states'].dtype == np.float32
    assert np.array_equal(x['ring_states'].astype(np.float32), y['ring_states'])


def test_export_is_declared_mirrored_and_present():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    assert re.search(r'COBEL_API int cobel_dqn_act_c2d\(const cobel_dqn_c2d_act_t\* run, void\* stream\);',
                     header)
    assert 'cobel_dqn_act_c2d' in _lib.EXPORTS
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.lib()._name], text=True)
    assert re.search(r'\bT cobel_dqn_act_c2d\b', out)
    assert _lib.lib().cobel_abi_version() == 1017


def test_struct_layout_agrees_with_the_c_compiler():
    from cobel_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cobel_hip.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(cobel_dqn_c2d_act_t), '
           'offsetof(cobel_dqn_c2d_act_t, q), offsetof(cobel_dqn_c2d_act_t, epsilon), '
           'offsetof(cobel_dqn_c2d_act_t, obs), offsetof(cobel_dqn_c2d_act_t, mon_stripes));'
           'return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        path, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(path, 'w') as f:
            f.write(src)
        subprocess.check_call(['cc', '-I', os.path.join(ROOT, 'include'), path, '-o', exe])
        size, q, eps, obs, stripes = map(int, subprocess.check_output([exe]).split())
    S = _lib.DQNActC2D
    assert size == C.sizeof(S) and q == S.q.offset == C.sizeof(_lib.C2D)
    assert eps == S.epsilon.offset and obs == S.obs.offset and stripes == S.mon_stripes.offset
    # the fields DeviceMonitors.fill and DQN._run_fused write carry cobel_dqn_act_t's names
    shared = ('q', 'policy_ctr', 'policy_stream', 'is_float64', 'epsilon', 'ring_states',
              'ring_next_states', 'ring_actions', 'ring_rewards', 'ring_nonterminal', 'ring_size',
              'ring_head', 'memory_ctr', 'slots', 'trial', 'step', 'trial_reward', 'active',
              'adam_steps', 'lat_sum', 'lat_cnt', 'reward_sum', 'trial_cap', 'mon_stripes',
              'steps_per_trial', 'trials_target', 'stepped', 'batch_slots', 'batch')
    for name in shared:
        assert hasattr(S, name) and hasattr(_lib.DQNAct, name), name
    assert not hasattr(S, 'model_rewards')


def _run(_lib):
    run = _lib.DQNActC2D()
    run.arena = cc.fill(_lib, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 4, 4, 1, (0, 0, 1, 1), (0.5, 0.5))
    for name in ('q', 'policy_ctr', 'ring_states', 'ring_next_states', 'ring_actions', 'ring_rewards',
                 'ring_nonterminal', 'ring_size', 'ring_head', 'memory_ctr', 'trial', 'step',
                 'trial_reward', 'active', 'stepped', 'batch_slots', 'obs', 'fallbacks'):
        setattr(run, name, FAKE)
    run.epsilon, run.slots, run.batch, run.steps_per_trial, run.trials_target = 0.1, 5, 3, 5, 3
    return run


def test_refusals_before_any_launch():
    from cobel_amd import _lib
    lib = _lib.lib()

    def call(run):
        _lib.check(lib.cobel_dqn_act_c2d(None if run is None else C.byref(run), None))

    call(_run(_lib))                                   # n = 0: nothing to do, OK
    with pytest.raises(AssertionError):
        call(None)
    for name in ('q', 'policy_ctr', 'ring_states', 'ring_head', 'trial', 'active', 'stepped', 'obs',
                 'fallbacks', 'memory_ctr'):
        run = _run(_lib)
        setattr(run, name, None)
        with pytest.raises(AssertionError):
            call(run)
    for name in ('reward_out', 'done_out', 'wall_out', 'adam_steps', 'lat_sum'):   # optional
        run = _run(_lib)
        assert getattr(run, name) is None
        call(run)
    run = _run(_lib)
    run.batch_slots = run.memory_ctr = None            # no batch asked for: no counter needed
    call(run)
    for name in ('edges', 'state', 'env_ctr'):
        run = _run(_lib)
        setattr(run.arena, name, None)
        with pytest.raises(AssertionError):
            call(run)
    for eps in (1.5, -0.1, float('nan')):
        run = _run(_lib)
        run.epsilon = eps
        with pytest.raises(AssertionError):
            call(run)
    run = _run(_lib)
    run.arena.lanes_per_instance = 3
    with pytest.raises(AssertionError, match='3 lanes per instance'):
        call(run)
    for name, bad in (('slots', 0), ('steps_per_trial', 0), ('batch', -1), ('trial_cap', -1)):
        run = _run(_lib)
        setattr(run, name, bad)
        with pytest.raises(IndexError):
            call(run)
    run = _run(_lib)
    run.arena.n_edges = 1025
    with pytest.raises(IndexError, match='1025 edges'):
        call(run)
    for name, off in (('obs', 4), ('fallbacks', 2), ('ring_actions', 4)):
        run = _run(_lib)
        setattr(run, name, FAKE + off)
        with pytest.raises(AssertionError):
            call(run)
