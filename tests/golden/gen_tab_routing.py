"""The routing table of the tabular agents: what ``cobel_tab_describe`` answers over a matrix of
worlds and runs that crosses every edge of the routing (which kernel, how much LDS, how many
workgroups per CU, how many instances per workgroup — or the refusal and its text).

Recorded from the library of the commit BEFORE a change of the host code around the kernels, on
an MI355X (the plans depend on the device's CU count and LDS size); the test that reads the table,
tests/test_gpu_routing.py, holds the library under test to it row by row.  Nothing is launched.

    COBEL_LIB=<library of the parent commit> python tests/golden/gen_tab_routing.py

Writes tab_routing.json: ``worlds`` (name -> states, actions, worlds, drawn), ``defaults`` (the
members of ``cobel_tab_run_t`` most rows share) and ``rows`` (name, world, the members of the run
that differ from the defaults — 0: not set — and the recorded rc / out / error).
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    sys.path.insert(0, p)

from tab_routing_common import describe, make_world  # noqa: E402

Q, DYNA = 0, 1
(LEARN, NO_REPLAY, EPISODIC, MASK_ACTIONS, TEST_STREAM, FORCE_WAVE, FORCE_LDS_MODEL) = (
    1, 2, 4, 8, 16, 32, 64)
TAB_GENERAL, NO_PWG, PWG_GLOBAL = 512, 1024, 2048
FLAGS = dict(LEARN=0, NO_REPLAY=NO_REPLAY, EPISODIC=EPISODIC, MASK_ACTIONS=MASK_ACTIONS,
             TEST_STREAM=TEST_STREAM, FORCE_WAVE=FORCE_WAVE, FORCE_LDS_MODEL=FORCE_LDS_MODEL,
             TAB_GENERAL=TAB_GENERAL, NO_PWG=NO_PWG, PWG_GLOBAL=PWG_GLOBAL)
STATES = (25, 256, 289, 625, 676, 1024, 1089, 4096, 10000, 10404, 16384)
BATCHES = (0, 1, 32, 62, 63, 130)
ACTIONS = (2, 6, 8, 9, 17, 32)


def scratch_bytes(n: int) -> int:
    return (256 + 7 * (n + 8)) * 4


# what a run may bring beyond the required arrays
OPTIONS = dict(
    model_index=dict(model_index='p'),
    occupancy=dict(occupancy='p'),
    param_sets=dict(param_sets='p', param_index='p', n_param_sets=3),
    last_exp=dict(last_exp='p'),
    scratch=dict(scratch='p', scratch_bytes=scratch_bytes(4096)),
    scratch_small=dict(scratch='p', scratch_bytes=scratch_bytes(4096) - 4),
    replay_log=dict(replay_log='p', log_cap=64),
    monitors=dict(lat_sum='p', lat_cnt='p', reward_sum='p', resp_cnt='p', trial_cap=8,
                  mon_stripes=4),
    lat_trace=dict(lat_trace='p', trial_cap=8),
)


# a learning run of 4 096 instances, 32 updates per step
DEFAULTS = dict(q='p', inst='p', n=4096, flags=LEARN, trials_target=10, steps_per_trial=50,
                step_budget=512, batch=32, alpha=0.9, gamma=0.99, epsilon=0.1, model_lr=0.9, seed=7)


def run(agent: int, **over) -> dict:
    """What a row changes in DEFAULTS: its agent, the model table Dyna-Q needs, and ``over``."""
    f = dict(agent=agent, model='p' if agent == DYNA else None)
    f.update(over)
    return f


def matrix():
    worlds, rows = {}, []

    def world(S, A=4, W=1, drawn=False):
        name = 's%d_a%d_w%d%s' % (S, A, W, '_drawn' if drawn else '')
        worlds[name] = dict(states=S, actions=A, worlds=W, drawn=drawn)
        return name

    def add(name, w, fields):
        rows.append(dict(name='%s/%s' % (w, name), world=w, run=fields))

    # four-action worlds: every state count x agent x batch, with and without the model digest
    # (Dyna-Q) or the experience log (QAgent)
    for S in STATES:
        w = world(S)
        for b in BATCHES:
            add('q_b%d' % b, w, run(Q, batch=b))
            add('q_b%d_log' % b, w, run(Q, batch=b, **OPTIONS['replay_log']))
            add('dyna_b%d' % b, w, run(DYNA, batch=b))
            add('dyna_b%d_midx' % b, w, run(DYNA, batch=b, model_index='p'))
            add('dyna_b%d_midx_episodic' % b, w,
                run(DYNA, batch=b, model_index='p', flags=LEARN | EPISODIC))
            add('q_b%d_log_episodic' % b, w,
                run(Q, batch=b, flags=LEARN | EPISODIC, **OPTIONS['replay_log']))
    # each flag alone on a learning run, each option alone, each instance count: on a world of
    # every routing class (tables in LDS with the world, PWG's range, beyond it, beyond k_tab_wpi)
    for S, W in ((25, 1), (25, 2), (676, 1), (676, 2), (1024, 1), (10404, 1)):
        w = world(S, 4, W)
        bases = (('q', run(Q)), ('q_log', run(Q, **OPTIONS['replay_log'])), ('dyna', run(DYNA)),
                 ('dyna_midx', run(DYNA, model_index='p')))
        for bname, base in bases:
            add('%s_test' % bname, w, dict(base, flags=None))
            for fname, f in FLAGS.items():
                fields = dict(base, flags=LEARN | f)
                if f == MASK_ACTIONS:
                    fields['action_mask'] = 'p'
                add('%s_flag_%s' % (bname, fname), w, fields)
            for oname, o in OPTIONS.items():
                add('%s_with_%s' % (bname, oname), w, dict(base, **o))
            for n in (0, 1, 63, 64, 4096):
                add('%s_n%d' % (bname, n), w, dict(base, n=n or None))
            add('%s_n65536_scratch' % bname, w,
                dict(base, n=65536, scratch='p', scratch_bytes=scratch_bytes(65536)))
            add('%s_midx_occupancy_forced_lds' % bname, w,
                dict(base, flags=LEARN | FORCE_LDS_MODEL, model_index='p', occupancy='p'))
    # drawn successors
    for S in (25, 676):
        w = world(S, drawn=True)
        for b in (0, 32, 130):
            add('q_b%d' % b, w, run(Q, batch=b))
            add('q_b%d_log' % b, w, run(Q, batch=b, **OPTIONS['replay_log']))
            add('dyna_b%d' % b, w, run(DYNA, batch=b))
            add('dyna_b%d_midx' % b, w, run(DYNA, batch=b, model_index='p'))
        add('dyna_no_replay', w, run(DYNA, flags=LEARN | NO_REPLAY))
        add('dyna_test', w, run(DYNA, flags=None))
        add('dyna_force_wave', w, run(DYNA, flags=LEARN | FORCE_WAVE))
    # other action counts: QAgent on one wavefront per instance, or the general kernel
    for A, S, W, drawn in [(a, 25, 1, False) for a in ACTIONS] + [
            (17, 256, 1, False), (17, 289, 1, False), (8, 1024, 1, False), (9, 1024, 1, False),
            (6, 1089, 1, False), (32, 625, 1, False), (6, 25, 2, False), (17, 256, 2, False),
            (6, 25, 1, True)]:
        w = world(S, A, W, drawn)
        for b in BATCHES:
            add('q_b%d' % b, w, run(Q, batch=b))
            add('q_b%d_log' % b, w, run(Q, batch=b, **OPTIONS['replay_log']))
        for fname, f in FLAGS.items():
            add('q_log_flag_%s' % fname, w, run(Q, flags=LEARN | f, **OPTIONS['replay_log'],
                                                 action_mask='p' if f == MASK_ACTIONS else None))
        add('q_log_test', w, run(Q, flags=None, **OPTIONS['replay_log']))
        add('q_log_mask_misaligned', w, run(Q, flags=LEARN | MASK_ACTIONS, action_mask='p+1',
                                            **OPTIONS['replay_log']))
        add('q_log_mask_misaligned_n0', w, run(Q, flags=LEARN | MASK_ACTIONS, action_mask='p+1',
                                               n=None, **OPTIONS['replay_log']))
        for oname, o in OPTIONS.items():
            add('q_with_%s' % oname, w, run(Q, **o))
        for n in (0, 1, 63, 64, 4096, 65536):
            add('q_log_n%d' % n, w, run(Q, n=n or None, **OPTIONS['replay_log']))
        add('q_aligned4', w, run(Q, q='p+4'))
        add('dyna', w, run(DYNA))
    # every argument error
    for w in (world(25), world(25, 6)):
        for name, fields in (
                ('null_run', None),
                ('no_q', run(DYNA, q=None)),
                ('no_inst', run(DYNA, inst=None)),
                ('q_off_4', run(Q, q='p+4')),
                ('q_off_1', run(Q, q='p+1')),
                ('inst_off_4', run(Q, inst='p+4')),
                ('n_negative', run(Q, n=-1)),
                ('agent_2', run(2)),
                ('agent_negative', run(-1)),
                ('dyna_no_model', run(DYNA, model=None)),
                ('batch_negative', run(Q, batch=-1)),
                ('steps_per_trial_0', run(Q, steps_per_trial=None)),
                ('epsilon_above_1', run(Q, epsilon=1.5)),
                ('epsilon_negative', run(Q, epsilon=-0.5)),
                ('mask_flag_without_mask', run(Q, flags=LEARN | MASK_ACTIONS)),
                ('trial_cap_negative', run(Q, trial_cap=-1)),
                ('log_cap_negative', run(Q, log_cap=-1)),
                ('param_index_without_sets', run(Q, param_index='p')),
                ('param_index_zero_sets', run(Q, param_index='p', param_sets='p')),
                ('model_index_general', run(Q, flags=LEARN | TAB_GENERAL, model_index='p')),
                ('errors_but_n0', run(2, n=None, q=None))):
            add(name, w, fields)
    rows.append(dict(name='null_world', world=None, run=run(Q)))
    rows.append(dict(name='null_world_n0', world=None, run=run(Q, n=None)))
    names = [r['name'] for r in rows]
    assert len(set(names)) == len(names)
    for r in rows:   # (None or 0 in a run: the member is not set)
        if r['run'] is not None:
            r['run'] = {k: v or 0 for k, v in r['run'].items() if (v or 0) != DEFAULTS.get(k, 0)}
    return worlds, rows


def main() -> None:
    import torch
    from cobel_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    worlds, rows = matrix()
    handles = {name: make_world(lib, spec) for name, spec in worlds.items()}
    for r in rows:
        fields = None if r['run'] is None else dict(DEFAULTS, **r['run'])
        r.update(describe(lib, _lib, handles.get(r['world']), fields, buf.data_ptr()))
    for h in handles.values():
        lib.cobel_world_destroy(h)
    path = os.path.join(HERE, 'tab_routing.json')
    with open(path, 'w') as f:
        f.write('{"worlds": %s,\n "defaults": %s,\n "rows": [\n' % (json.dumps(worlds),
                                                                   json.dumps(DEFAULTS)))
        f.write(',\n'.join(json.dumps(r) for r in rows))
        f.write('\n]}\n')
    kinds = sorted({(r['rc'], r['out'][0]) for r in rows})
    print('%d rows, %d worlds, (rc, kernel) pairs seen: %s -> %s' % (len(rows), len(worlds), kinds,
                                                                     path))


if __name__ == '__main__':
    main()
