"""What the slices of tests/test_gpu_fuzz_agents.py contain, asserted on the restatements alone, for
exactly the seeds the GPU tests run: a pass there means something only if the cases do reach the
shapes, branches and edges they are drawn for."""
import numpy as np
import pytest

import fuzz_agents_common as fa


# -- PMA ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pma_memory():
    import fuzz_pma as fz
    cases = [fz.draw_case(s) for s in fa.seeds(fa.PMA_MEMORY_FIRSTS, fa.PMA_MEMORY_CHUNK)]
    return cases, [fz.run_reference(c) for c in cases]


@pytest.fixture(scope='module')
def pma_agents():
    import fuzz_pma as fz
    cases = [fz.draw_case(s) for s in fa.seeds(fa.PMA_AGENT_FIRSTS, fa.PMA_AGENT_CHUNK)]
    return cases, [fz.run_reference(c) for c in cases]


def test_pma_slice_shapes(pma_memory):
    cases, _ = pma_memory
    assert {c['A'] for c in cases} == set(range(1, 9))
    assert sum(c['wide'] for c in cases) >= 2 and sum(c['S'] >= 127 for c in cases) >= 2
    assert any(c['wide'] and c['S'] > 128 for c in cases)
    assert any(c['wide'] and c['S'] <= 128 for c in cases)      # a narrow size through the wide form
    assert sum(c['S'] * c['A'] > 512 for c in cases) <= 3
    assert {c['n'] for c in cases} == {1, 2, 5, 64, 65}
    assert {c['gamma'] for c in cases} == {0.5, 0.9, 0.99}
    assert all(op[1] <= 8 for c in cases if c['wide'] for op in c['ops'] if op[0] == 'replay')


def test_pma_slice_scripts(pma_memory):
    import pma_common as pc
    cases, refs = pma_memory
    seen = {k: sum(mem.seen[k] for _, mem in refs) for k in ('replays', 'extended', 'tied')}
    print('PMA memory slice:', seen)
    assert seen['extended'] >= 10 and seen['tied'] >= 10
    fed, flipped, kinds = 0, set(), set()
    for c in cases:
        ops = c['ops']
        for k, op in enumerate(ops):
            if op[0] == 'set':
                flipped.add(op[1])
            if op[0] == 'replay':
                kinds.add(('none' if op[2] is None else 'state', op[3] is not None, op[4]))
            if op[0] == 'update_sr':
                later = [o for o in ops[k + 1:] if o[0] in ('replay', 'update_sr')]
                fed += bool(later) and later[0][0] == 'replay' and later[0][2] is not None
    assert fed >= 5
    assert flipped == set(pc.SWITCHES)
    assert any(op[0] == 'mask' for c in cases for op in c['ops'])
    assert {k[0] for k in kinds} == {'none', 'state'} and {k[1] for k in kinds} == {False, True}
    assert {k[2] for k in kinds} == {False, True}
    lengths = {op[1] for c in cases for op in c['ops'] if op[0] == 'replay'}
    assert 1 in lengths and max(lengths) >= 32
    # the SR the replays read did come from update_sr: it differs from the constructor's
    changed = sum(len(w['SR']) > 1 and not np.array_equal(w['SR'][0], w['SR'][-1]) for w, _ in refs)
    assert changed >= 5
    # repeated experiences, rewards of either sign and zero, terminal flags
    stores = [op for c in cases for op in c['ops'] if op[0] == 'store']
    assert any(a[1:3] == b[1:3] for c in cases
               for a, b in zip(c['ops'], c['ops'][1:]) if a[0] == b[0] == 'store')
    assert {np.sign(op[3]) for op in stores} == {-1.0, 0.0, 1.0} and {op[5] for op in stores} == {0, 1}


def test_pma_agent_slice(pma_agents):
    cases, refs = pma_agents
    at_goal = sum(bool((w['last'] >= 0).any()) for w, _ in refs)
    print('PMA agent slice: %d of %d cases end trials at the goal' % (at_goal, len(cases)))
    assert at_goal >= 3
    assert any(c['wide'] for c in cases) and any(c['shared'] for c in cases)
    assert any(not c['shared'] for c in cases)
    assert any(len(c['sessions']) == 2 for c in cases)
    assert any(s[1] == 1 for c in cases for s in c['sessions'])          # one step per trial
    assert any(s[3] for c in cases for s in c['sessions'])               # no_replay
    assert {type(c['mask']).__name__ for c in cases} >= {'NoneType', 'str', 'ndarray'}
    assert sum(mem.seen['extended'] for _, mem in refs) >= 3
    assert (2, 2) <= min((c['h'], c['w']) for c in cases) and max(c['S'] for c in cases) == 132


# -- AssociativeNetwork ---------------------------------------------------------------------------------
def test_anet_slice():
    import fuzz_anet as fz
    cases = [fz.draw_case(s) for s in fa.seeds(fa.ANET_FIRSTS, fa.ANET_CHUNK)]
    assert {c['G'] for c in cases} == {1, 2, 4, 8, 16, 32, 64}
    assert {c['n_actions'] - 1 for c in cases} >= {1, 8}
    drifting = 0
    for c in cases:
        per_wave = 64 // c['G']
        waves = np.arange(c['N']) // per_wave
        drifting += any(len(set(c['schedule_of'][waves == w].tolist())) > 1 for w in set(waves.tolist()))
    assert drifting >= 3
    # a last wavefront that is partly filled
    assert any(c['N'] % (64 // c['G']) for c in cases)
    tie = excitatory = inhibitory = cut = 0
    for c in cases:
        ref = fz.restate_instance(c, 0)
        q0 = ref['q'][0]
        tie += len(q0) > 1 and bool((q0 == q0[0]).all())
        excitatory += bool(ref['We'][-1].any())
        inhibitory += bool(ref['Wi'][-1].any())
        longest = max(len(t) for t in c['schedules'][int(c['schedule_of'][0])])
        cut += any(s[0] in ('train', 'test') and s[2] < longest for s in c['sessions'])
    print('ANet slice: first-step ties %d, excitatory %d, inhibitory %d, capped %d'
          % (tie, excitatory, inhibitory, cut))
    assert tie >= 1 and excitatory >= 5 and inhibitory >= 5 and cut >= 3
    kinds = {(fz._kind(c['kw']['saturation']), fz._kind(c['kw']['learning_rate']), fz._kind(c['eps']))
             for c in cases}
    assert {k[0] for k in kinds} == {k[1] for k in kinds} == {'scalar', 'table', 'per instance'}
    assert {k[2] for k in kinds} == {'scalar', 'per instance'}
    assert {s[0] for c in cases for s in c['sessions']} == {'train', 'test', 'rescale', 'alpha', 'predict'}
    assert {c['kw']['linear_update'] for c in cases} == {False, True}


# -- Continuous2D -----------------------------------------------------------------------------------------
def test_c2d_step_slice():
    import fuzz_c2d as fz
    cases = [fz.draw_case(s) for s in fa.seeds(fa.C2D_STEP_FIRSTS, fa.C2D_STEP_CHUNK)]
    seen = {}
    for c in cases:
        for k, v in fz.run_reference(c)['seen'].items():
            seen[k] = seen.get(k, 0) + v
    print('C2D step slice:', seen)
    # wall hits, guard refusals (move returning the start), trial ends, resets that needed more
    # than one candidate, counter wraps
    assert seen['wall'] >= 1000 and seen['guard'] >= 100 and seen['done'] >= 100
    assert seen['later_candidate'] >= 100 and seen['wrapped'] >= 10
    edges = {c['T'].shape[1] for c in cases}
    assert 3 in edges and 1024 in edges
    assert {c['arena'] for c in cases} == {'star', 'rectangle', 'eight'}
    assert sum(len(c['planted']['vertex']) for c in cases) >= 20
    assert sum(len(c['planted']['wall']) for c in cases) >= 10
    assert any(c['S'] is not c['T'] for c in cases) and any(c['S'] is c['T'] for c in cases)
    assert {c['n'] for c in cases} == set(fz.COUNTS)
    assert {lanes for c in cases for lanes in c['lanes']} == set(fz.LANES)
    assert {len(c['R']) for c in cases} >= {0, 1, 2}


def test_c2d_fallback_case_falls_back():
    import fuzz_c2d as fz
    seen = fz.run_reference(fz.draw_case(fa.C2D_FALLBACK_SEED))['seen']
    assert seen['fell_back'] >= 3 and seen['later_candidate'] >= 10


def test_c2d_wheel_slice_stays_under_the_cap():
    import fuzz_c2d as fz
    total = out = hits = 0
    for s in fa.C2D_WHEEL_SEEDS:
        c = fz.draw_case(s)
        assert c['params']['step_size'] <= 0.03
        assert c['T'][:4].min() >= 0.0 and c['T'][:4].max() <= 1.0      # inside the unit box
        seen = fz.run_reference(c)['seen']
        total, out, hits = total + seen['steps'], out + seen['left_out'], hits + seen['wall']
    print('C2D wheel slice: %d of %d instance-steps left out (%.2f %%), %d wall hits'
          % (out, total, 100.0 * out / total, hits))
    assert out <= fa.WHEEL_LEFT_OUT_CAP * total and hits >= 500


# -- MFEC -------------------------------------------------------------------------------------------------
def test_mfec_slice():
    import fuzz_mfec as fz
    refused, kept, evicting = [], [], 0
    for s in fa.MFEC_SEEDS:
        c = fz.draw_case(s)
        ref, rag, _ = fz.run_reference(c)
        if ref is None:
            refused.append(s)
            continue
        kept.append(c)
        evicting += rag.Q.evicted > 0
    print('MFEC slice: refused %s, %d cases evict' % (refused, evicting))
    assert len(fa.MFEC_SEEDS) == 30 and len(refused) <= fa.MFEC_REFUSED_CAP
    assert any(c['capacity'] > 64 for c in kept) and any(c['k'] == 32 for c in kept)
    assert evicting >= 1
    assert {c['kind'] for c in kept} == {'track', 'grid', 'hex'}


def test_mfec_wide_slice():
    """The slice of the second range: nothing refused by the restatement, and what it reaches."""
    import fuzz_mfec as fz
    seeds = [s for first in fa.MFEC_WIDE_FIRSTS for s in range(first, first + fa.MFEC_WIDE_CHUNK)]
    cases, evicting, longest = [], 0, 0
    for s in seeds:
        c = fz.draw_case(s)
        ref, rag, _ = fz.run_reference(c)
        assert ref is not None, fz.describe(c)
        cases.append(c)
        evicting += rag.Q.evicted > 0
        longest = max(longest, int(ref['buf_len'].max()))
        assert ref['ended'].any()
    print('MFEC wide slice: %d cases evict, longest buffer %d' % (evicting, longest))
    assert len(seeds) == 12 and min(seeds) >= fz.WIDE and evicting >= 3 and longest > 128
    assert {c['size'][1] for c in cases} == {5, 6, 7, 8}
    assert max(c['size'][0] for c in cases) > 1000 and min(c['size'][0] for c in cases) >= 100
    assert {c['features'] for c in cases} == {'lattice', 'onehot', 'random'}
    assert {c['capacity'] for c in cases} >= {64, 128, 300, 2048} and any(c['k'] == 32 for c in cases)
    assert {c['n'] for c in cases} == {1, 2, 65}
    # the first range draws what it always drew
    assert fz.draw_case(7) == {'seed': 7, 'kind': 'hex', 'size': (4,), 'capacity': 65, 'k': 32, 'eps': 0.3,
                               'trials': 31, 'steps': 50, 'n': 2, 'pick': 0, 'base': 300, 'D': 2}
