"""``cobel_sr_run`` in both forms (the sparse-reward wave kernel and the row-streaming kernel),
``cobel_sr_init`` and ``cobel_sr_retrieve_q`` with every table inside a frame of sentinels
(tests/frames_common.py): guards intact, framed run bit-equal to the plain run, the form told by
the kernel's ``traffic`` counters, and the edges reached — more trials than ``trial_cap``, SR
changed in the last instance and in the last row.  State counts: one per instantiation of
k_sr_wave (tests/test_gpu_sr_wave.py)."""
import numpy as np
import pytest
import torch

import frames_common as fc

pytestmark = pytest.mark.gpu

BIG_T = 0x7fffffff
DYADIC = [1.0, -0.5, 0.25, 0.5, -0.25, 0.125, 2.0, -1.0, 0.75, -0.125, 1.5, 0.0625]
SHAPES = [(1, 3), (5, 5), (13, 17), (16, 16), (20, 24), (31, 31), (32, 32)]
N = 5
BUDGETS, SPT, TRIAL_CAP = (40, 1, 33), 9, 3


def world_of(h, w, rewarded):
    """Terminal goal in the middle, starts at the first and the LAST state, ``rewarded`` rewarded
    states in two clusters beside the starts (fewer where the world is smaller than that)."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    S = h * w
    if S == 3:
        return make_gridworld(h, w, terminals=[0], goals=[0],
                              rewards=np.array([[0, 1.0], [1, -0.5]]), starting_states=[2])
    goal = S // 2
    cells = [goal]
    k = 1
    while len(cells) < min(rewarded, S - 4):
        for c in (S - 1 - k, k):
            if c not in cells and len(cells) < rewarded:
                cells.append(c)
        k += 1
    rewards = np.array([[c, DYADIC[j % len(DYADIC)]] for j, c in enumerate(cells)])
    return make_gridworld(h, w, terminals=[goal], goals=[goal], rewards=rewards,
                          starting_states=[S - 1, 0])


def sr_arrays(ag):
    out = {'sr': ag._sr, 'T': ag._T, 'rw': ag._rw, 'inst': ag.inst, 'last_exp': ag._last_exp,
           'traffic': ag.traffic}
    out.update(fc.monitor_arrays(ag.monitors))
    return {k: v.clone() for k, v in out.items()}


def drive(world, framed, stream_rows, mask, edit, shift=0):
    from cobel_amd import _lib
    from cobel_amd.agent import SR
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(world, n_envs=N, seed=31337, instance_base=7)
    ag = SR(env.observation_space, env.action_space, EpsilonGreedy(0.25), learning_rate=0.5,
            gamma=0.875)
    ag.stream_rows = stream_rows
    ag.track_occupancy = ag.track_responses = ag.track_instances = True
    if mask is not None:
        ag.mask_actions, ag.action_mask = True, mask
    ag._bind(env)
    if edit is not None:
        ag._rw[:, edit] = 0.5
    ag._env_in(env)
    flags = _lib.F_LEARN | ag._policy_in(ag.policy, env, False)
    if mask is not None:
        flags |= _lib.F_MASK_ACTIONS
    ag.monitors.reserve(TRIAL_CAP, N, True)
    frames = None
    if framed:
        frames = fc.Frames(shift)
        fc.swap_fused(frames, ag)
        frames.swap(ag, '_sr', fc.BIG)
        frames.swap(ag, '_T', 0)              # (an index table: state 0)
        frames.swap(ag, '_rw', fc.BIG)
        frames.swap(ag, 'traffic', fc.MARK)
        if mask is not None:
            fc.frame_mask(frames, ag)
    for b in BUDGETS:
        ag._launch(env, ag.policy, flags, BIG_T, SPT, b, 0)
    torch.cuda.synchronize()
    return sr_arrays(ag), ag, frames


@pytest.mark.parametrize('stream_rows', [False, True])
@pytest.mark.parametrize('h,w,variant', [(h, w, v) for h, w in SHAPES
                                         for v in ('three', 'twelve', 'dense')
                                         if h * w >= 25 or v == 'three'])
def test_sr_run(h, w, variant, stream_rows):
    """3 rewarded states (the 8-slot form), 12 (the 32-slot form), and a hand-edited estimate at a
    state the world does not reward (full row sums from memory); masks at three of the sizes.  (A
    world of three states has room for the first only.)"""
    from cobel_amd import _lib
    S = h * w
    world = world_of(h, w, 12 if variant == 'twelve' else 3)
    edit = S // 2 + 1 if variant == 'dense' else None
    mask = None
    if S in (25, 256, 961):
        nxt = np.asarray(world['next'])
        mask = nxt != np.arange(S)[:, None]
        mask[~mask.any(axis=1)] = True
    plain, _, _ = drive(world, False, stream_rows, mask, edit)
    framed, ag, frames = drive(world, True, stream_rows, mask, edit)
    frames.check()
    fc.assert_same(plain, framed)
    traffic = framed['traffic'].cpu().numpy()
    steps = N * sum(BUDGETS)
    if stream_rows:
        assert traffic.sum() == 0, 'the row-streaming kernel counts no traffic'
    else:
        assert traffic[1] == steps, 'the wave kernel writes one SR row per step'
        assert (traffic[3] > 0) == (variant == 'dense'), traffic
    assert ag.env_steps() == steps
    inst = framed['inst'].cpu().numpy()
    assert inst[:, _lib.I_TRIAL].max() > TRIAL_CAP, 'no instance ran past trial_cap'
    sr = framed['sr'].cpu().numpy()
    eye = np.eye(S, dtype=np.float32)
    assert not np.array_equal(sr[-1], eye), 'SR of the last instance did not change'
    assert any(not np.array_equal(sr[i, -1], eye[-1]) for i in range(N)), 'last row unchanged'
    assert framed['mon.occupancy'].sum().item() == steps
    assert (framed['rw'].cpu().numpy() != 0).any(), 'no reward was estimated'


@pytest.mark.parametrize('S', [3, 5, 21, 25, 37, 40, 41, 221])
@pytest.mark.parametrize('n', [1, 65])
def test_sr_init_and_retrieve_q(n, S):
    """Framed, and ``q_out`` against a float64 restatement of V[T[s, a]], V = SR @ rewards, on
    dense random tables.  (Up to 40 states — a padded row of at most 48 floats — the kernel used to
    zero one or two of the staged reward estimates with the stack of its plan builder: state 12 at
    25 states, state 0 at 40; the sizes up to 41 are here for that.)"""
    from cobel_amd import _lib
    lib = _lib.lib()
    dev = 'cuda'
    sr = fc.frame(torch.full((n, S, S), -3.0, dtype=torch.float32, device=dev), fc.BIG)
    T = fc.frame(torch.full((n, S, 4), -1, dtype=torch.int16, device=dev), 0)
    rw = fc.frame(torch.full((n, S), -3.0, dtype=torch.float32, device=dev), fc.BIG)
    _lib.check(lib.cobel_sr_init(_lib.ptr(sr.view), _lib.ptr(T.view), _lib.ptr(rw.view), n, S, None))
    torch.cuda.synchronize()
    assert sr.intact() and T.intact() and rw.intact()
    assert torch.equal(sr.view, torch.eye(S, device=dev).expand(n, S, S))
    assert torch.equal(T.view, torch.arange(S, device=dev).view(1, S, 1).expand(n, S, 4)
                       .to(torch.int16))
    assert not rw.view.any()
    # retrieve_q on tables with something in them: V[T[s, a]], V = SR @ rewards
    gen = torch.Generator(device=dev).manual_seed(n + S)
    sr.view.copy_(torch.rand((n, S, S), generator=gen, device=dev))
    # (no estimate is zero: one that the kernel dropped would otherwise go unnoticed)
    dyadic = torch.tensor([-0.5, -0.25, 0.25, 0.5], device=dev)
    rw.view.copy_(dyadic[torch.randint(0, 4, (n, S), generator=gen, device=dev)])
    T.view.copy_(torch.randint(0, S, (n, S, 4), generator=gen, device=dev).to(torch.int16))
    states = torch.randint(0, S, (n,), generator=gen, device=dev).to(torch.int32)
    states[-1] = S - 1
    outs = []
    for framed in (False, True):
        st = fc.frame(states, 0) if framed else None
        q = fc.frame(torch.full((n, 4), -3.0, device=dev), fc.BIG) if framed else None
        sv = st.view if framed else states
        qv = q.view if framed else torch.full((n, 4), -3.0, device=dev)
        _lib.check(lib.cobel_sr_retrieve_q(_lib.ptr(sr.view), _lib.ptr(T.view), _lib.ptr(rw.view),
                                           _lib.ptr(sv), _lib.ptr(qv), n, S, None))
        torch.cuda.synchronize()
        if framed:
            assert st.intact() and q.intact() and sr.intact() and T.intact() and rw.intact()
        outs.append(qv.clone())
    assert fc.same_bits(outs[0], outs[1])
    # float64 here, pairwise float32 sums there.  The S products are below 0.5 each (SR in [0, 1),
    # |rewards| <= 0.5) and rounded once (2^-24 relative); a pairwise sum of S terms adds at most
    # ceil(log2 S) roundings of partial sums below 0.5 S: (1 + 8) * 2^-24 * 0.5 S < 2.7e-7 S.
    V = (sr.view.double() * rw.view.double()[:, None, :]).sum(dim=2)
    idx = T.view[torch.arange(n, device=dev), states.long()].long()
    want = torch.gather(V, 1, idx)
    assert torch.allclose(outs[1].double(), want, rtol=0, atol=2.7e-7 * S)


@pytest.mark.parametrize('stream_rows', [False, True])
@pytest.mark.parametrize('h,w', [(5, 5), (20, 24)])
def test_tables_sixteen_bytes_off_a_256_byte_boundary(h, w, stream_rows):
    """``sr`` is checked for 16 bytes, ``inst`` and ``trans`` for 8, and the widest access of both
    kernels is a float4 at a multiple of 16 bytes from a table's base (480 states: float4 rows):
    every framed table starts 16 bytes behind a 256-byte boundary; same assertions."""
    world = world_of(h, w, 3)
    plain, _, _ = drive(world, False, stream_rows, None, None)
    framed, ag, frames = drive(world, True, stream_rows, None, None, shift=16)
    frames.check()
    fc.assert_same(plain, framed)
    assert ag._sr.data_ptr() % 256 == 16 and ag._rw.data_ptr() % 256 == 16
    traffic = framed['traffic'].cpu().numpy()
    assert (traffic.sum() == 0) if stream_rows else (traffic[1] == N * sum(BUDGETS))


@pytest.mark.parametrize('off', [1, 2])
def test_a_transition_table_off_its_eight_bytes_is_refused(off):
    """``trans`` is declared as 16-bit entries, but both kernels read a state's four successors as
    one 64-bit word: cobel_sr_run refuses a table that is not 8-byte aligned."""
    from cobel_amd import _lib
    from cobel_amd.agent import SR
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(world_of(5, 5, 3), n_envs=N, seed=31337)
    ag = SR(env.observation_space, env.action_space, EpsilonGreedy(0.25))
    ag._bind(env)
    ag._env_in(env)
    flags = _lib.F_LEARN | ag._policy_in(ag.policy, env, False)
    ag.monitors.reserve(TRIAL_CAP, N, True)
    big = torch.zeros(ag._T.numel() + 4, dtype=torch.int16, device=ag.device)
    big[off:off + ag._T.numel()] = ag._T.reshape(-1)
    ag._T = big[off:off + ag._T.numel()].view(ag._T.shape)
    assert ag._T.data_ptr() % 8 == 2 * off
    with pytest.raises(AssertionError, match='8-byte aligned'):
        ag._launch(env, ag.policy, flags, BIG_T, SPT, 20, 0)
    torch.cuda.synchronize()
    assert ag.env_steps() == 0, 'a refused run did something'
