"""``cobel_tab_run`` in its seven kernel forms and the Dyna-Q session calls, every caller-owned array
inside a frame of sentinels (tests/frames_common.py).

Each case runs one seeded session twice, plain and framed, and asserts: (1) every guard is intact,
(2) every array of the framed run equals the plain run's bit for bit — a read from beyond a table
picks up the poison and shows here —, (3) the kernel form the case is named after ran
(``cobel_tab_describe``), (4) the edge the case is about was reached (more trials than
``trial_cap``, a full replay log with steps after it, Q changed in the last instance and in the
last row, batches evaluated, a launch that was in fact sliced).  Whether the tables are RIGHT is
left to the tests against the oracles; rewards are dyadic (1, -0.5, 0.25) so that the atomically
accumulated reward sums are exact in any order.

Two arrays are framed but not compared: the scratch area, whose contents between calls are
undefined (ticket counters depend on which wave drew what), and — folded over their stripes
before the comparison — striped monitors, whose stripe is chosen by the wave that ran an
instance."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
from conftest import SEED

pytestmark = pytest.mark.gpu

BIG_T = 0x7fffffff
L_ABORT = 255       # COBEL_TAB_SCRATCH_ABORT_WORD


def _lib():
    from cobel_amd import _lib
    return _lib


def grid(h, w):
    """A field whose two starting states, the first and the LAST one, sit next to a rewarded state
    that ends no trial: Q changes in the last row from the first trials on."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    S = h * w
    goal = S // 2
    return make_gridworld(h, w, terminals=[goal],
                          rewards=np.array([[goal, 1.0], [S - 2, 0.25], [1, -0.5]]), goals=[goal],
                          starting_states=[S - 1, 0])


graph = fc.graph


def make_dynaq(world, n, eps=0.3, alpha=0.5, base=3, **attrs):
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(world, n_envs=n, seed=SEED, instance_base=base, device=torch.device('cuda', 0))
    ag = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(eps), learning_rate=alpha)
    for k, v in attrs.items():
        setattr(ag, k, v)
    return env, ag


def make_q(world, n, eps=0.3, alpha=0.5, gamma=0.9, base=3, topology=False, starts=None, **attrs):
    from cobel_amd.agent import QAgent
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.policy import EpsilonGreedy
    if topology:
        env = Topology(world, starts, n_envs=n, seed=SEED, instance_base=base)
    else:
        env = Gridworld(world, n_envs=n, seed=SEED, instance_base=base,
                        device=torch.device('cuda', 0))
    ag = QAgent(env.observation_space, env.action_space, EpsilonGreedy(eps), learning_rate=alpha,
                gamma=gamma)
    for k, v in attrs.items():
        setattr(ag, k, v)
    return env, ag


def swap_tabular(frames, ag):
    """Every array ``TabularAgent._launch`` and its ``_extra`` put into ``cobel_tab_run_t``."""
    fc.swap_fused(frames, ag)
    frames.swap(ag, '_q', fc.BIG)
    frames.swap(ag, 'batches_done', fc.MARK)
    # (ticket counters and rings whose entries name instances: 0, the empty entry — a ring entry
    #  read from a guard is one not yet written, a counter read from it hands out instance 0)
    frames.swap(ag, '_scratch', 0)
    if hasattr(ag, 'M') and hasattr(ag.M, 'table'):
        frames.swap(ag.M, 'table', fc.MODEL_POISON)
        frames.swap(ag.M, 'index', fc.INDEX_POISON)
    if getattr(ag, '_log', None) is not None:
        frames.swap(ag, '_log', fc.log_poison(ag.n_actions, ag._log_words()))


def tab_arrays(ag):
    out = {'q': ag._q, 'inst': ag.inst, 'last_exp': ag._last_exp, 'batches_done': ag.batches_done}
    if hasattr(ag, 'M') and hasattr(ag.M, 'table'):
        out.update(model=ag.M.table, index=ag.M.index, counter=ag.M.counter)
    if getattr(ag, '_log', None) is not None:
        out['log'] = ag._log
    for k, v in fc.monitor_arrays(ag.monitors).items():
        out[k] = v.sum(dim=0) if k[4:] in ag.monitors._PER_TRIAL else v
    return {k: v.clone() for k, v in out.items()}


def drive(make, framed, budgets, spt, batch, trial_cap, learn=True, extra=0, stripes=1, mask=None,
          log_cap=0, prior=None, shift=0):
    """One session of ``budgets`` launches; returns (arrays, agent, kernels described, frames)."""
    from cobel_amd.agent.agent import DeviceMonitors
    L = _lib()
    env, ag = make()
    if mask is not None:
        ag.mask_actions, ag.action_mask = True, mask
    if prior is not None:
        prior(ag, env)
    ag._bind(env)
    if stripes > 1:
        ag.monitors = DeviceMonitors(ag.device, env.handle.n_worlds, ag.n_states,
                                     ag.track_occupancy, ag.track_responses, stripes)
    ag._env_in(env)
    pol = ag.policy if learn else ag.policy_test
    flags = (L.F_LEARN if learn else 0) | extra | ag._policy_in(pol, env, not learn)
    if mask is not None:
        flags |= L.F_MASK_ACTIONS
    ag.monitors.reserve(trial_cap, ag.n_envs, True)
    assert ag.monitors.cap == trial_cap
    if log_cap:
        ag.reserve_replay(log_cap)
    # (the parameter sets are built by the first _hyper call and kept while the values stay)
    ag._hyper(L.TabRun(), ag.learning_rate, ag.gamma, pol.epsilon, ag._model_lr())
    frames = None
    if framed:
        frames = fc.Frames(shift)
        swap_tabular(frames, ag)
        if mask is not None:
            fc.frame_mask(frames, ag)
    kinds = set()
    for b in budgets:
        what = ag.describe_launch(env, pol, flags, BIG_T, spt, b, batch)
        kinds.add(what['kernel'])
        ag._launch(env, pol, flags, BIG_T, spt, b, batch)
    torch.cuda.synchronize()
    ag.check_launches()
    return tab_arrays(ag), ag, kinds, frames, what


def twin(make, expect, **how):
    """Plain and framed run of one session: assertions 1 to 3 and the preconditions all cases
    share; returns the framed agent and its arrays for the case's own."""
    L = _lib()
    plain, ag0, kinds0, _, _ = drive(make, False, **how)
    framed, ag, kinds, frames, what = drive(make, True, **how)
    frames.check()
    fc.assert_same(plain, framed)
    assert kinds == kinds0 == set(expect), (kinds, expect)
    inst = framed['inst'].cpu().numpy()
    # the monitors' edge: trials beyond trial_cap were finished (and counted nowhere)
    assert inst[:, L.I_TRIAL].max() > how['trial_cap'], 'no instance ran past trial_cap'
    if how.get('learn', True):
        q = framed['q'].cpu().numpy()
        assert q[-1].any(), 'Q of the last instance did not change'
        assert q[:, -1].any(), 'the last row of Q changed in no instance'
    return ag, framed, what


# -- one lane per instance ---------------------------------------------------------------------------
def test_lpi_q_agent_without_replay():
    """k_tab_lpi: QAgent, batch 0, 65 instances (a wave and one lane); the log is kept and full."""
    L = _lib()
    budgets = (9, 21, 7)
    cap = sum(budgets) - 3
    ag, out, _ = twin(lambda: make_q(grid(5, 5), 65), {L.TAB_KERNEL_LPI}, budgets=budgets, spt=5,
                      batch=0, trial_cap=2, log_cap=cap)
    assert (out['inst'][:, L.I_LOG_LEN] == cap).all(), 'the log is not exactly full'
    assert ag.env_steps() == 65 * sum(budgets)


def test_lpi_dynaq_test_session():
    """k_tab_lpi acting only: DynaQ.test() on learned tables; Dyna-Q training WITHOUT replay is
    routed to the wavefront kernel (tab_plan: a lane per instance keeps nothing but Q)."""
    L = _lib()
    twin(lambda: make_dynaq(grid(5, 5), 65), {L.TAB_KERNEL_LPI}, budgets=(30, 11), spt=5, batch=0,
         trial_cap=4, learn=False, prior=lambda ag, env: ag.train(env, 3, 10, 20))
    ag, out, _ = twin(lambda: make_dynaq(grid(5, 5), 65), {L.TAB_KERNEL_WPI}, budgets=(30, 11), spt=5,
                      batch=20, trial_cap=2, extra=L.F_NO_REPLAY)
    assert int(out['batches_done'].item()) == 0


# -- one wavefront per instance ----------------------------------------------------------------------
def _bump_mask(world):
    nxt = np.asarray(world['next'])
    m = nxt != np.arange(nxt.shape[0])[:, None]
    m[~m.any(axis=1)] = True
    return m


@pytest.mark.parametrize('h,w', [(5, 5), (7, 9)])
@pytest.mark.parametrize('form', ['mask', 'episodic', 'test', 'fast', 'index', 'psets', 'last_exp'])
def test_wavefront_per_instance(form, h, w):
    """k_tab_wpi and its two plain-training instantiations at 25 and 63 states (one short of a
    wave of rows), three instances, batch 62, ``model`` and ``model_index`` framed."""
    L = _lib()
    world = grid(h, w)
    how = dict(budgets=(25, 1, 30), spt=7, batch=62, trial_cap=2)
    expect = {L.TAB_KERNEL_WPI}
    make = lambda: make_dynaq(world, 3)
    if form == 'mask':      # (with the visit counters and the response counts)
        how['mask'] = _bump_mask(world)
        make = lambda: make_dynaq(world, 3, track_occupancy=True, track_responses=True)
    elif form == 'episodic':
        how['extra'] = L.F_EPISODIC
    elif form == 'test':
        how.update(learn=False, trial_cap=4, batch=0,
                   prior=lambda ag, env: ag.train(env, 3, 10, 62))
    elif form == 'fast':
        how.update(extra=L.F_FORCE_LDS_MODEL, budgets=(25, 2, 30))
        expect = {L.TAB_KERNEL_WPI_FAST}
    elif form == 'index':
        how['budgets'] = (25, 2, 30)
        expect = {L.TAB_KERNEL_WPI_INDEX}
    elif form == 'psets':
        how['budgets'] = (25, 2, 30)
        expect = {L.TAB_KERNEL_WPI_INDEX}
        make = lambda: make_dynaq(world, 3, eps=np.array([0.1, 0.3, 0.5]),
                                  alpha=np.array([0.5, 0.9, 0.25]))
    elif form == 'last_exp':
        how.update(budgets=(1,) * 24, spt=5)
    ag, out, _ = twin(make, expect, **how)
    if form != 'test':
        assert int(out['batches_done'].item()) > 0, 'no planning batch was evaluated'
    if form == 'psets':
        assert ag._pset_n == 3
    if form == 'last_exp':
        assert out['last_exp'][-1].any()


# -- persistent workgroups ---------------------------------------------------------------------------
def _pwg_n(side, extra):
    """Wave slots of the chip + 1 for this world: one wave of the last workgroup gets a second
    instance, the others of that workgroup none."""
    L = _lib()
    env, ag = make_dynaq(grid(side, side), 1)
    ag.extra_flags = extra
    ag._bind(env)
    ag._env_in(env)
    ag.monitors.reserve(2, 1, True)
    flags = L.F_LEARN | ag._policy_in(ag.policy, env, False)
    what = ag.describe_launch(env, ag.policy, flags, BIG_T, 9, 40, 50)
    assert what['kernel'] == L.TAB_KERNEL_PWG, what
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * what['instances_per_workgroup'] + 1, what['instances_per_workgroup']


@pytest.mark.parametrize('side,stripes', [(27, 1), (31, 3), (32, 1), (32, 3)])
def test_pwg_lds_waves(side, stripes):
    """k_tab_pwg with Q staged in LDS: 729 states (odd, no multiple of 4 or 64; the smallest odd
    square the plan gives to this kernel — up to 25 x 25 sixteen tables fit a CU and k_tab_wpi
    stays), 961 and 1 024; the last block of 64 rows is partial in the first two.  Budgets below 64
    steps keep the launches whole."""
    pwg_lds_case(side, stripes)


def pwg_lds_case(side, stripes):
    L = _lib()
    n, waves = _pwg_n(side, 0)
    ag, out, what = twin(lambda: make_dynaq(grid(side, side), n), {L.TAB_KERNEL_PWG},
                         budgets=(40, 23, 40), spt=9, batch=50, trial_cap=3, stripes=stripes)
    assert what['instances_per_workgroup'] == waves and n % waves == 1
    assert what['lds_bytes'] == waves * side * side * 16, 'not every wave keeps its Q in LDS'
    assert int(out['batches_done'].item()) > 0
    assert int(ag._scratch[128:192].sum().item()) == 0, 'the launch was sliced'
    return waves


def test_pwg_lds_waves_at_17x17_in_a_child_process():
    """289 states, the smallest table k_tab_pwg stages (its last block of 64 rows holds 33).  The
    plan gives such a world to k_tab_wpi — sixteen tables fit a CU — and LDS waves exist there under
    COBEL_DEBUG_PWG only, which the library reads once per process: the same case, sixteen LDS
    waves forced, in a process of its own."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    paths = [os.path.join(ROOT, 'tests'), ROOT, os.path.join(ROOT, 'cobel-rl_amd')]
    code = ('import sys; sys.path[:0] = %r\n'
            'import test_gpu_frames_tabular as T\n'
            'assert T.pwg_lds_case(17, 1) == 16\n'
            'print("CASE_OK")\n' % (paths,))
    env = dict(os.environ, COBEL_DEBUG='1', COBEL_DEBUG_PWG='16,0')
    done = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                          timeout=120)
    assert done.returncode == 0 and 'CASE_OK' in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


@pytest.mark.parametrize('side', [17, 32])
def test_pwg_global_memory_waves(side):
    """COBEL_F_PWG_GLOBAL: sixteen waves per workgroup work on Q in place (289 states: the first
    size the kernel takes at all)."""
    L = _lib()
    ag, out, what = twin(lambda: make_dynaq(grid(side, side), 17, extra_flags=L.F_PWG_GLOBAL),
                         {L.TAB_KERNEL_PWG}, budgets=(40, 23, 40), spt=9, batch=50, trial_cap=3)
    assert what['instances_per_workgroup'] == 16
    assert int(out['batches_done'].item()) > 0


def test_pwg_sliced_launch():
    """A launch handed out in slices of an instance's steps: rings and ticket counters live in a
    scratch area of exactly COBEL_TAB_SCRATCH_BYTES(n) bytes, framed."""
    L = _lib()
    n = 2600
    ag, out, _ = twin(lambda: make_dynaq(grid(32, 32), n), {L.TAB_KERNEL_PWG}, budgets=(67, 67),
                      spt=9, batch=50, trial_cap=3)
    assert ag._scratch.numel() * 4 == L.tab_scratch_bytes(n)
    # every instance was appended to its queue's ring once per slice after the first (`tail`,
    # word 128 + 8 q of the area): the launch was in fact sliced
    tails = ag._scratch[128:192].cpu().numpy().reshape(8, 8)[:, 0]
    assert tails.sum() >= n and tails.sum() % n == 0, tails
    assert int(ag._scratch[L_ABORT].item()) == 0
    assert int(out['batches_done'].item()) > 0


# -- other action counts -----------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('A', [1, 3, 6, 8, 9, 17, 32])
def test_wqn_rows_padded_in_lds(A, masked):
    """k_tab_wqn: rows padded to 8, 16 or 32 values in LDS are written back A wide; the replay log
    is exactly full three steps before the end, so the last appends must be dropped; word masks
    (A > 8) and byte masks framed.  One instance more than whole workgroups."""
    L = _lib()
    S = 40
    nodes = graph(S, A, 100 + A)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * cus + 1
    budgets = (7, 33, 5)
    cap = sum(budgets) - 3
    mask = None
    if masked:
        r = np.random.default_rng(7 * A)
        mask = r.random((S, A)) < 0.6
        mask[np.arange(S), r.integers(0, A, S)] = True
        mask[S - 1, A - 1] = True
    ag, out, what = twin(lambda: make_q(nodes, n, topology=True), {L.TAB_KERNEL_WQN},
                         budgets=budgets, spt=11, batch=16, trial_cap=2, log_cap=cap, mask=mask)
    assert what['instances_per_workgroup'] > 1 and n % what['instances_per_workgroup'] == 1
    assert tuple(ag._q.shape) == (n, S, A)
    assert (out['inst'][:, L.I_LOG_LEN] == cap).all(), 'the log is not exactly full'
    assert ag.env_steps() == n * sum(budgets)
    assert int(out['batches_done'].item()) > 0


def test_wqn_parameter_sets():
    L = _lib()
    pr = np.random.default_rng(5)
    n = 1025
    eps, alpha, gamma = (pr.choice([0.05, 0.2, 0.5], n), pr.choice([0.25, 0.5, 0.75], n),
                         pr.choice([0.75, 0.875], n))
    ag, out, _ = twin(lambda: make_q(graph(40, 6, 106), n, eps=eps, alpha=alpha, gamma=gamma,
                                     topology=True), {L.TAB_KERNEL_WQN}, budgets=(7, 33, 5),
                      spt=11, batch=16, trial_cap=2, log_cap=45)
    assert ag._pset_n > 4


# -- the general kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['dynaq_a4', 'q_a4', 'q_a6', 'dynaq_90x90', 'q_two_word_log'])
def test_general_kernel(case):
    """k_tab_general under ``force_general`` (and by itself where Q exceeds the LDS): four and six
    actions, one-word log entries and — nine actions on more than 8 192 states — two-word ones,
    65 instances."""
    L = _lib()
    how = dict(budgets=(9, 21, 7), spt=5, batch=12, trial_cap=2)
    if case == 'dynaq_a4':
        make = lambda: make_dynaq(grid(5, 5), 65, force_general=True)
    elif case == 'q_a4':
        make = lambda: make_q(grid(5, 5), 65, force_general=True)
        how['log_cap'] = 34
    elif case == 'q_a6':
        make = lambda: make_q(graph(25, 6, 6), 65, topology=True, force_general=True,
                              track_occupancy=True, track_responses=True)
        how['log_cap'] = 34
    elif case == 'q_two_word_log':     # (nine actions, 8 200 states: two 64-bit words per entry)
        world = graph(8200, 9, 9)
        make = lambda: make_q(world, 65, topology=True, starts=['8199', '0'])
        how['log_cap'] = 34
    else:
        world = grid(90, 90)
        make = lambda: make_dynaq(world, 65)
    ag, out, _ = twin(make, {L.TAB_KERNEL_GENERAL}, **how)
    if 'log_cap' in how:
        assert (out['inst'][:, L.I_LOG_LEN] == 34).all()
        assert ag._log_words() == (2 if case == 'q_two_word_log' else 1)
        assert tuple(ag._log.shape) == (65, 34 * ag._log_words())
        assert bool(ag._log[-1, -1] != 0) or bool(ag._log[-1, -2] != 0), 'the last entry is empty'
    if case != 'dynaq_90x90':      # (8 100 states: twelve random pairs rarely meet a learned one)
        assert int(out['batches_done'].item()) > 0


# -- the Dyna-Q session calls ------------------------------------------------------------------------
def _learned(side, n):
    """A Dyna-Q agent after a short training session, for the calls between sessions."""
    env, ag = make_dynaq(grid(side, side), n)
    ag.train(env, 8, 40, 30)      # (long enough for a single instance to learn a few dozen pairs)
    return env, ag


def _session_arrays(ag):
    return {k: v.clone() for k, v in dict(q=ag._q, model=ag.M.table, index=ag.M.index,
                                          inst=ag.inst, counter=ag.M.counter).items()}


def _swap_session(frames, ag):
    frames.swap(ag, '_q', fc.BIG)
    frames.swap(ag, 'inst', fc.inst_poison())
    frames.swap(ag.M, 'table', fc.MODEL_POISON)
    frames.swap(ag.M, 'index', fc.INDEX_POISON)


@pytest.mark.parametrize('side', [5, 17])
@pytest.mark.parametrize('n', [1, 65])
@pytest.mark.parametrize('lane', [False, True])
def test_dynaq_replay_between_sessions(lane, n, side):
    """cobel_dynaq_replay in its WAVE and LANE forms: three batches of 1, 62 and 100 pairs."""
    L = _lib()
    outs = []
    for framed in (False, True):
        env, ag = _learned(side, n)
        if lane:
            ag.extra_flags = L.F_REPLAY_LANE
        frames = fc.Frames()
        if framed:
            _swap_session(frames, ag)
        before = ag._q.clone()
        for batch in (1, 62, 100):
            assert ag.replay_plan(batch, 3)['form'] == ('lane' if lane else 'wave')
            ag.replay(batch, 3)
        torch.cuda.synchronize()
        if framed:
            frames.check()
        outs.append(_session_arrays(ag))
        assert not torch.equal(before[-1], ag._q[-1]), 'planning changed nothing in the last instance'
        assert int(ag.M.counter.min().item()) >= 9
    fc.assert_same(*outs)


@pytest.mark.parametrize('side', [5, 17])
@pytest.mark.parametrize('n', [1, 65])
@pytest.mark.parametrize('planning', [False, True])
def test_dynaq_update_and_model_store(planning, n, side):
    """cobel_dynaq_update (both forms, ``td[N]`` framed, instances without an experience, one
    experience outside the tables) and cobel_model_store with and without the digest."""
    L = _lib()
    S = side * side
    r = np.random.default_rng(n + side)
    exp = np.zeros((n, 6), dtype=np.int32)
    exp[:, 0] = r.integers(0, S, n)
    exp[:, 1] = r.integers(0, 4, n)
    exp[:, 2] = r.integers(0, S, n)
    exp[:, 3] = r.integers(0, 2, n)
    exp[:, 4] = r.choice([1.0, -0.5, 0.25], n).astype(np.float32).view(np.int32)
    exp[-1, :3] = (S - 1, 3, S - 2)                 # the last instance writes its last row
    if n > 1:
        exp[::7, 0] = -1                            # no experience
        exp[3, 0], exp[5, 1], exp[8, 2] = S, 4, S   # pairs outside the tables: skipped
    outs = []
    for framed in (False, True):
        env, ag = _learned(side, n)
        frames = fc.Frames()
        exps = torch.as_tensor(exp, device='cuda')
        td = torch.full((n,), -3.0, dtype=torch.float64, device='cuda')
        if framed:
            _swap_session(frames, ag)
            exps = frames.add('exps', exps, [0, 0, 0, 1, int(np.float32(fc.BIG).view(np.int32)), 0])
            td = frames.add('td', td, fc.BIG)
        before = ag._q.clone()
        run = ag._table_run('update_q')
        L.check(L.lib().cobel_dynaq_update(ag._handle.ptr, C.byref(run), L.ptr(exps),
                                           L.UPDATE_PLANNING if planning else L.UPDATE_ONLINE,
                                           L.ptr(td), L.current_stream(ag.device)))
        stream = L.current_stream(ag.device)
        L.check(L.lib().cobel_model_store(L.ptr(ag.M.table), L.ptr(ag.M.index), n, S, L.ptr(exps),
                                          0.5, stream))
        L.check(L.lib().cobel_model_store(L.ptr(ag.M.table), None, n, S, L.ptr(exps), 0.5, stream))
        torch.cuda.synchronize()
        if framed:
            frames.check()
        out = _session_arrays(ag)
        out['td'] = td.clone()
        outs.append(out)
        assert float(td[-1].item()) != -3.0 and not torch.equal(before[-1, S - 1], ag._q[-1, S - 1])
        rec = int(ag.M.table[-1, S - 1, 3].item())
        assert (rec >> 32) & 0xFFFF == S - 2, 'the model record of the last pair was not stored'
        if n > 1:
            assert float(td[0].item()) == 0.0, 'td of an instance without an experience'
    fc.assert_same(*outs)


@pytest.mark.parametrize('S', [25, 289])
@pytest.mark.parametrize('n', [1, 65])
def test_model_init_and_index_build(n, S):
    L = _lib()
    model = fc.frame(torch.full((n, S, 4), -1, dtype=torch.int64, device='cuda'), fc.MODEL_POISON)
    index = fc.frame(torch.full((n, S, 4), -1, dtype=torch.int16, device='cuda'), fc.INDEX_POISON)
    L.check(L.lib().cobel_model_init(L.ptr(model.view), n, S, None))
    L.check(L.lib().cobel_model_index_build(L.ptr(model.view), L.ptr(index.view), n, S, None))
    torch.cuda.synchronize()
    assert model.intact() and index.intact()
    # R = 0, NS[s][a] = s, nonterminal = 0 — and the digest of exactly that — in every cell
    want = (torch.arange(S, device='cuda').view(1, S, 1) << 32).expand(n, S, 4)
    assert torch.equal(model.view, want)
    assert torch.equal(index.view, torch.arange(S, device='cuda').view(1, S, 1).expand(n, S, 4)
                       .to(torch.int16))


# -- alignment ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['wpi_index', 'pwg_lds', 'wqn'])
def test_tables_sixteen_bytes_off_a_256_byte_boundary(form):
    """The allocator hands out 512-byte-aligned blocks; the header promises 16 bytes for Q and 8
    for the other tables, and the widest access of the kernels is 16 bytes at a multiple of 16 from
    a table's base (float4 rows, the 16-byte LDS loads of k_tab_pwg).  Every framed table of these
    runs starts 16 bytes behind a 256-byte boundary; same four assertions."""
    L = _lib()
    if form == 'wpi_index':
        ag, out, _ = twin(lambda: make_dynaq(grid(7, 9), 3), {L.TAB_KERNEL_WPI_INDEX},
                          budgets=(25, 2, 30), spt=7, batch=62, trial_cap=2, shift=16)
    elif form == 'pwg_lds':
        n, _ = _pwg_n(31, 0)
        ag, out, _ = twin(lambda: make_dynaq(grid(31, 31), n), {L.TAB_KERNEL_PWG},
                          budgets=(40, 23, 40), spt=9, batch=50, trial_cap=3, shift=16)
    else:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        ag, out, _ = twin(lambda: make_q(graph(40, 6, 106), 4 * cus + 1, topology=True),
                          {L.TAB_KERNEL_WQN}, budgets=(7, 33, 5), spt=11, batch=16, trial_cap=2,
                          log_cap=42, shift=16)
    assert ag._q.data_ptr() % 256 == 16 and ag.inst.data_ptr() % 256 == 16
    assert int(out['batches_done'].item()) > 0


@pytest.mark.parametrize('off', [1, 2])
def test_a_model_digest_off_its_eight_bytes_is_refused(off):
    """``model_index`` is declared as 16-bit entries, but k_tab_pwg reads a state's four as one
    64-bit word: cobel_tab_run (and cobel_tab_describe) refuse a digest that is not 8-byte aligned
    instead of running on it."""
    L = _lib()
    env, ag = make_dynaq(grid(5, 5), 3)
    ag._bind(env)
    ag._env_in(env)
    flags = L.F_LEARN | ag._policy_in(ag.policy, env, False)
    ag.monitors.reserve(2, 3, True)
    big = torch.zeros(ag.M.index.numel() + 4, dtype=torch.int16, device=ag.device)
    ag.M.index = big[off:off + ag.M.index.numel()].view(ag.M.index.shape)
    assert ag.M.index.data_ptr() % 8 == 2 * off
    with pytest.raises(AssertionError, match='8-byte aligned'):
        ag.describe_launch(env, ag.policy, flags, BIG_T, 7, 30, 20)
    with pytest.raises(AssertionError, match='8-byte aligned'):
        ag._launch(env, ag.policy, flags, BIG_T, 7, 30, 20)
    torch.cuda.synchronize()
    assert not ag._q.any() and ag.env_steps() == 0, 'a refused run did something'
