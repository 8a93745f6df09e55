"""A session cut in the middle of a trial continues identically whichever kernel picks it up: the
instance record (``inst``: state, step, trial, the stream counters, the trial-in-progress bit, the
trial's reward) and the trial protocol are one contract between k_tab_general, k_tab_rollout and
k_tab_pol (stated in csrc/cobel_tab_session.h).  Straight through the C ABI, every table inside
sentinel frames; a handful of launches of three instances per case."""
import ctypes as C

import numpy as np
import pytest

import frames_common as fc

pytestmark = pytest.mark.gpu

N, TRIALS, STEPS, CUT = 3, 3, 6, 4
SEED, BASE = 0xC0BE1, 5


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def grid3():
    """3 x 3 open field, actions left / up / right / down (a wall keeps the state), the far corner
    rewarded and terminal."""
    nxt = np.zeros((9, 4), dtype=np.uint16)
    for s in range(9):
        x, y = s % 3, s // 3
        nxt[s] = [s - 1 if x > 0 else s, s - 3 if y > 0 else s, s + 1 if x < 2 else s,
                  s + 3 if y < 2 else s]
    reward, terminal = np.zeros(9, dtype=np.float32), np.zeros(9, dtype=np.uint8)
    reward[8], terminal[8] = 1.0, 1
    return nxt, reward, terminal, np.array([0, 1, 3], dtype=np.uint16)


def graph4():
    """Four nodes, two neighbours each; node 3 is rewarded and terminal."""
    nxt = np.array([[1, 2], [3, 0], [0, 1], [3, 3]], dtype=np.uint16)
    reward, terminal = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.uint8)
    reward[3], terminal[3] = 1.0, 1
    return nxt, reward, terminal, np.array([0, 2], dtype=np.uint16)


WORLDS = {'grid3': grid3, 'graph4': graph4}


def make_world(lib, name):
    nxt, reward, terminal, starts = WORLDS[name]()
    off = np.array([0, len(starts)], dtype=np.int32)
    handle = C.c_void_p()
    rc = lib.cobel_world_create_n(nxt.ctypes.data, reward.ctypes.data, terminal.ctypes.data,
                                  starts.ctypes.data, off.ctypes.data, nxt.shape[0], 1, nxt.shape[1],
                                  0, C.byref(handle))
    assert rc == 0, lib.cobel_last_error()
    return handle, nxt.shape[0], nxt.shape[1]


class Session:
    """The tables of one session of N instances, each inside a sentinel frame, and the run struct
    that points at them.  ``fork()``: a second session that starts from copies of this one's state."""

    def __init__(self, torch, S, A, source=None, log=False, record=False):
        self.torch, self.S, self.A, self.frames = torch, S, A, fc.Frames()
        dev = 'cuda'
        rng = np.random.default_rng(7)
        fresh = {
            'q': torch.as_tensor(rng.standard_normal((N, S, A)).astype(np.float32), device=dev),
            'inst': torch.zeros((N, fc.INST_WORDS), dtype=torch.int32, device=dev),
            'lat_sum': torch.zeros(TRIALS, dtype=torch.int64, device=dev),
            'lat_cnt': torch.zeros(TRIALS, dtype=torch.int64, device=dev),
            'reward_sum': torch.zeros(TRIALS, dtype=torch.float64, device=dev),
            'resp_cnt': torch.zeros(TRIALS, dtype=torch.int64, device=dev),
            'lat_trace': torch.full((N, TRIALS), -1, dtype=torch.int32, device=dev),
            'steps_done': torch.zeros(1, dtype=torch.int64, device=dev),
            'batches_done': torch.zeros(1, dtype=torch.int64, device=dev),
        }
        if log:
            fresh['log'] = torch.zeros((N, TRIALS * STEPS), dtype=torch.int64, device=dev)
        poison = {'q': fc.BIG, 'inst': fc.inst_poison(), 'reward_sum': fc.BIG,
                  'log': fc.log_poison(A)}
        self.t = {}
        for k, v in fresh.items():
            init = v if source is None else source.t[k]
            self.t[k] = self.frames.add(k, init.clone(), poison.get(k, fc.MARK))
        if record:     # a rollout's record: not part of the state that is handed over
            for k, shape, dtype, mark in (('start', (N, TRIALS), torch.int16, 0),
                                          ('states', (N, TRIALS, STEPS), torch.int16, 0),
                                          ('actions', (N, TRIALS, STEPS), torch.uint8, 0),
                                          ('length', (N, TRIALS), torch.int32, fc.MARK)):
                self.t[k] = self.frames.add(k, torch.zeros(shape, dtype=dtype, device=dev), mark)

    def fork(self, **kw):
        return Session(self.torch, self.S, self.A, source=self, **kw)

    def fill(self, _lib, run, flags, budget, agent=None, batch=0):
        for k in ('q', 'inst', 'lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt', 'lat_trace',
                  'steps_done', 'batches_done'):
            setattr(run, k, self.t[k].data_ptr())
        if 'log' in self.t:
            run.replay_log, run.log_cap = self.t['log'].data_ptr(), TRIALS * STEPS
        run.n, run.trial_cap, run.instance_base = N, TRIALS, BASE
        run.agent = _lib.AGENT_Q if agent is None else agent
        run.flags, run.trials_target, run.steps_per_trial = flags, TRIALS, STEPS
        run.step_budget, run.batch = budget, batch
        run.alpha, run.gamma, run.epsilon, run.model_lr = 0.9, 0.8, 0.3, 0.9
        run.seed, run.mon_stripes = SEED, 1
        return run

    def state(self, keys):
        self.torch.cuda.synchronize()
        self.frames.check()
        return {k: self.t[k].clone() for k in keys}


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert fc.same_bits(a[k], b[k]), '%s: %s differs' % (what, k)


TEST_KEYS = ('q', 'inst', 'lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt', 'lat_trace', 'steps_done')


@pytest.mark.parametrize('world', sorted(WORLDS))
def test_a_test_session_cut_mid_trial_goes_on_in_either_kernel(torch_cuda, world):
    """EpsilonGreedy 0.3, nothing learns.  Four steps on the general kernel leave every instance
    inside a trial; cobel_tab_run (general) and cobel_tab_rollout finish the session from copies of
    that state and leave the same bytes, which are those of the uncut session."""
    from cobel_amd import _lib
    lib = _lib.lib()
    handle, S, A = make_world(lib, world)
    try:
        general = _lib.F_TAB_GENERAL

        def tab_run(session, budget):
            run = session.fill(_lib, _lib.TabRun(), general, budget)
            _lib.check(lib.cobel_tab_run(handle, C.byref(run), None))

        uncut = Session(torch_cuda, S, A)
        tab_run(uncut, 0)
        want = uncut.state(TEST_KEYS)

        head = Session(torch_cuda, S, A)
        tab_run(head, CUT)
        cut = head.state(TEST_KEYS)
        inst = cut['inst'].cpu().numpy()
        assert (inst[:, _lib.I_FLAGS] & 1).all(), 'the cut is not inside a trial'
        assert (inst[:, _lib.I_TRIAL] < TRIALS).all() and int(cut['steps_done'].item()) == N * CUT

        a = head.fork()
        tab_run(a, 0)
        b = head.fork(record=True)
        ro = _lib.TabRollout()
        b.fill(_lib, ro.run, 0, 0)
        for k in ('start', 'states', 'actions', 'length'):
            setattr(ro, k, b.t[k].data_ptr())
        ro.trials, ro.steps = TRIALS, STEPS
        _lib.check(lib.cobel_tab_rollout(handle, C.byref(ro), None))

        got_a, got_b = a.state(TEST_KEYS), b.state(TEST_KEYS)
        same(got_a, got_b, 'general against rollout')
        same(got_a, want, 'cut against uncut')
        head.frames.check()
        final = got_a['inst'].cpu().numpy()
        assert (final[:, _lib.I_TRIAL] == TRIALS).all() and not (final[:, _lib.I_FLAGS] & 1).any()
        assert int(got_a['lat_cnt'].sum().item()) == N * TRIALS
        assert fc.same_bits(got_a['q'], cut['q']), 'a test session wrote Q'
    finally:
        lib.cobel_world_destroy(handle)


def test_a_learning_policy_session_cut_mid_trial_equals_the_uncut_one(torch_cuda):
    """QAgent with a log, batch 2, ExclusiveEpsilonGreedy 0.3 on the two-action graph:
    cobel_tab_policy_run stopped after four steps and resumed leaves the Q tables, the log, the
    instance words and the monitors of the uncut call."""
    from cobel_amd import _lib
    lib = _lib.lib()
    handle, S, A = make_world(lib, 'graph4')
    keys = TEST_KEYS + ('log', 'batches_done')
    try:
        def policy_run(session, budget):
            prun = _lib.TabPolicyRun()
            session.fill(_lib, prun.run, _lib.F_LEARN, budget, batch=2)
            prun.policy, prun.policy_param = _lib.POLICY_EXCLUSIVE, 0.3
            _lib.check(lib.cobel_tab_policy_run(handle, C.byref(prun), None))

        uncut = Session(torch_cuda, S, A, log=True)
        policy_run(uncut, 0)
        want = uncut.state(keys)

        cut = Session(torch_cuda, S, A, log=True)
        policy_run(cut, CUT)
        mid = cut.state(keys)
        inst = mid['inst'].cpu().numpy()
        assert (inst[:, _lib.I_FLAGS] & 1).all(), 'the cut is not inside a trial'
        assert (inst[:, _lib.I_LOG_LEN] == CUT).all() and int(mid['steps_done'].item()) == N * CUT
        policy_run(cut, 0)
        got = cut.state(keys)
        same(got, want, 'cut against uncut')
        final = got['inst'].cpu().numpy()
        assert (final[:, _lib.I_TRIAL] == TRIALS).all() and not (final[:, _lib.I_FLAGS] & 1).any()
        assert not fc.same_bits(got['q'], mid['q']), 'nothing was learnt after the cut'
    finally:
        lib.cobel_world_destroy(handle)
