"""TEST INFRASTRUCTURE: QAgent and DynaQ on a Gridworld or a Topology with a Softmax, an
ExclusiveEpsilonGreedy or a RandomDiscrete policy (policy/softmax.py, policy/greedy.py:91-147,
policy/random.py:13-75 of the reference).  The three policies restated in NumPy on a ``TapeRNG`` in
the device's order of operations (csrc/tabular_policy.hip), plugged into ``RefQAgent`` / ``RefDynaQ``
of oracle/ref_loop.py; the cases of tests/golden/tabpol_traces.npz; the worlds; the fillers of
``cobel_tab_policy_run_t``.  Reads only oracle/.

Deliberate differences from the reference, both in the last bits of a Softmax probability only (as
tests/qseq_common.py has them): the sum of the exponentials runs in action order, where NumPy adds
eight values pairwise (up to seven it adds them in order too), and the device's ``exp`` is not
NumPy's.  A draw at least ``MARGIN`` away from every edge of its CDF selects the same action either
way; then every action, reward, table, log entry and counter is the reference's bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import ref_loop
from oracle.philox import STREAM_AUX, STREAM_ENV, STREAM_MEMORY, STREAM_POLICY, TapeRNG

SEED = 0xC0BE1
MARGIN = 1e-9            # the traces: every draw at least this far from every edge of its CDF
SWEEP_MARGIN = 1e-12     # the sweeps of the GPU module: what equality on the device may hinge on
TRIALS, STEPS = 6, 20

SOFTMAX, EXCLUSIVE, RANDOM = 'softmax', 'exclusive', 'random'


# -- the policies ---------------------------------------------------------------------------------------
def softmax_probs(v, beta, mask=None) -> np.ndarray:
    """policy/softmax.py:77-86 in float64, the sum in action order."""
    v = np.asarray(v, dtype=np.float64)
    on = np.ones(len(v), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    e = np.zeros(len(v))
    e[on] = np.exp((v[on] - np.amax(v[on])) * beta)
    total = 0.0
    for x in e:
        total = total + x
    return np.where(on, e / total, 0.0)


def exclusive_probs(v, epsilon, mask=None) -> np.ndarray:
    """policy/greedy.py:137-147: the reference's operations in the reference's order."""
    v = np.asarray(v, dtype=np.float64)
    on = np.ones(len(v), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    p = np.zeros(len(v))
    ties = np.amax(v[on]) == v[on]
    n_ties = int(np.sum(ties))
    t = ties.astype(np.float64)
    p[on] = ((1.0 - epsilon) * t) / float(n_ties)
    p[on] = p[on] + (epsilon * (1.0 - t)) / float(max(int(on.sum()) - n_ties, 1))
    return p


def cdf_of(p) -> np.ndarray:
    """cumsum(p) / cumsum(p)[-1], the cumulative sum in order (Generator.choice)."""
    run, cum = 0.0, []
    for a, x in enumerate(p):
        run = float(x) if a == 0 else run + float(x)
        cum.append(run)
    return np.array(cum) / cum[-1]


class RefPolicy:
    """One of the three policies on a tape; ``margin`` keeps the least distance between a draw and
    an edge of the CDF it was compared with."""

    def __init__(self, kind, par, rng, n_actions=None):
        self.kind, self.par, self.rng, self.n_actions = kind, par, rng, n_actions
        self.margin = float('inf')
        self.underflowed = False

    def get_action_probs(self, v, mask=None):
        if self.kind == RANDOM:
            return np.full(self.n_actions, 1.0 / self.n_actions)
        return (softmax_probs if self.kind == SOFTMAX else exclusive_probs)(v, float(self.par), mask)

    def select_action(self, v, mask=None):
        if self.kind == RANDOM:
            return int(self.rng.integers(self.n_actions))
        p = self.get_action_probs(v, mask)
        if self.kind == SOFTMAX and np.any((p == 0.0) & (True if mask is None else np.asarray(mask, dtype=bool))):
            self.underflowed = True      # an exponential of an action on offer came out as exact zero
        cdf = cdf_of(p)
        u = self.rng.random()
        if len(cdf) > 1:
            self.margin = min(self.margin, float(np.abs(cdf[:-1] - u).min()))
        return int(np.searchsorted(cdf, u, side='right'))


def make_policy(spec, rng, n_actions):
    """spec = (kind, parameter): a ``RefPolicy``, or the restated EpsilonGreedy for ('eps', e)."""
    kind, par = spec
    if kind == 'eps':
        return ref_loop.RefEpsilonGreedy(par, rng)
    return RefPolicy(kind, par, rng, n_actions)


# -- worlds ---------------------------------------------------------------------------------------------
def grid4(tools):
    """4 x 4 gridworld, one wall, one terminal goal, by a ``gridworld_tools`` module (the project's
    or the reference's)."""
    return tools.make_gridworld(4, 4, terminals=[3], rewards=np.array([[3, 1.0]]), goals=[3],
                                invalid_states=[5], starting_states=[12, 15, 8])


def hex_nodes(tools):
    """The smallest hexagonal lattice with a node that has all six neighbours: hexagonal(3), eight
    nodes of which seven are starting nodes; the goal is the terminal node the builder picks."""
    return tools.hexagonal(3, (0.0, 1.0), 1.0, None)


def ring_nodes(n_nodes: int, n_actions: int, goal=True):
    """A hand-made graph of ``n_actions`` neighbours per node (the library's track builders list
    four): action j of node i leads to node (i + 1 + j) % n, the last node is the terminal goal."""
    nodes = {}
    for i in range(n_nodes):
        nodes[str(i)] = {'pose': (float(i), 0.5 * i, 0.0, 1.0, 0.0, 0.0),
                         'neighbors': [str((i + 1 + j) % n_nodes) for j in range(n_actions)],
                         'terminal': bool(goal and n_nodes > 1 and i == n_nodes - 1),
                         'reward': 1.0 if (goal and i == n_nodes - 1) else 0.0}
    return nodes, [k for k, nd in nodes.items() if not nd['terminal']]


def node_tables(nodes, starts) -> dict:
    ids = list(nodes.keys())
    index = {k: i for i, k in enumerate(ids)}
    return dict(next=np.array([[index[m] for m in nodes[k]['neighbors']] for k in ids], dtype=np.uint16),
                reward=np.array([nodes[k]['reward'] for k in ids], dtype=np.float64),
                terminal=np.array([bool(nodes[k]['terminal']) for k in ids]).astype(np.uint8),
                starts=np.array([index[k] for k in starts], dtype=np.uint16))


def world_tables(world) -> dict:
    nxt = world['next'] if 'next' in world else np.argmax(world['sas'], axis=2)
    return dict(next=np.asarray(nxt).astype(np.uint16),
                reward=np.asarray(world['rewards'], dtype=np.float64),
                terminal=(np.asarray(world['terminals']) != 0).astype(np.uint8),
                starts=np.asarray(world['starting_states']).astype(np.uint16))


def two_action_mask(next_table) -> np.ndarray:
    """An action mask that removes two actions (left and down: the goal of ``grid4`` lies up and to
    the right) in the states of even index."""
    m = np.ones(np.asarray(next_table).shape, dtype=bool)
    m[0::2, 0] = False
    m[0::2, 3] = False
    return m


# -- the cases of the fixture ------------------------------------------------------------------------------
# name: world, agent, policy, batch, instance, options
CASES = {
    'q_soft05': ('grid4', 'q', (SOFTMAX, 0.5), 8, 0, {}),
    'q_soft5': ('grid4', 'q', (SOFTMAX, 5.0), 8, 1, {}),
    'q_excl': ('grid4', 'q', (EXCLUSIVE, 0.3), 8, 2, {}),
    'q_random': ('grid4', 'q', (RANDOM, None), 8, 3, {}),
    'dynaq_soft05': ('grid4', 'dynaq', (SOFTMAX, 0.5), 8, 4, {}),
    'dynaq_soft5': ('grid4', 'dynaq', (SOFTMAX, 5.0), 8, 5, {}),
    'dynaq_excl': ('grid4', 'dynaq', (EXCLUSIVE, 0.3), 8, 6, {}),
    'dynaq_random': ('grid4', 'dynaq', (RANDOM, None), 8, 7, {}),
    'dynaq_soft_mask': ('grid4', 'dynaq', (SOFTMAX, 2.0), 8, 8, {'mask': True}),
    'dynaq_soft_noreplay': ('grid4', 'dynaq', (SOFTMAX, 2.0), 0, 9, {'no_replay': True}),
    'q_soft_hex': ('hex', 'q', (SOFTMAX, 2.0), 8, 10, {}),
    'dynaq_soft_then_eps': ('grid4', 'dynaq', (SOFTMAX, 2.0), 8, 11, {'test': ('eps', 0.1)}),
}
KEYS = ('world', 'agent', 'policy', 'batch', 'inst', 'opt')


def case(name) -> dict:
    return dict(zip(KEYS, CASES[name]))


def case_tables(c, grid_tools, topo_tools) -> dict:
    if c['world'] == 'hex':
        return node_tables(*hex_nodes(topo_tools))
    return world_tables(grid4(grid_tools))


# -- one instance, restated ---------------------------------------------------------------------------------
def pack_log(M, n_actions: int) -> np.ndarray:
    """A list of (state, action, reward, next state, non-terminal) as the words of
    ``cobel_tab_run_t.replay_log`` (one per entry; worlds of up to eight actions)."""
    out = np.zeros(len(M), dtype=np.uint64)
    for k, (s, a, r, ns, nt) in enumerate(M):
        hi = int(s) | (int(ns) << 14) | (int(a) << 28) | (int(nt) << (30 if n_actions <= 4 else 31))
        out[k] = int(np.float32(r).view(np.uint32)) | (hi << 32)
    return out


class Restated:
    """The environment, the policies and the agent of one instance (global id ``g``) on fresh tapes."""

    def __init__(self, tabs, agent, policy, g, seed=SEED, test_policy=None, alpha=None, gamma=None,
                 mask=None):
        S, A = np.asarray(tabs['next']).shape
        self.S, self.A, self.kind, self.seed, self.g = S, A, agent, seed, g
        self.env = ref_loop.RefGridworld(tabs, TapeRNG(seed, g, STREAM_ENV))
        self.policies = []
        self.pol = self.policy_object(policy, STREAM_POLICY)
        self.pol_test = None if test_policy is None else self.policy_object(test_policy, STREAM_AUX)
        self.mem_rng = TapeRNG(seed, g, STREAM_MEMORY)
        kw = {}
        if alpha is not None:
            kw['learning_rate'] = float(alpha)
        if gamma is not None:
            kw['gamma'] = float(gamma)
        if agent == 'dynaq':
            self.ag = ref_loop.RefDynaQ(S, A, self.pol, self.mem_rng, dtype=np.float32,
                                        policy_test=self.pol_test, **kw)
        else:
            self.ag = ref_loop.RefQAgent(S, A, self.pol, self.mem_rng, dtype=np.float32,
                                         policy_test=self.pol_test, **kw)
        if mask is not None:
            self.ag.mask_actions, self.ag.action_mask = True, np.asarray(mask, dtype=bool)
        self.trace = ref_loop.new_trace(with_q=True)

    def policy_object(self, spec, stream):
        """A further policy object of this instance on a tape of its own from counter 0: STREAM_POLICY
        for one that trains, STREAM_AUX (the device's STREAM_POLICY_TEST) for a ``policy_test``."""
        pol = make_policy(spec, TapeRNG(self.seed, self.g, stream), self.A)
        self.policies.append(pol)
        return pol

    def session(self, pol, trials, steps, batch, learn, no_replay=False):
        """One session that selects with the policy object ``pol``, assigned to the agent as
        ``policy`` (a training session) or ``policy_test`` (a test session) for its duration."""
        keep = self.ag.policy, self.ag.policy_test
        if learn:
            self.ag.policy = pol
            self.train(trials, steps, batch, no_replay)
        else:
            self.ag.policy_test = pol
            self.test(trials, steps)
        self.ag.policy, self.ag.policy_test = keep

    def edit_world(self, tabs):
        """The environment reads its tables at every step and reset: replace them between sessions."""
        e = self.env
        assert np.asarray(tabs['next']).shape == (self.S, self.A)
        e.next, e.reward = np.asarray(tabs['next']), np.asarray(tabs['reward'], dtype=np.float64)
        e.terminal, e.starts = np.asarray(tabs['terminal']), np.asarray(tabs['starts'])

    def train(self, trials, steps, batch, no_replay=False):
        if self.kind == 'dynaq':
            self.ag.train(self.env, trials, steps, batch, no_replay, trace=self.trace)
        else:
            self.ag.train(self.env, trials, steps, batch, trace=self.trace)

    def test(self, trials, steps):
        self.ag.test(self.env, trials, steps, trace=self.trace)

    def margin(self) -> float:
        return min(getattr(p, 'margin', float('inf')) for p in self.policies)

    def record(self) -> dict:
        tr = self.trace
        a = np.array(tr['sarsn'], dtype=np.float64).reshape(-1, 5)
        d = dict(state=a[:, 0].astype(np.int16), action=a[:, 1].astype(np.int8), reward=a[:, 2],
                 next_state=a[:, 3].astype(np.int16), nonterminal=a[:, 4].astype(np.int8),
                 td=np.array(tr['td'], dtype=np.float64), steps=np.array(tr['steps'], dtype=np.int32),
                 trial_reward=np.array(tr['trial_reward'], dtype=np.float64),
                 Q_trial=np.array(tr['Q_trial'], dtype=np.float32), Q=np.array(self.ag.Q, dtype=np.float32),
                 ctr_env=np.int64(self.env.rng.index), ctr_policy=np.int64(self.pol.rng.index),
                 ctr_policy_test=np.int64(0 if self.pol_test is None else self.pol_test.rng.index),
                 ctr_memory=np.int64(self.mem_rng.index), margin=np.float64(self.margin()),
                 env_state=np.int64(self.env.current_state))
        if self.kind == 'dynaq':
            d.update(M_rewards=np.array(self.ag.M.rewards, dtype=np.float32),
                     M_states=self.ag.M.states.astype(np.int16),
                     M_terminals=self.ag.M.terminals.astype(np.int8))
        else:
            d['log'] = pack_log(self.ag.M, self.A)
        return d


def restate_case(name, tabs) -> dict:
    c = case(name)
    opt = c['opt']
    mask = two_action_mask(tabs['next']) if opt.get('mask') else None
    r = Restated(tabs, c['agent'], c['policy'], c['inst'], test_policy=opt.get('test'), mask=mask)
    r.train(TRIALS, STEPS, c['batch'], bool(opt.get('no_replay')))
    n_train = len(r.trace['sarsn'])
    if opt.get('test'):
        r.test(TRIALS, STEPS)
    d = r.record()
    d['n_train_steps'] = np.int64(n_train)
    return d


EXACT = ('state', 'action', 'reward', 'next_state', 'nonterminal', 'td', 'steps', 'trial_reward',
         'Q_trial', 'Q', 'ctr_env', 'ctr_policy', 'ctr_policy_test', 'ctr_memory', 'M_rewards',
         'M_states', 'M_terminals', 'log', 'n_train_steps')
# what the records of a sweep case add (scripts/fuzz_tabpol.py): the carried state and the counters
# of the further policy objects
SWEEP_EXACT = EXACT + ('env_state', 'ctr_second', 'ctr_eps_test', 'ctr_eps_train')


# -- test sessions on the policy kernel (tests/test_gpu_tabpol_seams.py) ------------------------------------
# name: agent, training policy, policy_test (None: the default, the training policy's object), instance
TEST_TRIALS, TEST_STEPS, TEST_BATCH = 3, 12, 8
TEST_CASES = {
    'q_test_soft': ('q', (EXCLUSIVE, 0.3), (SOFTMAX, 2.0), 20),
    'q_test_excl': ('q', (SOFTMAX, 2.0), (EXCLUSIVE, 0.3), 21),
    'q_test_random': ('q', (SOFTMAX, 2.0), (RANDOM, None), 31),
    'q_test_default': ('q', (SOFTMAX, 2.0), None, 23),
    'dynaq_test_soft': ('dynaq', (EXCLUSIVE, 0.3), (SOFTMAX, 2.0), 24),
    'dynaq_test_excl': ('dynaq', (SOFTMAX, 2.0), (EXCLUSIVE, 0.3), 25),
    'dynaq_test_random': ('dynaq', (SOFTMAX, 2.0), (RANDOM, None), 26),
    'dynaq_test_default': ('dynaq', (SOFTMAX, 2.0), None, 27),
}
TEST_KEYS = ('agent', 'policy', 'test', 'inst')


def session_case(name) -> dict:
    return dict(zip(TEST_KEYS, TEST_CASES[name]))


def restated_test_case(name, tabs, g=None) -> Restated:
    """A short training session on ``grid4`` (TRIALS x STEPS), then a test session (TEST_TRIALS x
    TEST_STEPS): the instance after both."""
    c = session_case(name)
    r = Restated(tabs, c['agent'], c['policy'], c['inst'] if g is None else g, test_policy=c['test'])
    r.train(TRIALS, STEPS, TEST_BATCH)
    r.n_train = len(r.trace['sarsn'])
    r.test(TEST_TRIALS, TEST_STEPS)
    return r


def restate_test_case(name, tabs) -> dict:
    r = restated_test_case(name, tabs)
    d = r.record()
    d['n_train_steps'] = np.int64(r.n_train)
    return d


# -- the device side -------------------------------------------------------------------------------------------
def device_policy(spec, n_actions):
    from cobel_amd.policy import EpsilonGreedy, ExclusiveEpsilonGreedy, RandomDiscrete, Softmax
    kind, par = spec
    if kind == SOFTMAX:
        return Softmax(par)
    if kind == EXCLUSIVE:
        return ExclusiveEpsilonGreedy(par)
    if kind == RANDOM:
        return RandomDiscrete(n_actions)
    return EpsilonGreedy(par)


def device_env(world_name, n_envs, seed=SEED, base=0):
    """The case's world as a device environment."""
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.misc import gridworld_tools, topology_tools
    if world_name == 'hex':
        nodes, starts = hex_nodes(topology_tools)
        return Topology(nodes, starts, n_envs=n_envs, seed=seed, instance_base=base)
    return Gridworld(grid4(gridworld_tools), n_envs=n_envs, seed=seed, instance_base=base)


def device_agent(env, agent, policy, test_policy=None, alpha=None, gamma=None, mask=None):
    from cobel_amd.agent import DynaQ, QAgent
    A = int(env.action_space.n)
    kw = {}
    if alpha is not None:
        kw['learning_rate'] = alpha
    if gamma is not None:
        kw['gamma'] = gamma
    cls = DynaQ if agent == 'dynaq' else QAgent
    pol_test = None if test_policy is None else device_policy(test_policy, A)
    ag = cls(env.observation_space, env.action_space, device_policy(policy, A), pol_test, **kw)
    if mask is not None:
        ag.mask_actions, ag.action_mask = True, np.asarray(mask, dtype=bool)
    ag.track_instances = True
    return ag


def device_tables(ag, i: int, A: int) -> dict:
    """Instance i of a device agent in the restatement's terms."""
    from cobel_amd import _lib
    inst = ag.inst[i].cpu().numpy()
    d = dict(Q=ag._q[i].cpu().numpy(), ctr_env=int(inst[_lib.I_CTR_ENV]) & 0xffffffff,
             ctr_memory=int(inst[_lib.I_CTR_MEMORY]) & 0xffffffff,
             steps=ag.monitors.lat_trace[i].cpu().numpy())
    if hasattr(ag.M, 'table'):
        raw = ag.M.table[i].cpu().numpy().astype(np.int64).view(np.uint64).reshape(-1, A)
        d['M_rewards'] = (raw & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
        d['M_states'] = ((raw >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int16)
        d['M_terminals'] = ((raw >> np.uint64(48)) & np.uint64(1)).astype(np.int8)
    else:
        n = int(inst[_lib.I_LOG_LEN])
        d['log'] = ag._log[i, :n].cpu().numpy().view(np.uint64) if ag._log is not None else \
            np.zeros(0, dtype=np.uint64)
    return d


def assert_instance(ag, i, ref: Restated, batch, what=''):
    """Tables, records, counters and per-trial latencies of instance i equal the restatement's."""
    got, want = device_tables(ag, i, ref.A), ref.record()
    keys = ['Q', 'ctr_env', 'M_rewards', 'M_states', 'M_terminals', 'log']
    if batch > 0:      # (without a batch the reference still makes its empty draw; the kernels none)
        keys.append('ctr_memory')
    for k in keys:
        if k in want:
            assert np.array_equal(got[k], want[k]), '%s instance %d: %s differs' % (what, i, k)
    n = len(want['steps'])
    assert np.array_equal(got['steps'][:n], want['steps']), '%s instance %d: latencies' % (what, i)
    pol = ag.policy.counter[i].item()
    assert pol == int(want['ctr_policy']), '%s instance %d: policy counter' % (what, i)


# -- struct fillers ---------------------------------------------------------------------------------------------
class FakeWorld(C.Structure):
    """The leading fields of the library's world handle (``struct cobel_world``, csrc/cobel_common.h)
    up to the transition lists: what the argument checks of ``cobel_tab_policy_run`` read before
    they ask the runtime for a device."""
    _fields_ = [('n_states', C.c_int32), ('n_worlds', C.c_int32), ('device', C.c_int32),
                ('rec', C.c_void_p), ('starts', C.c_void_p), ('start_off', C.c_void_p),
                ('h_start_off', C.c_void_p), ('max_rewarded_states', C.c_int32),
                ('queue', C.c_void_p), ('rw', C.c_void_p), ('n_actions', C.c_int32),
                ('next_n', C.c_void_p), ('reward_s', C.c_void_p), ('terminal_s', C.c_void_p),
                ('succ_off', C.c_void_p), ('tail_', C.c_uint8 * 128)]


def fake_world(n_states=16, n_actions=4, succ_off=None) -> FakeWorld:
    w = FakeWorld()
    w.n_states, w.n_worlds, w.device, w.n_actions = n_states, 1, 0, n_actions
    w.succ_off = succ_off
    return w


class HostArrays:
    """Host arrays standing in for the device buffers of a launch that is refused before it reads
    any of them; 64-byte aligned."""

    def __init__(self, n=4, n_states=16, n_actions=4):
        def aligned(count, dtype):
            raw = np.zeros(count * np.dtype(dtype).itemsize + 64, dtype=np.uint8)
            skip = -raw.ctypes.data % 64
            return raw[skip:skip + count * np.dtype(dtype).itemsize].view(dtype)
        self.q = aligned(n * n_states * n_actions, np.float32)
        self.model = aligned(n * n_states * n_actions, np.uint64)
        self.log = aligned(n * 8, np.uint64)
        self.inst = aligned(n * 12, np.int32)
        self.mask = aligned(n_states, np.uint8)
        self.params = aligned(4, np.float64)
        self.sets = aligned(512, np.uint8)
        self.index = aligned(n, np.uint16)
        self.n = n


def fill_policy_run(_lib, arrays: HostArrays, **changes):
    """A ``cobel_tab_policy_run_t`` every check accepts, then ``changes``: ``run__<field>`` sets a
    field of the embedded run, anything else a field of the outer struct."""
    pr = _lib.TabPolicyRun()
    r = pr.run
    r.q, r.inst, r.model = arrays.q.ctypes.data, arrays.inst.ctypes.data, arrays.model.ctypes.data
    r.n, r.trial_cap, r.trials_target, r.steps_per_trial = arrays.n, 2, 2, 5
    r.agent, r.flags, r.batch = _lib.AGENT_DYNAQ, _lib.F_LEARN, 8
    r.alpha, r.gamma, r.model_lr, r.seed = 0.9, 0.9, 0.9, SEED
    pr.policy, pr.policy_param = _lib.POLICY_SOFTMAX, 2.0
    for key, value in changes.items():
        if key.startswith('run__'):
            setattr(r, key[5:], value)
        else:
            setattr(pr, key, value)
    return pr


# -- the sweeps of the GPU module (tests/test_gpu_tabpol.py), restated per instance -----------------------------
def grid4b(tools):
    """A second 4 x 4 world for stacks: another wall, another goal."""
    return tools.make_gridworld(4, 4, terminals=[12], rewards=np.array([[12, 2.0]]), goals=[12],
                                invalid_states=[6], starting_states=[3, 0, 11])


def grid4c(tools):
    """A third one: two walls, a goal with a negative reward beside a rewarded terminal."""
    return tools.make_gridworld(4, 4, terminals=[0, 10], rewards=np.array([[0, 1.0], [10, -1.0]]),
                                goals=[0], invalid_states=[9, 2], starting_states=[15, 7])


# name: worlds, agent, policy kind, instances, instance_base, batch, trials, steps, per-instance
# parameters, the instances that are restated (None: all)
SWEEPS = {
    'sets130_dynaq': (('grid4',), 'dynaq', SOFTMAX, 130, 0, 8, 3, 10, True, None),
    'sets20_q_excl': (('grid4',), 'q', EXCLUSIVE, 20, 0, 4, 3, 10, True, None),
    'tail1025_q': (('grid4',), 'q', SOFTMAX, 1025, 0, 2, 2, 4, False,
                   (0, 1, 2, 3, 4, 511, 512, 1020, 1021, 1022, 1023, 1024)),
    'two_worlds_dynaq': (('grid4', 'grid4b'), 'dynaq', SOFTMAX, 6, 0, 8, 3, 10, False, None),
    'base1000_q': (('grid4',), 'q', EXCLUSIVE, 5, 1000, 8, 3, 10, False, None),
    'a1_q': (('ring3x1',), 'q', SOFTMAX, 3, 0, 4, 3, 6, False, None),
    'a2_q': (('ring3x2',), 'q', SOFTMAX, 3, 0, 4, 3, 6, False, None),
    'a2_q_random': (('ring3x2',), 'q', RANDOM, 3, 0, 4, 3, 6, False, None),
    'a8_q': (('ring9x8',), 'q', SOFTMAX, 3, 0, 8, 3, 10, False, None),
    'a8_q_excl': (('ring9x8',), 'q', EXCLUSIVE, 3, 0, 8, 3, 10, False, None),
    's1_q': (('ring1x1',), 'q', SOFTMAX, 3, 0, 4, 2, 5, False, None),
    's1024_dynaq': (('open32',), 'dynaq', SOFTMAX, 3, 0, 8, 1, 8, False, None),
    'b0_dynaq': (('grid4',), 'dynaq', SOFTMAX, 3, 0, 0, 3, 10, False, None),
    'b1_dynaq': (('grid4',), 'dynaq', SOFTMAX, 3, 0, 1, 3, 10, False, None),
    'b62_dynaq': (('grid4',), 'dynaq', SOFTMAX, 3, 0, 62, 3, 10, False, None),
    'b0_q': (('grid4',), 'q', SOFTMAX, 3, 0, 0, 3, 10, False, None),
    'b1_q': (('grid4',), 'q', RANDOM, 3, 0, 1, 3, 10, False, None),
    'b62_q': (('grid4',), 'q', SOFTMAX, 3, 0, 62, 3, 10, False, None),
}
SWEEP_KEYS = ('worlds', 'agent', 'kind', 'n', 'base', 'batch', 'trials', 'steps', 'sets', 'check')
# the sweeps of tests/test_gpu_tabpol_seams.py: three, five and seven actions (the pad cells of a row
# at odd widths), nine instances on THREE parameter combinations (``sets`` = 3: instance i runs
# combination i % 3), three worlds with instance_base 5 (instance i lives in world (5 + i) % 3)
SEAM_SWEEPS = {
    'a3_q': (('ring9x3',), 'q', SOFTMAX, 3, 0, 8, 3, 10, False, None),
    'a3_q_excl': (('ring9x3',), 'q', EXCLUSIVE, 3, 0, 8, 3, 10, False, None),
    'a5_q': (('ring9x5',), 'q', SOFTMAX, 3, 0, 8, 3, 10, False, None),
    'a5_q_random': (('ring9x5',), 'q', RANDOM, 3, 0, 8, 3, 10, False, None),
    'a7_q': (('ring9x7',), 'q', SOFTMAX, 3, 0, 8, 6, 14, False, None),
    'a7_q_excl': (('ring9x7',), 'q', EXCLUSIVE, 3, 0, 8, 6, 14, False, None),
    'shared9_dynaq': (('grid4',), 'dynaq', SOFTMAX, 9, 0, 8, 6, 14, 3, None),
    'shared9_q_excl': (('grid4',), 'q', EXCLUSIVE, 9, 0, 8, 6, 14, 3, None),
    'three_worlds_base5_dynaq': (('grid4', 'grid4b', 'grid4c'), 'dynaq', SOFTMAX, 6, 5, 8, 6, 14, False, None),
    'three_worlds_base5_q': (('grid4', 'grid4b', 'grid4c'), 'q', EXCLUSIVE, 6, 5, 8, 6, 14, False, None),
}


def sweep(name) -> dict:
    return dict(zip(SWEEP_KEYS, SWEEPS[name] if name in SWEEPS else SEAM_SWEEPS[name]))


def sweep_world(wname, grid_tools):
    """(device-side description, compact tables) of a sweep's world."""
    if wname.startswith('ring'):
        n_nodes, n_actions = (int(x) for x in wname[4:].split('x'))
        nodes, starts = ring_nodes(n_nodes, n_actions, goal=n_nodes > 1)
        return ('nodes', nodes, starts), node_tables(nodes, starts)
    world = {'grid4': grid4, 'grid4b': grid4b, 'grid4c': grid4c,
             'open32': lambda t: t.make_open_field(32, 32, 0, 1)}[wname](grid_tools)
    return ('grid', world), world_tables(world)


def sweep_params(s) -> dict:
    """The per-instance columns of a sweep: the policy's parameter, the learning rate and the
    discount (distinct values, so that every instance is a parameter set of its own)."""
    n = s['n']
    k = np.arange(n, dtype=np.float64)
    if s['sets'] is not True and s['sets']:      # a count: that many combinations, shared
        k = k % int(s['sets'])
    par = None
    if s['kind'] == SOFTMAX:
        par = (0.5 + 0.05 * k) if s['sets'] else 2.0
    elif s['kind'] == EXCLUSIVE:
        par = (0.05 + 0.04 * k) if s['sets'] else 0.3
    alpha = (0.5 + 0.003 * k) if s['sets'] else None
    gamma = (0.6 + 0.002 * k) if s['sets'] else None
    return dict(par=par, alpha=alpha, gamma=gamma)


def restate_sweep(name, grid_tools) -> dict:
    """{instance: Restated} of a sweep, after its training session."""
    s = sweep(name)
    tabs = [sweep_world(w, grid_tools)[1] for w in s['worlds']]
    p = sweep_params(s)
    out = {}
    for i in (range(s['n']) if s['check'] is None else s['check']):
        g = s['base'] + i
        pick = lambda col: None if col is None else (col[i] if np.ndim(col) else col)   # noqa: E731
        r = Restated(tabs[g % len(tabs)], s['agent'], (s['kind'], pick(p['par'])), g,
                     alpha=pick(p['alpha']), gamma=pick(p['gamma']))
        r.train(s['trials'], s['steps'], s['batch'])
        out[i] = r
    return out
