"""What the rollout tests share (tests/test_host_rollout.py, tests/test_gpu_rollout.py) and what the
generator of their fixture reads (tests/golden/gen_rollout.py): the cases, the planted tables, the
worlds, a restatement of one test session per instance on the project's Philox streams, and the
fillers of ``cobel_tab_rollout_t``."""
import ctypes as C

import numpy as np

SEED = 0xC0BE1
PAD_STATE, PAD_ACTION = -1, 255

# name: world, agent, table, instance, epsilon, trials, steps, a policy_test of its own, action mask
# (the reference's QAgent has no action mask and its DynaQ takes Discrete observations only)
CASES = {
    'open5_dynaq_zeros': ('open5', 'dynaq', 'zeros', 0, 0.1, 3, 12, False, False),
    'open5_dynaq_plateau': ('open5', 'dynaq', 'plateau', 1, 0.1, 4, 20, True, False),
    'open5_dynaq_trained': ('open5', 'dynaq', 'trained', 2, 0.1, 5, 25, True, False),
    'open5_q_plateau': ('open5', 'q', 'plateau', 3, 0.3, 4, 20, False, False),
    'open5_q_trained': ('open5', 'q', 'trained', 4, 0.0, 4, 25, True, False),
    'walls8_dynaq_zeros': ('walls8', 'dynaq', 'zeros', 5, 0.1, 3, 16, True, True),
    'walls8_dynaq_plateau': ('walls8', 'dynaq', 'plateau', 6, 0.2, 4, 30, False, True),
    'walls8_dynaq_trained': ('walls8', 'dynaq', 'trained', 7, 0.1, 5, 40, False, True),
    'track4_q_zeros': ('track4', 'q', 'zeros', 8, 0.1, 3, 9, False, False),
    'track4_q_plateau': ('track4', 'q', 'plateau', 9, 0.1, 4, 9, True, False),
    'track4_q_trained': ('track4', 'q', 'trained', 10, 0.1, 5, 9, False, False),
}
TRAIN_TRIALS = 20       # the `trained` tables: that many trials of the reference's train()


def case(name) -> dict:
    keys = ('world', 'agent', 'table', 'inst', 'eps', 'trials', 'steps', 'test_policy', 'mask')
    return dict(zip(keys, CASES[name]))


# -- planted tables ------------------------------------------------------------------------------------
def plateau_table(n_states: int, n_actions: int, seed: int = 5) -> np.ndarray:
    """float32 ``[S, A]``: in every state two actions share the maximum exactly (a two-way tie the
    selection splits by the draw), the others lie below it at distinct values."""
    r = np.random.default_rng(seed)
    q = np.zeros((n_states, n_actions), dtype=np.float32)
    for s in range(n_states):
        order = r.permutation(n_actions)
        q[s, order] = np.float32(0.125) * np.arange(n_actions, dtype=np.float32)
        q[s, order[-2:]] = np.float32(0.75)
    return q


def planted_table(kind: str, n_states: int, n_actions: int):
    if kind == 'zeros':
        return np.zeros((n_states, n_actions), dtype=np.float32)
    if kind == 'plateau':
        return plateau_table(n_states, n_actions)
    return None     # 'trained': the fixture holds it


# -- worlds --------------------------------------------------------------------------------------------
WALLS_8X8 = dict(terminals=[7, 56], rewards=[[7, 1.0], [56, -0.5], [30, 0.25]], goals=[7],
                 invalid_states=[10, 11, 12, 20, 28, 36, 44, 45, 50],
                 invalid_transitions=[(0, 1), (1, 0), (62, 63), (63, 62), (33, 34)],
                 starting_states=[63, 32, 3, 27])


def grid_world(tools, name):
    """``open5`` / ``walls8`` by a ``gridworld_tools`` module — the project's or the reference's."""
    if name == 'open5':
        return tools.make_open_field(5, 5, 0, 1)
    assert name == 'walls8'
    kw = dict(WALLS_8X8, rewards=np.array(WALLS_8X8['rewards']))
    return tools.make_gridworld(8, 8, **kw)


def bump_mask(next_table) -> np.ndarray:
    """Action mask that forbids the moves which leave the state unchanged."""
    nxt = np.asarray(next_table)
    m = nxt != np.arange(nxt.shape[0])[:, None]
    m[~m.any(axis=1)] = True
    return m


def node_tables(nodes, starts) -> dict:
    """A node dictionary as the compact tables of a world (rows in the dictionary's order)."""
    ids = list(nodes.keys())
    index = {k: i for i, k in enumerate(ids)}
    return dict(next=np.array([[index[m] for m in nodes[k]['neighbors']] for k in ids],
                              dtype=np.uint16),
                reward=np.array([nodes[k]['reward'] for k in ids], dtype=np.float64),
                terminal=np.array([bool(nodes[k]['terminal']) for k in ids]).astype(np.uint8),
                starts=np.array([index[k] for k in starts], dtype=np.uint16),
                coordinates=np.array([nodes[k]['pose'] for k in ids], dtype=np.float64))


def world_tables(world) -> dict:
    """Compact tables of a grid world dictionary that carries ``next`` or the dense ``sas``."""
    nxt = world['next'] if 'next' in world else np.argmax(world['sas'], axis=2)
    return dict(next=np.asarray(nxt).astype(np.uint16),
                reward=np.asarray(world['rewards'], dtype=np.float64),
                terminal=(np.asarray(world['terminals']) != 0).astype(np.uint8),
                starts=np.asarray(world['starting_states']).astype(np.uint16),
                coordinates=np.asarray(world['coordinates'], dtype=np.float64))


# -- one test session per instance, restated -----------------------------------------------------------
def pack_session(sarsn, steps_log, trials: int, steps: int) -> dict:
    """Per-step rows (state, action, ., next state, .) and ``logs['steps']`` per trial as the four
    arrays of a record for one instance."""
    out = dict(start=np.full(trials, -1, dtype=np.int16),
               states=np.full((trials, steps), PAD_STATE, dtype=np.int16),
               actions=np.full((trials, steps), PAD_ACTION, dtype=np.uint8),
               length=np.zeros(trials, dtype=np.int32))
    at = 0
    for t in range(trials):
        n = int(steps_log[t]) + 1
        rows = sarsn[at:at + n]
        at += n
        out['start'][t] = rows[0][0]
        out['states'][t, :n] = [r[3] for r in rows]
        out['actions'][t, :n] = [r[1] for r in rows]
        out['length'][t] = n
    assert at == len(sarsn)
    return out


def restate(tabs: dict, q, instance: int, eps: float, trials: int, steps: int, test_policy: bool,
            mask=None, seed: int = SEED, sessions: int = 1, sas=None) -> list:
    """``sessions`` test sessions of one instance (global id ``instance``) after the constructor's
    start draw, in NumPy on the project's Philox streams: the loop of the reference's ``test()``
    as oracle/ref_loop.py restates it.  Returns one packed record per session."""
    from oracle import philox, ref_loop
    world = dict(tabs)
    if sas is not None:
        world['sas'] = sas
    else:
        world.pop('sas', None)
    env = ref_loop.RefGridworld(world, philox.TapeRNG(seed, instance, philox.STREAM_ENV,
                                                      double_sub=1))
    stream = philox.STREAM_AUX if test_policy else philox.STREAM_POLICY     # (AUX: POLICY_TEST)
    pol = ref_loop.RefEpsilonGreedy(eps, philox.TapeRNG(seed, instance, stream))
    n_states, n_actions = np.asarray(tabs['next']).shape
    ag = ref_loop.RefDynaQ(n_states, n_actions, pol, None, dtype=np.float32)
    ag.Q[:] = np.asarray(q, dtype=np.float32)
    if mask is not None:
        ag.mask_actions, ag.action_mask = True, np.asarray(mask, dtype=bool)
    out = []
    for _ in range(sessions):
        tr = ref_loop.new_trace()
        ag.test(env, trials, steps, trace=tr)
        out.append(pack_session(tr['sarsn'], tr['steps'], trials, steps))
    return out


# -- struct fillers ----------------------------------------------------------------------------------------
class FakeWorld(C.Structure):
    """The leading fields of the library's world handle (``struct cobel_world``, csrc/cobel_common.h)
    up to the action count: what the argument checks of ``cobel_tab_rollout`` read before they ask
    the runtime for a device.  tests/test_gpu_rollout.py holds it against a real handle."""
    _fields_ = [('n_states', C.c_int32), ('n_worlds', C.c_int32), ('device', C.c_int32),
                ('rec', C.c_void_p), ('starts', C.c_void_p), ('start_off', C.c_void_p),
                ('h_start_off', C.c_void_p), ('max_rewarded_states', C.c_int32),
                ('queue', C.c_void_p), ('rw', C.c_void_p), ('n_actions', C.c_int32),
                ('tail_', C.c_uint8 * 128)]


def fake_world(n_states=25, n_actions=4) -> FakeWorld:
    w = FakeWorld()
    w.n_states, w.n_worlds, w.device, w.n_actions = n_states, 1, 0, n_actions
    return w


class HostArrays:
    """Host arrays standing in for the device buffers of a launch that is refused before it reads
    any of them; 64-byte aligned."""

    def __init__(self, n=4, n_states=25, n_actions=4, trials=2, steps=5):
        def aligned(count, dtype):
            raw = np.zeros(count * np.dtype(dtype).itemsize + 64, dtype=np.uint8)
            skip = -raw.ctypes.data % 64
            return raw[skip:skip + count * np.dtype(dtype).itemsize].view(dtype)
        self.q = aligned(n * n_states * n_actions, np.float32)
        self.inst = aligned(n * 12, np.int32)
        self.start = aligned(n * trials, np.int16)
        self.length = aligned(n * trials, np.int32)
        self.states = aligned(n * trials * steps, np.int16)
        self.actions = aligned(n * trials * steps, np.uint8)
        self.n, self.trials, self.steps = n, trials, steps


def fill_rollout(_lib, arrays: HostArrays, **changes):
    """A ``cobel_tab_rollout_t`` every check accepts, then ``changes``: ``run__<field>`` sets a
    field of the embedded run, anything else a field of the rollout struct."""
    ro = _lib.TabRollout()
    r = ro.run
    r.q, r.inst = arrays.q.ctypes.data, arrays.inst.ctypes.data
    r.n, r.trial_cap, r.trials_target = arrays.n, arrays.trials, arrays.trials
    r.steps_per_trial, r.step_budget, r.agent, r.flags = arrays.steps, 0, _lib.AGENT_Q, 0
    r.epsilon, r.seed = 0.1, SEED
    ro.start, ro.states = arrays.start.ctypes.data, arrays.states.ctypes.data
    ro.actions, ro.length = arrays.actions.ctypes.data, arrays.length.ctypes.data
    ro.trials, ro.steps, ro.record_flags = arrays.trials, arrays.steps, 0
    for key, value in changes.items():
        if key.startswith('run__'):
            setattr(r, key[5:], value)
        else:
            setattr(ro, key, value)
    return ro
