"""Tabular Dyna-Q — ``cobel.agent.DynaQ`` (agent/dyna_q.py:17-330) on the fused HIP kernel.

Same constructor, ``train(interface, trials, steps, batch_size=32, no_replay=False)``,
``test``, ``predict_on_batch`` and attributes (``Q``, ``M``, ``learning_rate``, ``gamma``,
``action_mask``, ``mask_actions``, ``episodic_replay``, ``current_trial``, ``stop``).  Tables are
float32; see include/cobel_hip.h for the exact arithmetic (bit-exact against the reference run
with float32 tables).  Up to 62 planning updates per step one wavefront plans a batch in one pass;
larger ``batch_size`` values (the reference has no limit) run as several passes of the same kernels.

``replay(batch_size, n_batches)``, ``update_q(experience)`` and ``M.store_batch(experience)`` are
the reference's three public calls (agent/dyna_q.py:193-211, :275-330) as device calls between
sessions: planning without moving, custom loops over all instances.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from ..memory import _device
from ..memory.dyna_q import DynaQMemory, _is_array, pack_experiences
from ..policy.greedy import EpsilonGreedy
from ..spaces import Discrete
from .tabular import TabularAgent


def infer_planning(experience: dict) -> bool:
    """Which arithmetic ``update_q`` takes when it is not told (see there): False = online float32,
    True = planning."""
    r, t = experience['reward'], experience['terminal']
    if any(_is_array(v) for v in experience.values()):
        return False
    return not (type(r) in (int, float, bool) and type(t) in (int, float, bool))


class DynaQ(TabularAgent):
    agent_kind = _lib.AGENT_DYNAQ
    # the model records and their digest are laid out for four actions (the reference's DynaQ takes
    # Discrete observations only — gridworlds — so other action counts cannot reach it either)
    general_actions = False

    def __init__(self, observation_space, action_space, policy, policy_test=None,
                 learning_rate: float = 0.99, gamma: float = 0.99, memory=None,
                 custom_callbacks=None) -> None:
        assert type(observation_space) is Discrete, 'DynaQ requires a discrete observation space!'
        assert type(action_space) is Discrete, 'DynaQ requires a discrete action space!'
        super().__init__(observation_space, action_space, policy, policy_test, learning_rate,
                         gamma, custom_callbacks)
        self.M = DynaQMemory(self.n_states, self.n_actions) if memory is None else memory
        self.episodic_replay = False

    def _alloc_tables(self) -> None:
        super()._alloc_tables()
        self.M._bind(self.n_envs, self.device, self._seed, self._instance_base)

    def _extra(self, run) -> None:
        run.model = _lib.ptr(self.M.table)
        run.model_index = _lib.ptr(self.M.index)
        self.inst[:, _lib.I_CTR_MEMORY] = self.M.counter

    def _model_lr(self):
        return self.M.learning_rate

    def _launch(self, interface, *args, **kwargs) -> None:
        self._handle = interface.handle      # (replay / update_q between sessions)
        super()._launch(interface, *args, **kwargs)
        self.M.counter.copy_(self.inst[:, _lib.I_CTR_MEMORY])

    # -- the reference's public calls between sessions -------------------------------------------
    def _table_run(self, what: str, batch: int = 0) -> _lib.TabRun:
        if self._q is None or getattr(self, '_handle', None) is None:
            raise RuntimeError('DynaQ.%s: the agent has no device tables yet — they are allocated '
                               'by its first train() / test() session' % what)
        run = _lib.TabRun()
        run.q, run.inst = _lib.ptr(self._q), _lib.ptr(self.inst)
        run.n, run.instance_base = self.n_envs, self._instance_base
        run.agent, run.flags, run.batch = self.agent_kind, self.extra_flags, batch
        run.seed = self._seed
        # (no selection in these calls: a policy without an epsilon hands in none)
        eps = self.policy.epsilon if type(self.policy) is EpsilonGreedy else 0.0
        self._hyper(run, self.learning_rate, self.gamma, eps, self._model_lr())
        self._extra(run)
        return run

    def replay(self, batch_size: int, n_batches: int = 1) -> None:
        """agent/dyna_q.py:319-330, ``n_batches`` times in ONE launch (the reference's call is
        ``n_batches = 1``): per batch ``batch_size`` pairs drawn from the memory stream at
        ``M.counter`` — what ``M.retrieve_batch`` and a planning step of ``train`` consume —, their
        model records, the updates in the reference's order in the planning arithmetic, the
        counter advanced by one.  Stream-ordered with sessions and with the memory's calls."""
        run = self._table_run('replay', int(batch_size))
        _lib.check(_lib.lib().cobel_dynaq_replay(self._handle.ptr, C.byref(run), int(n_batches),
                                                 _lib.current_stream(self.device)))
        self.M.counter.copy_(self.inst[:, _lib.I_CTR_MEMORY])

    def replay_plan(self, batch_size: int, n_batches: int = 1) -> dict:
        """What ``replay`` would launch (``cobel_dynaq_replay_plan``)."""
        run = self._table_run('replay_plan', int(batch_size))
        out = _device.plan4(_lib.lib().cobel_dynaq_replay_plan, self._handle.ptr, C.byref(run),
                            int(n_batches))
        return {'form': 'lane' if out[0] == _lib.REPLAY_LANE else 'wave', 'lds_bytes': int(out[1]),
                'threads_per_workgroup': int(out[2]), 'instances_per_workgroup': int(out[3])}

    def update_q(self, experience: dict, planning: bool | None = None) -> dict:
        """agent/dyna_q.py:275-301 for every instance: the values of ``experience`` are scalars
        (all instances get the same) or ``[N]`` arrays / device tensors; ``state < 0`` leaves an
        instance untouched.  Returns the experience with ``'td'``: a float for one instance, a
        float64 device tensor ``[N]`` otherwise.

        The reference's expression takes its precision from the TYPES in the dictionary, and on
        float32 tables the two cases differ in the last bit.  ``planning`` says which one to
        compute; with ``None`` it is inferred as the reference's own types decide it:

        * ``reward`` and ``terminal`` both plain Python numbers — what ``train()`` builds — : the
          online form, float32 throughout (``gamma * terminal`` first, one rounding per operation);
        * anything NumPy-typed in either — what the memories hand out (``M.retrieve_batch``) — :
          the planning form, TD in float64, one rounding into the float32 Q;
        * array-valued experiences: the online form unless ``planning=True``."""
        run = self._table_run('update_q')
        if planning is None:
            planning = infer_planning(experience)
        exps = pack_experiences(experience, self.n_envs, self.n_states, self.device)
        td = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().cobel_dynaq_update(
            self._handle.ptr, C.byref(run), _lib.ptr(exps),
            _lib.UPDATE_PLANNING if planning else _lib.UPDATE_ONLINE, _lib.ptr(td),
            _lib.current_stream(self.device)))
        experience['td'] = float(td.item()) if self.n_envs == 1 else td
        return experience

    def train(self, interface, trials: int, steps: int, batch_size: int = 32,
              no_replay: bool = False) -> None:
        assert batch_size >= 0
        extra = (_lib.F_NO_REPLAY if no_replay else 0) | \
                (_lib.F_EPISODIC if self.episodic_replay else 0)
        self._session(interface, trials, steps, batch_size, True, extra)

    def test(self, interface, trials: int, steps: int) -> None:
        self._session(interface, trials, steps, 0, False)
