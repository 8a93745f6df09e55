"""Vectorised gridworld environment on the HIP library.

API of the reference's ``cobel.interface.Gridworld`` (interface/gridworld.py:33-156):
``Gridworld(world, widget=None, rng=None)`` with ``step`` / ``reset`` / ``get_position`` and the
attributes ``world``, ``observation_space``, ``action_space``, ``current_state``,
``current_coordinates``, ``rng``.  Additions: ``n_envs`` independent instances advance in
lockstep on one GPU, ``world`` may be a list of same-sized worlds (instance g uses world
g % len(worlds)), and randomness comes from the counter-based streams of the library
(``seed``; a ``numpy.random.Generator`` passed as ``rng`` only donates a seed).

The transition itself is ``cobel_env_step`` / ``cobel_env_reset`` (include/cobel_hip.h); agents
from ``cobel_amd.agent`` bypass this object during ``train`` and run the fused kernels on the
same world handle and the same per-instance state.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from ..spaces import Discrete
from .interface import Interface


def _as_seed(rng) -> int:
    if rng is None:
        return int.from_bytes(os.urandom(8), 'little')
    if isinstance(rng, (int, np.integer)):
        return int(rng) & 0xFFFFFFFFFFFFFFFF
    if hasattr(rng, 'integers'):  # numpy Generator: donate 64 bits
        return int(rng.integers(0, 2**63 - 1)) & 0xFFFFFFFFFFFFFFFF
    raise AssertionError('rng must be None, an int seed or a numpy Generator')


def _stacked(worlds: list) -> dict:
    """The host arrays ``cobel_world_create_n`` / ``cobel_world_update`` take for a list of worlds,
    plus the list form of their transition rows where any of them has distributions
    (``'lists'``: offsets, successors, cumulative probabilities; else None)."""
    S = int(worlds[0]['states'])
    if not all(int(w['states']) == S for w in worlds):
        raise ValueError('worlds must have equal state counts')
    tabs = [w.compact() if hasattr(w, 'compact') else _compact(w) for w in worlds]
    out = dict(
        next=np.ascontiguousarray(np.stack([t['next'] for t in tabs]), dtype=np.uint16),
        reward=np.ascontiguousarray(np.stack([t['reward'] for t in tabs]), dtype=np.float32),
        terminal=np.ascontiguousarray(np.stack([t['terminal'] for t in tabs]), dtype=np.uint8),
        starts=np.ascontiguousarray(np.concatenate([t['starts'] for t in tabs]), dtype=np.uint16),
        off=np.zeros(len(tabs) + 1, dtype=np.int32), lists=None)
    out['off'][1:] = np.cumsum([len(t['starts']) for t in tabs])
    # worlds whose transition rows are distributions: list form for all of them (a table row
    # is a list of one successor with cumulative probability 1)
    if any('transitions' in t for t in tabs):
        offs, sts, cdfs, base = [np.zeros(1, dtype=np.uint32)], [], [], 0
        for t in tabs:
            if 'transitions' in t:
                o, st, cd = t['transitions']
            else:
                flat = np.asarray(t['next'], dtype=np.uint16).reshape(-1)
                o = np.arange(len(flat) + 1, dtype=np.uint32)
                st, cd = flat, np.ones(len(flat))
            offs.append(o[1:].astype(np.uint64) + base)
            sts.append(st)
            cdfs.append(cd)
            base += len(st)
        out['lists'] = (np.ascontiguousarray(np.concatenate(offs), dtype=np.uint32),
                        np.ascontiguousarray(np.concatenate(sts), dtype=np.uint16),
                        np.ascontiguousarray(np.concatenate(cdfs), dtype=np.float64))
    return out


_TABLES = ('next', 'reward', 'terminal', 'starts', 'off')


class WorldHandle:
    """Owns one ``cobel_world_t`` (device copies of the compact tables of 1..W worlds) and host
    copies of what it last uploaded: ``update`` compares against them and rewrites the device
    tables, in stream order, only where a world has changed."""

    def __init__(self, worlds: list, device: torch.device) -> None:
        S = int(worlds[0]['states'])
        assert all(int(w['states']) == S for w in worlds), 'worlds must have equal state counts'
        host = _stacked(worlds)
        nxt = host['next']
        assert nxt.ndim == 3 and nxt.shape[:2] == (len(worlds), S)
        self.n_states, self.n_worlds, self.device = S, len(worlds), device
        self.n_actions = int(nxt.shape[2])      # 4: gridworlds and 4-neighbour graphs
        self.ptr = C.c_void_p()
        self._create(host)
        self.stochastic = host['lists'] is not None
        self._host = host

    def _create(self, host: dict) -> None:
        _lib.check(_lib.lib().cobel_world_create_n(
            host['next'].ctypes.data, host['reward'].ctypes.data, host['terminal'].ctypes.data,
            host['starts'].ctypes.data, host['off'].ctypes.data, self.n_states, self.n_worlds,
            self.n_actions, self.device.index or 0, C.byref(self.ptr)))
        if host['lists'] is not None:
            o, st, cd = host['lists']
            _lib.check(_lib.lib().cobel_world_set_transitions(
                self.ptr, o.ctypes.data, st.ctypes.data, cd.ctypes.data, len(st)))

    def _push_tables(self, host: dict, stream) -> None:
        _lib.check(_lib.lib().cobel_world_update(
            self.ptr, host['next'].ctypes.data, host['reward'].ctypes.data,
            host['terminal'].ctypes.data, host['starts'].ctypes.data, host['off'].ctypes.data,
            stream))

    def _push_lists(self, lists, stream) -> None:
        if lists is None:
            _lib.check(_lib.lib().cobel_world_update_transitions(self.ptr, None, None, None, 0,
                                                                 stream))
        else:
            o, st, cd = lists
            _lib.check(_lib.lib().cobel_world_update_transitions(
                self.ptr, o.ctypes.data, st.ctypes.data, cd.ctypes.data, len(st), stream))

    def update(self, worlds: list, stream=None) -> bool:
        """Bring the device tables in line with ``worlds`` (``cobel_world_update`` /
        ``cobel_world_update_transitions``: launches enqueued on ``stream`` before see the old
        world, launches after it the new one; nothing waits).  Returns whether anything had to
        be pushed.  The sizes of a handle are fixed: another world count, state count or action
        count raises ``ValueError``."""
        if len(worlds) != self.n_worlds:
            raise ValueError('the handle holds %d worlds, %d were given: the device tables are '
                             'sized at construction' % (self.n_worlds, len(worlds)))
        for w in worlds:
            if int(w['states']) != self.n_states:
                raise ValueError('a world of %d states cannot replace one of %d: the device '
                                 'tables are sized at construction'
                                 % (int(w['states']), self.n_states))
        host = _stacked(worlds)
        if host['next'].shape != self._host['next'].shape:
            raise ValueError('transition table of shape %s cannot replace one of shape %s: state '
                             'and action counts are fixed at construction'
                             % (host['next'].shape[1:], self._host['next'].shape[1:]))
        if len(host['reward'][0]) != self.n_states or len(host['terminal'][0]) != self.n_states:
            raise ValueError('rewards / terminals must keep their %d entries' % self.n_states)
        pushed = False
        # (the host copies follow each push on its own: if the second one is refused the copies
        #  still say what the device holds)
        if not all(np.array_equal(host[k], self._host[k]) for k in _TABLES):
            self._push_tables(host, stream)
            self._host = dict(host, lists=self._host['lists'])
            pushed = True
        old, new = self._host['lists'], host['lists']
        if (old is None) != (new is None) or (new is not None and not all(
                np.array_equal(a, b) for a, b in zip(old, new))):
            self._push_lists(new, stream)
            self._host, self.stochastic = host, new is not None
            pushed = True
        return pushed

    def __del__(self) -> None:
        try:
            if self.ptr:
                _lib.lib().cobel_world_destroy(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def _compact(world: dict) -> dict:
    """Compact tables of a reference-style WorldDict that only carries the dense ``sas``."""
    from ..misc.gridworld_tools import is_one_hot, successor_table, transition_lists
    out = {}
    if 'sas' in world and not world.get('deterministic', True) and not is_one_hot(world['sas']):
        out['transitions'] = transition_lists(world['sas'])
    nxt = successor_table(world['sas']) if 'sas' in world else world['next']
    return dict(out, next=np.asarray(nxt, dtype=np.uint16),
                reward=np.asarray(world['rewards'], dtype=np.float32),
                terminal=(np.asarray(world['terminals']) != 0).astype(np.uint8),
                starts=np.asarray(world['starting_states'], dtype=np.uint16))


class Gridworld(Interface):
    def __init__(self, world, widget=None, rng=None, n_envs: int = 1, seed: int | None = None,
                 device=None, instance_base: int = 0) -> None:
        super().__init__(widget)
        worlds = list(world) if isinstance(world, (list, tuple)) else [world]
        # (world['deterministic'] = False makes the reference DRAW the successor from the row of
        #  sas instead of taking its argmax, gridworld.py:115-123.  With one-hot rows — all any
        #  builder produces — that is the same step; rows that are distributions travel to the
        #  library as successor lists, WorldHandle below, and the draw happens on the device)
        self.worlds = worlds
        self.world = worlds[0]
        self.n_envs = int(n_envs)
        assert self.n_envs >= 1
        self.rng = rng
        self.seed = _as_seed(rng) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.instance_base = int(instance_base)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        assert self.device.type == 'cuda', 'cobel_amd runs on a GPU; there is no CPU fallback'
        self.handle = WorldHandle(worlds, self.device)
        self.observation_space = Discrete(self.handle.n_states)
        self.action_space = Discrete(4)
        self.state = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self.env_ctr = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        self._reward = torch.zeros(self.n_envs, dtype=torch.float32, device=self.device)
        self._done = torch.zeros(self.n_envs, dtype=torch.uint8, device=self.device)
        self._coords = [np.asarray(w['coordinates'], dtype=float) for w in worlds]
        self.reset()  # the reference's constructor draws a start state too (gridworld.py:89)

    # -- live worlds ------------------------------------------------------------------------
    # The reference reads world['sas'] / ['rewards'] / ['terminals'] / ['starting_states'] on every
    # step and reset (gridworld.py:115-126, :142): edit the world between two calls and the next
    # call sees it.  Here step(), reset() and every agent session begin with sync_world().
    live_world = True   # set False to promise that the world is never edited: no comparison

    def sync_world(self) -> bool:
        """Compare the worlds (arrays edited in place, entries replaced, ``env.world`` or a member
        of ``env.worlds`` exchanged, rows of ``sas`` turned into distributions or back) with what
        the device holds and push what differs, in stream order; host-only work otherwise.
        Returns whether anything was pushed.  State and action counts are fixed
        (``ValueError``)."""
        if not self.live_world:
            return False
        if self.world is not self.worlds[0]:      # env.world = other_world
            self.worlds[0] = self.world
        pushed = self.handle.update(self.worlds, self._stream())
        self._coords = [np.asarray(w['coordinates'], dtype=float) for w in self.worlds]
        return pushed

    # -- reference surface ------------------------------------------------------------------
    @property
    def current_state(self):
        return int(self.state[0].item()) if self.n_envs == 1 else self.state

    @current_state.setter
    def current_state(self, value) -> None:
        v = torch.as_tensor(value, dtype=torch.int32)
        if v.numel() and (int(v.min()) < 0 or int(v.max()) >= self.handle.n_states):
            raise IndexError('state outside the world (%d states)' % self.handle.n_states)
        if self.n_envs == 1 and not torch.is_tensor(value):
            self.state.fill_(int(value))
        else:
            self.state.copy_(v.to(self.device))

    @property
    def current_coordinates(self):
        return self.get_position()

    def _stream(self):
        return _lib.current_stream(self.device)

    def step(self, action):
        """``(observation, reward, end_trial, truncated, logs)``; see gridworld.py:92-129."""
        self.sync_world()
        if self.n_envs == 1 and not torch.is_tensor(action):
            a = int(action)
            assert 0 <= a < 4, 'invalid action'
            act = torch.full((1,), a, dtype=torch.uint8, device=self.device)
        else:
            act = torch.as_tensor(action, device=self.device).to(torch.uint8).contiguous()
            assert act.shape == (self.n_envs,)
        # (worlds whose rows are distributions draw the successor: one double of the env stream at
        #  the counter the trial starts share; a world of tables steps as cobel_env_step does)
        _lib.check(_lib.lib().cobel_env_step_draw(
            self.handle.ptr, _lib.ptr(self.state), _lib.ptr(act), _lib.ptr(self._reward),
            _lib.ptr(self._done), _lib.ptr(self.env_ctr), self.seed, self.n_envs,
            self.instance_base, self._stream()))
        if self.n_envs == 1:
            out = torch.stack([self.state.to(torch.float64), self._reward.to(torch.float64),
                               self._done.to(torch.float64)]).cpu().numpy()[:, 0]
            return int(out[0]), np.float64(out[1]), bool(out[2]), False, {}
        return self.state, self._reward, self._done.bool(), False, {}

    def reset(self, mask=None):
        """``(observation, logs)``; uniform draw over ``starting_states`` (gridworld.py:131-145)."""
        self.sync_world()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        _lib.check(_lib.lib().cobel_env_reset(
            self.handle.ptr, _lib.ptr(self.state), _lib.ptr(m), _lib.ptr(self.env_ctr), self.seed,
            self.n_envs, self.instance_base, self._stream()))
        return self.current_state, {}

    def get_position(self):
        states = self.state.cpu().numpy()
        if self.n_envs == 1:
            return np.copy(self._coords[self.instance_base % len(self._coords)][states[0]])
        w = (self.instance_base + np.arange(self.n_envs)) % len(self._coords)
        return np.stack([self._coords[wi][s] for wi, s in zip(w, states)])

    # visualisation hooks of the reference are accepted and ignored (widget is always None here)
    def init_visualization(self) -> None:
        pass

    def update_visualization(self, logs=None) -> None:
        pass
