"""What tests/golden/gen_tab_routing.py and tests/test_gpu_routing.py share: the synthetic worlds
of the routing table and the call of ``cobel_tab_describe`` for one of its rows.

``cobel_tab_describe`` launches nothing and reads none of the run's arrays, so every array of a
row points into one small device buffer; what a row says about an array is whether it is there
and how it is aligned (``'p'``: present and aligned, ``'p+1'`` / ``'p+4'``: that many bytes off).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

POINTERS = ('q', 'model', 'model_index', 'replay_log', 'inst', 'action_mask', 'lat_sum', 'lat_cnt',
            'reward_sum', 'resp_cnt', 'lat_trace', 'occupancy', 'steps_done', 'last_exp',
            'param_sets', 'param_index', 'batches_done', 'scratch')


def make_world(lib, spec: dict) -> C.c_void_p:
    """A ring world of ``states`` states and ``actions`` actions (action a leads a + 1 states on),
    the last state rewarded and terminal, ``worlds`` copies; ``drawn``: every row a distribution
    over staying and moving."""
    S, A, W = spec['states'], spec['actions'], spec['worlds']
    s = np.arange(S)[:, None]
    nxt = np.ascontiguousarray(np.broadcast_to((s + np.arange(A)[None, :] + 1) % S, (W, S, A)),
                               dtype=np.uint16)
    reward = np.zeros((W, S), dtype=np.float32)
    terminal = np.zeros((W, S), dtype=np.uint8)
    reward[:, -1], terminal[:, -1] = 1.0, 1
    starts = np.zeros(W, dtype=np.uint16)
    off = np.arange(W + 1, dtype=np.int32)
    ptr = C.c_void_p()
    rc = lib.cobel_world_create_n(nxt.ctypes.data, reward.ctypes.data, terminal.ctypes.data,
                                  starts.ctypes.data, off.ctypes.data, S, W, A, 0, C.byref(ptr))
    assert rc == 0, lib.cobel_last_error()
    if spec['drawn']:
        pairs = W * S * A
        o = np.arange(pairs + 1, dtype=np.uint32) * 2
        st = np.empty(2 * pairs, dtype=np.uint16)
        st[0::2] = np.broadcast_to(s, (W, S, A)).reshape(-1)
        st[1::2] = nxt.reshape(-1)
        cdf = np.tile(np.array([0.5, 1.0]), pairs)
        rc = lib.cobel_world_set_transitions(ptr, o.ctypes.data, st.ctypes.data, cdf.ctypes.data,
                                             len(st))
        assert rc == 0, lib.cobel_last_error()
    return ptr


def describe(lib, _lib, world_ptr, fields: dict | None, base: int) -> dict:
    """One row: ``fields`` are the members of ``cobel_tab_run_t`` (0: not set; None: a NULL run);
    returns the code, the four numbers and, where the call is refused, the error text."""
    out = (C.c_int32 * 4)(9, 9, 9, 9)
    run = None
    if fields is not None:
        run = _lib.TabRun()
        for k, v in fields.items():
            if not v:
                continue
            if k in POINTERS:
                v = base + (int(v[2:]) if len(v) > 1 else 0)
            setattr(run, k, v)
    rc = lib.cobel_tab_describe(world_ptr, C.byref(run) if run is not None else None, out)
    row = dict(rc=rc, out=list(out))
    if rc != 0:
        row['error'] = lib.cobel_last_error().decode('utf-8', 'replace')
    return row
