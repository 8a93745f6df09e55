"""The routing of the tabular agents, pinned: ``cobel_tab_describe`` answers every row of
tests/golden/tab_routing.json — recorded from the commit before the routing was gathered into one
planner (tests/golden/gen_tab_routing.py) — with the same code, the same four numbers and, where
it refuses, the same text.  Nothing is launched."""
import json
import os

import pytest

from conftest import GOLDEN
from tab_routing_common import describe, make_world

# The one known difference.  Action masks of worlds with more than eight actions are 32-bit words
# and must be 4-byte aligned; that used to be checked when the general kernel was launched, so
# ``cobel_tab_describe`` described a run that ``cobel_tab_run`` then refused.  It is an argument
# check now, and both refuse it.
MASK_TEXT = ('cobel_tab_run: the action masks of a %d-action world are 32-bit words, '
             '4-byte aligned')
REFUSED_NOW = {
    's25_a9_w1/q_log_mask_misaligned': 9,
    's25_a17_w1/q_log_mask_misaligned': 17,
    's25_a32_w1/q_log_mask_misaligned': 32,
    's256_a17_w1/q_log_mask_misaligned': 17,
    's289_a17_w1/q_log_mask_misaligned': 17,
    's1024_a9_w1/q_log_mask_misaligned': 9,
    's625_a32_w1/q_log_mask_misaligned': 32,
    's256_a17_w2/q_log_mask_misaligned': 17,
}


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


@pytest.mark.gpu
def test_describe_matches_the_pinned_routing_table(torch_cuda):
    torch = torch_cuda
    from cobel_amd import _lib
    lib = _lib.lib()
    with open(os.path.join(GOLDEN, 'tab_routing.json')) as f:
        table = json.load(f)
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    handles = {name: make_world(lib, spec) for name, spec in table['worlds'].items()}
    try:
        kinds, wrong = set(), []
        for row in table['rows']:
            fields = None if row['run'] is None else dict(table['defaults'], **row['run'])
            got = describe(lib, _lib, handles.get(row['world']), fields, buf.data_ptr())
            want = {k: row[k] for k in ('rc', 'out', 'error') if k in row}
            if row['name'] in REFUSED_NOW:
                assert want == dict(rc=_lib.OK, out=[_lib.TAB_KERNEL_GENERAL, 0, 0, 64])
                want = dict(rc=_lib.E_ARG, out=[0, 0, 0, 0],
                            error=MASK_TEXT % REFUSED_NOW[row['name']])
            if got != want:
                wrong.append((row['name'], want, got))
            kinds.add((got['rc'], got['out'][0]))
        assert not wrong, '%d of %d rows differ, the first: %s' % (len(wrong), len(table['rows']),
                                                                   wrong[:5])
        # the table reaches every kernel and every kind of refusal
        assert {k for rc, k in kinds if rc == _lib.OK} == set(range(7))
        assert {rc for rc, _ in kinds} == {_lib.OK, _lib.E_ARG, _lib.E_RANGE, _lib.E_UNSUPPORTED}
        assert len(table['rows']) >= 1700
    finally:
        for h in handles.values():
            lib.cobel_world_destroy(h)
