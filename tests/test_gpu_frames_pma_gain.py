"""The four entry points of csrc/pma_gain.hip — ``cobel_pma_gain_batch``, ``cobel_pma_gain_seq``,
``cobel_pma_action_probs`` and ``cobel_pma_update_q`` — with every input table and every output
inside a frame of sentinels (tests/frames_common.py): guards intact, the framed run bit-equal to
the plain run, and the results those of the restatement, so the work was done.  48 and 100
backups, three instances (the last one's tables end where the guard begins), one and three
sequences per instance, shared and per-instance Q tables and sequences."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
import pma_gain_common as gc
from conftest import SEED

pytestmark = pytest.mark.gpu

POISON = {'rewards': fc.BIG, 'states': 0, 'terminals': 1, 'T': fc.BIG, 'SR': fc.BIG,
          'update_mask': 1}
# a record that decodes to a valid step: state 0, action 0, successor 0, non-terminal
REC_POISON = 0


def swap_memory(frames, mem):
    for name in mem._dev:
        frames.swap(mem._dev, name, POISON[name])
    frames.swap(mem, 'counter', fc.MARK)
    mem._policy_counter()
    frames.swap(mem.policy, 'counter', fc.MARK)
    pows = mem._power_tables(gc.MAX_SEQ)
    mem._pows = (mem._pows[0], frames.add('gamma_pow', pows, fc.BIG))


def run(case, n_seq, framed):
    from cobel_amd import _lib as L
    frames = fc.Frames() if framed else None
    add = (lambda label, t, poison: frames.add(label, t, poison)) if framed else (lambda l, t, p: t)
    mem = gc.device_memory(case, SEED, frames=(lambda m: swap_memory(frames, m)) if framed else None)
    dev, stream = mem.device, L.current_stream(mem.device)
    S, A = case['S'], case['A']
    names = ('len7', 'repeat', 'len32')[:n_seq]
    out = {}
    bits = add('action_mask', mem._mask_bits(case['mask']), (1 << A) - 1)
    for qname, stride in (('ties', 0), ('random', S * A)):
        q = add('q', torch.as_tensor(case['Q'][qname], device=dev).contiguous(), fc.BIG)
        # compute_gain_batch
        gain = add('gain', torch.full((gc.N, A * S), -1.0, dtype=torch.float64, device=dev), fc.BIG)
        m = mem._mem(None, bits)
        L.check(L.lib().cobel_pma_gain_batch(C.byref(m), L.ptr(q), stride, L.ptr(gain), stream))
        out['gain_batch/' + qname] = gain.clone()
        # compute_gain: one list for all, then one per instance (rotated)
        for per in (False, True):
            ups = [case['seqs'][k] for k in names]
            if per:
                ups = [gc.per_instance([case['seqs'][names[(k + i) % n_seq]] for i in range(gc.N)])
                       for k in range(n_seq)]
            steps, lens, max_len, is_per = mem._sequences(ups, 'frames')
            assert is_per == per
            steps = add('steps', steps, REC_POISON)
            sg = add('seq_gain', torch.full((gc.N, n_seq), -1.0, dtype=torch.float64, device=dev),
                     fc.BIG)
            m = mem._mem(None, bits, max_len)
            L.check(L.lib().cobel_pma_gain_seq(
                C.byref(m), L.ptr(q), stride, L.ptr(steps), L.ptr(lens), n_seq, max_len,
                n_seq * max_len if per else 0, L.ptr(sg), stream))
            out['gain_seq/%s/%d' % (qname, per)] = sg.clone()
    # update_q in place on the framed [N][S][A] table, a shared and a per-instance sequence
    for per in (False, True):
        q = add('q_updated', torch.as_tensor(case['Q']['random'], device=dev).contiguous(), fc.BIG)
        up = case['seqs']['len32']
        if per:
            up = gc.per_instance([case['seqs'][k] for k in ('twice', 'len32', 'len7')])
        steps, lens, max_len, _ = mem._sequences([up], 'frames')
        steps = add('update_steps', steps, REC_POISON)
        pows = mem._power_tables(max_len)[1]
        m = mem._mem()
        L.check(L.lib().cobel_pma_update_q(
            C.byref(m), L.ptr(q), L.ptr(steps), L.ptr(lens), max_len, max_len if per else 0,
            mem.learning_rate_q, pows.data_ptr(), pows.numel(), stream))
        out['update_q/%d' % per] = q.clone()
    # action_probs_batch on the tiled table, as the reference calls it
    rows = A * S
    tq = add('tiled_q', torch.as_tensor(np.tile(case['Q']['ties'], (A, 1)), device=dev).contiguous(),
             fc.BIG)
    tb = add('tiled_mask', bits.repeat(A).contiguous(), (1 << A) - 1)
    probs = add('probs', torch.full((rows, A), -1.0, dtype=torch.float64, device=dev), fc.BIG)
    L.check(L.lib().cobel_pma_action_probs(L.ptr(tq), L.ptr(tb), rows, A, gc.EPS, L.ptr(probs), stream))
    out['probs'] = probs.clone()
    torch.cuda.synchronize()
    if framed:
        frames.check()
    gc.assert_counters_rest(mem)
    out.update({k: v.clone() for k, v in mem._dev.items()})
    return out


@pytest.mark.parametrize('n_seq', [1, 3])
@pytest.mark.parametrize('name', ['small_3x4', 'demo_5x5'])
def test_pma_gain_calls_in_frames(name, n_seq):
    case = gc.build(name)
    assert case['S'] * case['A'] == {'small_3x4': 48, 'demo_5x5': 100}[name]
    plain, framed = run(case, n_seq, False), run(case, n_seq, True)
    fc.assert_same(plain, framed)
    # the work was done: the values are the restatement's
    want = gc.expected(name)
    assert np.array_equal(framed['gain_batch/ties'].cpu().numpy(), want['gain_batch/masked/ties'])
    assert np.array_equal(framed['gain_batch/random'].cpu().numpy(), want['gain_batch/masked/random'])
    cols = [gc.GAIN_SEQS.index(k) for k in ('len7', 'repeat', 'len32')[:n_seq]]
    assert np.array_equal(framed['gain_seq/random/0'].cpu().numpy(),
                          want['gain_seq/original/masked/random'][:, cols])
    assert np.array_equal(framed['update_q/0'].cpu().numpy(), want['update_q/len32'])
    assert np.array_equal(framed['probs'].cpu().numpy(), want['probs/masked'])
    assert not torch.equal(framed['update_q/1'][0], framed['update_q/0'][0])
