"""tests/frames_common.py on the CPU: the frame helper notices a write one element in front of or
behind a framed table, not one inside it; the guards are as large and as aligned as promised; a
pattern poison continues a table of records by whole records on both sides."""
import numpy as np
import pytest
import torch

import frames_common as fc

DTYPES = [torch.float32, torch.float64, torch.int64, torch.int32, torch.int16, torch.uint8]


def _table(dtype, shape=(3, 7, 5)):
    n = int(np.prod(shape))
    return (torch.arange(n) % 100).to(dtype).reshape(shape)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shift', [0, 16])
def test_a_write_outside_the_view_is_seen_and_one_inside_is_not(dtype, shift):
    t = _table(dtype)
    f = fc.frame(t, 77, shift)
    size = t.element_size()
    assert f.view.shape == t.shape and f.view.dtype == dtype and torch.equal(f.view, t)
    assert f.view.device.type == 'cpu'
    assert f.intact()
    # the guards: at least 4 KiB each, the front one a multiple of 256 bytes (plus the shift asked for)
    front = f.view.data_ptr() - f.buf.data_ptr()
    back = f.buf.numel() - front - t.numel() * size
    assert front >= 4096 and back >= 4096 and (front - shift) % 256 == 0 and back % 256 == 0
    assert f.view.data_ptr() % 256 == shift
    flat = f.buf.view(dtype) if f.buf.numel() % size == 0 else None
    assert flat is not None
    first = front // size
    # inside: first and last element
    f.view.reshape(-1)[0] = 1
    f.view.reshape(-1)[-1] = 1
    assert f.intact()
    for where in (first - 1, first + t.numel(), 0, flat.numel() - 1):
        keep = flat[where].clone()
        flat[where] = 1
        assert not f.intact(), where
        assert f.damage()
        flat[where] = keep
        assert f.intact()
    assert f.damage() == []


def test_a_single_changed_byte_is_seen():
    f = fc.frame(_table(torch.float64), fc.BIG)
    at = f.front + f.nbytes + 3         # (a byte in the middle of the first guard element behind)
    f.buf[at] ^= 1
    assert not f.intact() and f.damage() == [f.nbytes + 3]
    f.buf[at] ^= 1
    assert f.intact()


def test_pattern_poison_continues_the_records():
    t = torch.zeros((5, fc.INST_WORDS), dtype=torch.int32)
    f = fc.frame(t, fc.inst_poison())
    flat = f.buf.view(torch.int32)
    first = f.front // 4
    behind = flat[first + t.numel():first + t.numel() + 2 * fc.INST_WORDS].tolist()
    assert behind == fc.inst_poison() * 2
    before = flat[first - 2 * fc.INST_WORDS:first].tolist()
    assert before == fc.inst_poison() * 2


def test_poison_values():
    f = fc.frame(torch.zeros(6, dtype=torch.float32), fc.BIG)
    g = f.buf[:f.front].view(torch.float32)
    assert bool(torch.isfinite(g).all()) and float(g[0]) > 1e30
    bits = int(g.view(torch.int32)[0]) & 0xFFFFFFFF
    assert not (0xFFFFFFC0 <= bits <= 0xFFFFFFFF)
    # a model record and its digest: state 0, non-terminal, the huge reward
    rec = fc.MODEL_POISON
    assert np.uint32(rec & 0xFFFFFFFF).view(np.float32) == np.float32(fc.BIG)
    assert (rec >> 32) & 0xFFFF == 0 and (rec >> 48) & 0xFF == 1
    assert fc.INDEX_POISON & 0x3FFF == 0 and fc.INDEX_POISON & 0x4000 and fc.INDEX_POISON & 0x8000
    for A, nt_bit in ((4, 30), (6, 31), (17, 31)):
        hi = (fc.log_poison(A) >> 32) & 0xFFFFFFFF
        assert hi == 1 << nt_bit
    w0, w1 = fc.log_poison(4, words=2)
    assert np.uint32(w0 & 0xFFFFFFFF).view(np.float32) == np.float32(fc.BIG)
    assert (w0 >> 32) == 1 << 8 and w1 == 0        # action 0, non-terminal; state 0 -> state 0


def test_frames_swap_and_check():
    class Holder:
        pass

    h = Holder()
    h.table = _table(torch.float32)
    h.none = None
    raw = {'lat_sum': _table(torch.int64, (1, 9))}
    frames = fc.Frames()
    view = frames.swap(h, 'table', fc.BIG)
    assert frames.swap(h, 'none', 0) is None
    frames.swap(raw, 'lat_sum', fc.MARK)
    mine = frames.add('mine', _table(torch.int16, (4,)), 0)
    assert h.table is view and mine.dtype == torch.int16
    frames.check()
    raw['lat_sum'][0, 3] += 1
    frames.check()
    keep = h.table
    h.table = keep.clone()                    # "silently reallocated"
    with pytest.raises(AssertionError, match='reallocated'):
        frames.check()
    h.table = keep
    frames.items[0][1].buf[0] ^= 0xFF
    with pytest.raises(AssertionError, match='guard bytes changed'):
        frames.check()


def test_same_bits_sees_nan_payloads_and_signed_zeros():
    a = np.array([0.0, np.nan], dtype=np.float32)
    b = a.copy()
    assert fc.same_bits(a, b)
    b[0] = -0.0
    assert not fc.same_bits(a, b)
    b = a.copy()
    b.view(np.uint32)[1] ^= 1
    assert not fc.same_bits(a, b)
    assert not fc.same_bits(a, a.astype(np.float64))
