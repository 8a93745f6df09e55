"""Sentinel frames around the tables of the older kernel families (tests/test_gpu_frames_*.py).

``frame(t, poison)`` puts a tensor in the middle of a larger buffer whose two guards are filled with
``poison``; ``Frames.swap(obj, name, poison)`` does so in place for a tensor an agent, a memory or a
monitor object keeps in an attribute (or a dictionary entry) and hands to a kernel at launch time.
After the run ``Frames.check()`` asserts that no guard changed, byte for byte, and that no framed
attribute was reallocated behind the test's back.

The guards serve two ends.  A stray WRITE changes a guard.  A stray READ picks up the poison, which
is chosen so that it changes the results — the framed run is compared bit for bit with a plain run
of the same seeded session — without ever forming an address: a huge finite float in value tables
(NaN would be dropped by ``fmaxf`` and by comparison chains), a record that decodes to state 0 in
tables that hold indices, a recognisable integer in counters.

``poison`` is a number (every guard element gets it) or a 1-D sequence of numbers, a pattern that
is laid out as if it went on periodically THROUGH the table: the element right behind the table
gets ``pattern[numel % len]`` and the one right in front of it ``pattern[-1]``, so a table of
records (``inst``: 12 words each) is continued by whole records on both sides."""
import numpy as np

GUARD = 4096               # bytes of each guard: a multiple of 256, so a table keeps its alignment
BIG = 7.77e30              # value tables: huge, finite, positive, not a tag pattern 0xffffffc0..ff
MARK = 0x5A5A5A5A          # counters and monitors (int32 / int64)


class Frame:
    """``view``: a tensor shaped like ``t`` holding its contents, ``front`` bytes behind the start of
    a buffer and followed by ``GUARD`` bytes more.  ``shift`` (a multiple of 16) moves the table
    that many bytes off the 256-byte boundary it would otherwise start on."""

    def __init__(self, torch, t, poison, shift=0):
        assert t.is_contiguous() and shift % 16 == 0 and 0 <= shift < 256
        self.torch = torch
        size = t.element_size()
        nbytes = t.numel() * size
        self.front, self.nbytes = GUARD + shift, nbytes
        assert self.front % size == 0 and GUARD % size == 0
        total = self.front + nbytes + GUARD
        self._alloc = torch.empty(total + 256, dtype=torch.uint8, device=t.device)
        skip = -self._alloc.data_ptr() % 256      # (0 on the device: its allocator aligns to 512)
        self.buf = self._alloc[skip:skip + total]
        assert self.buf.data_ptr() % 256 == 0
        pattern = np.atleast_1d(np.asarray(poison))
        pattern = torch.as_tensor(pattern.astype(_np_dtype(torch, t.dtype)), device=t.device)
        nf, nb, k = self.front // size, GUARD // size, pattern.numel()
        # (element e of the table has index e: the front guard holds indices -nf .. -1)
        idx_front = torch.arange(-nf, 0, device=t.device) % k
        idx_back = (torch.arange(0, nb, device=t.device) + t.numel()) % k
        self.buf[:self.front].view(t.dtype).copy_(pattern[idx_front])
        self.buf[self.front + nbytes:].view(t.dtype).copy_(pattern[idx_back])
        self.view = self.buf[self.front:self.front + nbytes].view(t.dtype).view(t.shape)
        self.view.copy_(t)
        self._guards = (self.buf[:self.front].clone(), self.buf[self.front + nbytes:].clone())

    def intact(self):
        """Both guards hold what they were filled with, byte for byte."""
        eq = self.torch.equal
        return bool(eq(self.buf[:self.front], self._guards[0])
                    and eq(self.buf[self.front + self.nbytes:], self._guards[1]))

    def damage(self):
        """Byte offsets, relative to the table's first byte, of the guard bytes that changed."""
        f = (self.buf[:self.front] != self._guards[0]).nonzero().reshape(-1) - self.front
        b = (self.buf[self.front + self.nbytes:] != self._guards[1]).nonzero().reshape(-1) \
            + self.nbytes
        return [int(x) for x in f[:8].tolist()] + [int(x) for x in b[:8].tolist()]


def _np_dtype(torch, dtype):
    return {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64,
            torch.int32: np.int32, torch.int16: np.int16, torch.uint8: np.uint8,
            torch.int8: np.int8, torch.bool: np.bool_}[dtype]


def frame(t, poison, shift=0):
    """The framed copy of device (or CPU) tensor ``t``: use ``.view``, ask ``.intact()``."""
    import torch
    return Frame(torch, t, poison, shift)


class Frames:
    """The frames of one run.  ``swap`` frames what an object keeps, ``add`` a tensor the test owns
    (it returns the view to hand on); ``check`` is assertion 1 of every case."""

    def __init__(self, shift=0):
        self.shift = shift
        self.items = []                     # (label, frame, holder, key)

    def add(self, label, t, poison):
        f = frame(t, poison, self.shift)
        self.items.append((label, f, None, None))
        return f.view

    def swap(self, obj, name, poison):
        """Frame ``obj.<name>`` (``obj[name]`` for a dictionary) in place; None stays None."""
        is_dict = isinstance(obj, dict)
        t = obj[name] if is_dict else getattr(obj, name)
        if t is None:
            return None
        f = frame(t, poison, self.shift)
        if is_dict:
            obj[name] = f.view
        else:
            setattr(obj, name, f.view)
        self.items.append(('%s.%s' % (type(obj).__name__, name), f, obj, name))
        return f.view

    def check(self):
        assert self.items, 'nothing was framed'
        for label, f, obj, name in self.items:
            if obj is not None:
                now = obj[name] if isinstance(obj, dict) else getattr(obj, name)
                assert now is not None and now.data_ptr() == f.view.data_ptr(), \
                    label + ' was reallocated'
            assert f.intact(), '%s: guard bytes changed at offsets %r (table of %d bytes)' % (
                label, f.damage(), f.nbytes)


def same_bits(a, b):
    """Bit-for-bit equality of two tensors / arrays (NaNs compare by their bits)."""
    a = a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)
    b = b.detach().cpu().numpy() if hasattr(b, 'detach') else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_same(plain, framed):
    """Assertion 2: every array of the framed run equals the plain run's bit for bit."""
    assert plain.keys() == framed.keys()
    for key in plain:
        assert same_bits(plain[key], framed[key]), key + ' differs between plain and framed run'


# -- what the tabular, SR and SFMA agents share ----------------------------------------------------
INST_WORDS = 12            # cobel_hip.h: COBEL_I_WORDS
_BIG_BITS = int(np.float32(BIG).view(np.uint32))
MODEL_POISON = _BIG_BITS | (1 << 48)          # {f32 R = BIG; u16 next state 0; u8 nonterminal 1}
INDEX_POISON = 0xC000 - (1 << 16)             # next 0 | nonterminal << 14 | (R != 0) << 15, as int16


def inst_poison():
    """An ``inst`` record at state 0 whose other words are recognisable (and positive: a poisoned
    step or trial counter ends a run early, it never indexes anything)."""
    return [0] + [MARK] * (INST_WORDS - 1)


def log_poison(n_actions, words=1):
    """A replay-log entry: state 0 -> state 0 by action 0, non-terminal, reward BIG.  One word, or
    the two of worlds beyond 16 384 states ({reward, action | nonterminal << 8}, {state, next})."""
    if words == 2:
        return [_BIG_BITS | (1 << 40), 0]
    nt = 30 if n_actions <= 4 else 31
    v = _BIG_BITS | (1 << (32 + nt))
    return v - (1 << 64) if v >= (1 << 63) else v


def swap_monitors(frames, mon):
    """Every array ``DeviceMonitors.fill`` hands to a launch struct."""
    for name in mon._PER_TRIAL:
        frames.swap(mon._raw, name, BIG if name == 'reward_sum' else MARK)
    frames.swap(mon, 'lat_trace', MARK)
    frames.swap(mon, 'occupancy', MARK)
    frames.swap(mon, 'steps_done', MARK)


def monitor_arrays(mon):
    out = {'mon.' + k: v for k, v in mon._raw.items() if v is not None}
    for name in ('lat_trace', 'occupancy', 'steps_done'):
        if getattr(mon, name) is not None:
            out['mon.' + name] = getattr(mon, name)
    return out


def swap_fused(frames, ag):
    """What ``FusedAgent._fill_run`` hands on: ``inst``, ``last_exp``, the monitors, and — once
    ``_hyper`` built them — the parameter sets and their index.  The action mask is rebuilt at
    every launch: ``frame_mask`` replaces the builder."""
    frames.swap(ag, 'inst', inst_poison())
    frames.swap(ag, '_last_exp', MARK)
    swap_monitors(frames, ag.monitors)
    frames.swap(ag, '_pset_dev', 0)        # (512-byte records of doubles: zeros are valid sets)
    frames.swap(ag, '_pidx_dev', 0)        # (index of a set: set 0)


def frame_mask(frames, ag):
    """The framed action-mask bits, handed out by ``ag._mask_bits`` at every launch.  Guards: all
    actions allowed (a mask of no action has no successor to offer)."""
    bits = type(ag)._mask_bits(ag)
    allowed = (1 << ag.n_actions) - 1
    view = frames.add('action_mask', bits, allowed - (1 << 32) if allowed >= (1 << 31) else allowed)
    ag._mask_bits = lambda: view
    return view


# -- worlds the cases share ---------------------------------------------------------------------------
def graph(S, A, seed):
    """Random graph of ``A`` neighbours per node (a Topology); the last node leads to a rewarded one."""
    r = np.random.default_rng(seed)
    nbr = r.integers(0, S, (S, A))
    nbr[S - 1, A - 1] = 11
    terminal = np.zeros(S, dtype=bool)
    terminal[[7, 23]] = True
    reward = np.zeros(S)
    reward[7], reward[23], reward[11] = 1.0, -0.5, 0.25
    return {str(i): {'id': str(i), 'pose': np.array([float(i % 7), float(i // 7), 0., 0., 0., 0.]),
                     'neighbors': [str(int(j)) for j in nbr[i]], 'reward': float(reward[i]),
                     'terminal': bool(terminal[i])} for i in range(S)}
