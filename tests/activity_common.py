"""A plain NumPy restatement (no scipy, no torch, no project code) of what cobel_mlp_activity
(csrc/mlp_fit.hip) and cobel_activity_process / cobel_place_fields (csrc/activity.hip) compute —
TorchNetwork.get_layer_activity and analysis/network_spatial.py of the reference — the seeded maps
the tests share, and the fillers of the launch struct.

The casts the reference leaves to NumPy's promotion rules are written out: ``threshold`` and
``cutoff`` are taken in the array's dtype (``a.dtype.type(threshold)``), which is what NumPy 2
does with a Python float beside a float32 array."""
import ctypes as C

import numpy as np

import mlp_common as mc
import mlp_tanh_common as mt

APPLY = {'none': 0, 'relu': 1, 'tanh': 2}
HIDDEN = {'relu': 0, 'tanh': 1}


# ---------------------------------------------------------------------------------------------
# layer activity
def _apply(pre, apply):
    if apply == 'relu':
        return np.maximum(pre, 0.0)
    if apply == 'tanh':
        return np.tanh(pre)
    assert apply == 'none'
    return pre


def layer_activity(p, x, layer, hidden, apply, units=None):
    """[U or K, P]: ``apply`` of the output of Linear ``layer`` (0 .. 2) of the network ``p`` (a dict
    of mlp_common) on the rows of x [P, D], units-major; ``hidden`` is what the network applies
    between its layers."""
    h1, h2, _ = (mt if hidden == 'tanh' else mc).forward(p, x)
    source = (x, h1, h2)[layer]
    pre = source @ p['w%d' % (layer + 1)].T + p['b%d' % (layer + 1)]
    act = _apply(pre, apply).T
    return act if units is None else act[np.asarray(units)]


def stack_activity(stack, probes, layer, hidden, apply, units=None):
    """[n, U or K, P] in float64 for a stack of mlp_common; probes [P, D] or [n, P, D]."""
    n = stack['w1'].shape[0]
    probes = np.asarray(probes, dtype=np.float64)
    return np.stack([layer_activity(mc.one(stack, j), probes if probes.ndim == 2 else probes[j],
                                    layer, hidden, apply, units) for j in range(n)])


def fill_activity(lib, params, probes, out, n, P, D, O, layer, hidden, apply, units=None,
                  per_instance=False):
    run = lib.MLPActivity()
    mc._three(lib, run.w, params, ('w1', 'w2', 'w3'))
    mc._three(lib, run.b, params, ('b1', 'b2', 'b3'))
    run.probes, run.out, run.units = lib.ptr(probes), lib.ptr(out), lib.ptr(units)
    run.n, run.n_probes, run.n_inputs, run.n_outputs = n, P, D, O
    w1 = params['w1']
    run.is_float64 = int((w1.element_size() if hasattr(w1, 'element_size') else w1.itemsize) == 8)
    run.layer, run.hidden_activation, run.apply = layer, HIDDEN[hidden], APPLY[apply]
    run.n_units = 0 if units is None else int(units.numel() if hasattr(units, 'numel') else units.size)
    run.probes_per_instance = int(bool(per_instance))
    return run


# ---------------------------------------------------------------------------------------------
# process_activity_maps
def process(rows, threshold=0.15):
    """A processed copy of rows [R, P]: x -= min, x /= max(x), x[x < threshold] = 0 per row."""
    a = np.array(rows, copy=True)
    T = a.dtype.type
    with np.errstate(all='ignore'):
        a -= np.amin(a, axis=1).reshape(-1, 1)
        a /= np.amax(a, axis=1).reshape(-1, 1)
        a[a < T(threshold)] = T(0)
    return a


# ---------------------------------------------------------------------------------------------
# classify_place_field, sigma = 0
def label(mask):
    """4-connected components of a boolean map, numbered 1 .. in the order of their first cell in
    row-major order (scipy.ndimage.label's numbering): a flood fill, one component at a time."""
    H, W = mask.shape
    labels = np.zeros((H, W), dtype=np.int32)
    count = 0
    for r0 in range(H):
        for c0 in range(W):
            if not mask[r0, c0] or labels[r0, c0]:
                continue
            count += 1
            labels[r0, c0] = count
            todo = [(r0, c0)]
            while todo:
                r, c = todo.pop()
                for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                    if 0 <= rr < H and 0 <= cc < W and mask[rr, cc] and not labels[rr, cc]:
                        labels[rr, cc] = count
                        todo.append((rr, cc))
    return labels, count


def classify(a, size_threshold=0.5, cutoff=0.25):
    """(has_field, field, error, features, largest_area) of one map [H, W]."""
    assert 0 < size_threshold < 1 and 0 < cutoff < 1
    T = a.dtype.type
    with np.errstate(all='ignore'):
        thr = T(cutoff) * np.max(a)
        field = np.where(a < thr, T(0), a)
    labels, features = label(field > 0)
    cells = a.shape[0] * a.shape[1]
    largest_area = cells
    if features:
        areas = []
        for k in range(1, features + 1):
            rr, cc = np.nonzero(labels == k)
            areas.append(int((rr.max() - rr.min() + 1) * (cc.max() - cc.min() + 1)))
        largest = int(np.argmax(areas))          # the first maximum
        largest_area = areas[largest]
        field = np.where(labels == largest + 1, field, T(0))
    error = 1 if features == 0 else 2 if features > 4 else \
        3 if float(largest_area) > size_threshold * float(cells) else 0
    assert field.dtype == a.dtype
    return error == 0, field, error, features, largest_area


def classify_many(maps, size_threshold=0.5, cutoff=0.25):
    """classify over maps [M, H, W]: has_field u8 [M], error / features / largest_area i32 [M],
    fields [M, H, W]."""
    got = [classify(m, size_threshold, cutoff) for m in maps]
    return (np.array([g[0] for g in got], dtype=np.uint8),
            np.array([g[2] for g in got], dtype=np.int32),
            np.array([g[3] for g in got], dtype=np.int32),
            np.array([g[4] for g in got], dtype=np.int32),
            np.stack([g[1] for g in got]))


# ---------------------------------------------------------------------------------------------
# the maps
def serpentine(H, W):
    """One component that winds through every second row: full even rows joined at alternating ends."""
    a = np.zeros((H, W))
    a[0::2] = 1.0
    for k, r in enumerate(range(1, H, 2)):
        a[r, W - 1 if k % 2 == 0 else 0] = 1.0
    return a


def named_maps(H, W, dtype):
    """The planted maps that fit H x W, by name, in ``dtype``."""
    rng = np.random.default_rng(1000 * H + W)
    m = {}
    m['zero'] = np.zeros((H, W))
    m['negative'] = -rng.uniform(0.5, 1.0, (H, W))
    m['nan'] = np.full((H, W), np.nan)
    one_nan = rng.uniform(0.0, 1.0, (H, W))
    one_nan[H // 2, W // 2] = np.nan
    m['one_nan'] = one_nan
    m['constant'] = np.full((H, W), 0.7)
    m['serpentine'] = serpentine(H, W)
    m['serpentine_t'] = serpentine(W, H).T.copy()
    m['random'] = rng.uniform(0.0, 1.0, (H, W)) * (rng.random((H, W)) < 0.55)
    checker = np.zeros((H, W))
    checker[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = 1.0
    m['checkerboard'] = checker
    comb = np.zeros((H, W))
    comb[0, :] = 1.0
    comb[:, 0::2] = 1.0
    m['comb'] = comb
    if H >= 5 and W >= 7:
        blob = np.zeros((H, W))
        blob[1:3, 2:4] = [[1.0, 0.9], [0.8, 0.7]]
        m['blob'] = blob
        two = np.zeros((H, W))                    # equal boxes: the first wins
        two[0:2, 4:6] = 0.9
        two[3:5, 0:2] = 1.0
        m['two_equal'] = two
        ell = np.zeros((H, W))                    # box H x (W - 1) > half, cells H + W - 2 < half
        ell[:, 0] = 1.0
        ell[H - 1, :W - 1] = 1.0
        m['ell'] = ell
        for count in (4, 5):
            b = np.zeros((H, W))
            for k, (r, c) in enumerate(((0, 0), (0, 3), (0, 6), (3, 0), (4, 6))[:count]):
                b[r, c] = 1.0 - 0.1 * k
            m['blobs%d' % count] = b
        diag = np.zeros((H, W))
        diag[1, 1] = diag[2, 2] = 1.0
        m['diagonal'] = diag
        plateau = np.zeros((H, W))                # a == thr stays: 0.25 * 1.0 exactly
        plateau[1, 1:4] = 1.0
        plateau[2, 1:4] = 0.25
        plateau[3, 1:4] = np.nextafter(0.25, 0.0)
        m['plateau'] = plateau
    return {k: v.astype(dtype) for k, v in m.items()}


def random_maps(seed, count, dtype):
    """The seeded sweep: ``count`` maps of 1 x 1 .. 8 x 8 with plateaus, ties, negative, sparse,
    all-NaN, all-zero and all-negative maps, as (map, cutoff, size_threshold)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        H, W = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        kind = int(rng.integers(0, 8))
        if kind == 0:
            a = rng.integers(0, 4, (H, W)) / 3.0                    # plateaus and ties
        elif kind == 1:
            a = rng.standard_normal((H, W))
        elif kind == 2:
            a = rng.uniform(0, 1, (H, W)) * (rng.random((H, W)) < 0.3)
        elif kind == 3:
            a = np.full((H, W), np.nan)
        elif kind == 4:
            a = np.zeros((H, W))
        elif kind == 5:
            a = -rng.uniform(0, 1, (H, W))
        elif kind == 6:
            a = rng.integers(0, 2, (H, W)).astype(np.float64)
        else:
            a = rng.uniform(0, 1, (H, W))
        out.append((a.astype(dtype), float(rng.choice([0.1, 0.25, 0.5])),
                    float(rng.choice([0.3, 0.5]))))
    return out


def process_rows(P, dtype):
    """Rows [R, P] for cobel_activity_process: random, negative, constant, with a NaN, with
    infinities, all equal but one."""
    rng = np.random.default_rng(77 + P)
    rows = [rng.standard_normal(P), -rng.uniform(1, 2, P), np.full(P, 0.3), rng.uniform(0, 1, P),
            rng.uniform(0, 1, P), rng.uniform(0, 1, P), np.zeros(P), rng.uniform(0, 1e-3, P)]
    rows[3][P // 2] = np.nan
    rows[4][0] = np.inf
    rows[5][P - 1] = -np.inf
    rows[6][P // 3] = 1.0
    return np.stack(rows).astype(dtype)


def sizeof_fields(cls):
    return C.sizeof(cls), [getattr(cls, f).offset for f, _ in cls._fields_]


# ---------------------------------------------------------------------------------------------
# place_like
def pdist(points):
    points = np.asarray(points, dtype=np.float64)
    i, j = np.triu_indices(points.shape[0], k=1)
    return np.sqrt(((points[i] - points[j]) ** 2).sum(axis=1))


def _centers_pdist(fields_sliced, n):
    centers = np.zeros((max(1, n), 6, 2))
    for i, field in enumerate(fields_sliced):
        for j, angle in enumerate(field):
            centers[i, j] = divmod(np.argmax(angle), 25)
    angles = np.deg2rad(np.arange(0, 360, 60, dtype='int32'))
    vectors = np.stack([np.cos(angles), np.sin(angles)], axis=1)
    return np.array([pdist(c) for c in centers]), pdist(vectors)


def place_like(fields, resolution, size_threshold=0.5, cutoff=0.25):
    """analysis/network_spatial.py:178-252 on top of ``classify``: (fields, ids, pdist of the
    centers, pdist of the direction vectors)."""
    area, n_units = int(np.prod(resolution)), fields.shape[2]
    stacked = np.vstack((fields, np.mean(fields, axis=0).reshape((1, area, n_units))))
    is_field = np.zeros((stacked.shape[0], n_units))
    largest = np.zeros((stacked.shape[0], area, n_units))
    for i in range(n_units):
        for j in range(stacked.shape[0]):
            got = classify(stacked[j, :, i].reshape(resolution), size_threshold, cutoff)
            is_field[j, i], largest[j, :, i] = got[0], got[1].flatten()
    ids = np.squeeze(np.array(np.where(np.all(is_field, axis=0))))
    if ids.shape != () and ids.size > 0:
        f = np.array([largest[:, :, p] for p in ids])
        pd, v = _centers_pdist(f[:, :6, :], len(ids))
    else:
        pd, v = np.full((1, 15), 15), np.full((1, 15), 15)
    ids = np.where(np.all(np.array(pd) < 10, axis=1), ids, -1)
    ids = ids[ids != -1]
    f = np.array([largest[:, :, p] for p in ids])
    if ids.size > 0:
        pd, v = _centers_pdist(f[:, :6, :], len(ids))
    else:
        pd = np.full((1, 15), 15)
    return f, ids, pd, v


def place_like_fields(case):
    """Synthetic ``fields`` [6, 625, 4] at resolution (25, 25): a unit qualifies if every trial
    and the mean hold one small blob at (nearly) the same place.  'several': units 0 and 2
    qualify, 1 is silent in one trial, 3 moves across the arena; 'one': unit 1 alone; 'none'."""
    rng = np.random.default_rng({'several': 1, 'one': 2, 'none': 3}[case])
    fields = np.zeros((6, 25, 25, 4))

    def blob(t, u, r, c):
        fields[t, r:r + 3, c:c + 3, u] = rng.uniform(0.5, 1.0, (3, 3))

    good = {'several': (0, 2), 'one': (1,), 'none': ()}[case]
    for u in range(4):
        for t in range(6):
            if u in good:
                blob(t, u, 8 + u + t % 2, 5 + 2 * u)
            elif u == 3:
                blob(t, u, 3 * t, 20 - 3 * t)          # wanders: the mean map has six blobs
            elif t != 4:
                blob(t, u, 12, 12)                      # silent in trial 4
    return fields.reshape(6, 625, 4)


# ---------------------------------------------------------------------------------------------
# the fixture's network (tests/golden/gen_activity.py records the reference on it)
FIXTURE_D, FIXTURE_O, FIXTURE_P = 7, 4, 40
MONITOR_INTERVALS = {'every': 0, 'third': 3, 'trials': (0, 2, 5)}
MONITOR_UPDATES = 8


def fixture_params():
    return mc.one(mc.draw_networks(np.random.default_rng(20240), 1, FIXTURE_D, FIXTURE_O,
                                   np.float64), 0)


def fixture_probes():
    return np.random.default_rng(20241).standard_normal((FIXTURE_P, FIXTURE_D))


def monitor_params(t):
    """The network at the t-th ``update`` of the monitor fixture: every parameter scaled."""
    return {k: v * (1.0 + 0.05 * t) for k, v in fixture_params().items()}


def load_params(torch, model, names, p):
    with torch.no_grad():
        for k, name in enumerate(names):
            model.get_submodule(name).weight.copy_(torch.from_numpy(p['w%d' % (k + 1)]))
            model.get_submodule(name).bias.copy_(torch.from_numpy(p['b%d' % (k + 1)]))


def torch_models(torch, p):
    """name -> (model, names of its Linear layers, activations, hidden, requests): the fixture's
    network as a custom-forward module with an ``activations`` dict (ReLU and tanh) and as an
    ``nn.Sequential`` with a list; ``requests`` are (layer, Linear index, apply) triples."""
    nn = torch.nn

    def custom(act):
        class Net(nn.Module):
            def __init__(self):
                super().__init__()
                self.fc1, self.fc2 = nn.Linear(FIXTURE_D, 64), nn.Linear(64, 64)
                self.fc3 = nn.Linear(64, FIXTURE_O)

            def forward(self, x):
                return self.fc3(act(self.fc2(act(self.fc1(x)))))
        return Net().double()

    def sequential(module):
        return nn.Sequential(nn.Linear(FIXTURE_D, 64), module(), nn.Linear(64, 64), module(),
                             nn.Linear(64, FIXTURE_O)).double()

    fcs, seq = ('fc1', 'fc2', 'fc3'), ('0', '2', '4')
    out = {
        'custom_relu': (custom(torch.relu), fcs, {'fc1': torch.relu, 'fc2': None, 'fc3': torch.tanh},
                        'relu', [('fc1', 0, 'relu'), ('fc2', 1, 'none'), ('fc3', 2, 'tanh'),
                                 (0, 0, 'relu'), (1, 1, 'none'), (2, 2, 'tanh')]),
        'custom_tanh': (custom(torch.tanh), fcs, {'fc1': torch.tanh, 'fc2': torch.tanh, 'fc3': None},
                        'tanh', [('fc1', 0, 'tanh'), ('fc2', 1, 'tanh'), ('fc3', 2, 'none')]),
        'sequential_relu': (sequential(nn.ReLU), seq, [None, None, torch.relu, None, None], 'relu',
                            [(0, 0, 'none'), (1, 0, 'relu'), (2, 1, 'relu'), (3, 1, 'relu'),
                             (4, 2, 'none')]),
        'sequential_tanh': (sequential(nn.Tanh), seq, [torch.tanh, None, None, None, torch.relu],
                            'tanh', [(0, 0, 'tanh'), (1, 0, 'tanh'), (2, 1, 'none'), (3, 1, 'tanh'),
                                     (4, 2, 'relu')]),
    }
    for model, names, _, _, _ in out.values():
        load_params(torch, model, names, p)
    return out


FIXTURE_SHAPES = [(1, 1), (1, 8), (8, 1), (5, 7), (25, 25), (32, 32)]
