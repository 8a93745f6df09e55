"""Layer activity and place-field analysis without a GPU: the NumPy restatement
(tests/activity_common.py) against the reference's own functions where the reference and scipy are
at hand, the exports and the launch struct, every refusal the library decides before a launch, and
the host side of cobel_amd.analysis.network_spatial."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activity_common as ac  # noqa: E402
import mlp_common as mc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_mlp_activity', 'cobel_activity_process', 'cobel_place_fields',
       'cobel_place_fields_plan')


# -- the restatement ----------------------------------------------------------------------------------
def _scipy_classify(a, size_threshold, cutoff):
    """classify_place_field of the reference with sigma = 0, on scipy (analysis/network_spatial.py:
    107-133 said again: scipy is what defines the numbering of the components)."""
    nd = pytest.importorskip('scipy.ndimage')
    with np.errstate(all='ignore'):
        field = np.where(a < cutoff * np.max(a), 0, a)
    labels, features = nd.label(field > 0)
    largest, area = 0, [np.prod(a.shape)]
    if features != 0:
        area = np.prod([field[s].shape for s in nd.find_objects(labels)], axis=1)
        largest = int(np.argmax(area))
        field = np.where(labels == largest + 1, field, 0)
    error = 1 if features == 0 else 2 if features > 4 else \
        3 if area[largest] > size_threshold * np.prod(a.shape) else 0
    return error, features, int(area[largest]), field


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_classifier_restatement_against_scipy(dtype):
    hit = set()
    for a, cutoff, size in ac.random_maps(5, 600, dtype):
        error, features, area, field = _scipy_classify(a, size, cutoff)
        has, got, e, f, la = ac.classify(a, size, cutoff)
        assert (e, f, la, has) == (error, features, area, error == 0), (a, cutoff, size)
        assert got.dtype == field.dtype and np.array_equal(got, field, equal_nan=True)
        hit.add(e)
    assert hit == {0, 1, 2, 3}
    for H, W in ((1, 1), (1, 8), (8, 1), (5, 7), (25, 25), (32, 32)):
        for name, a in ac.named_maps(H, W, dtype).items():
            error, features, area, field = _scipy_classify(a, 0.5, 0.25)
            _, got, e, f, la = ac.classify(a, 0.5, 0.25)
            assert (e, f, la) == (error, features, area), (H, W, name)
            assert np.array_equal(got, field, equal_nan=True), (H, W, name)


def test_named_maps_are_what_they_claim():
    m = ac.named_maps(5, 7, np.float64)
    want = {'zero': (1, 0), 'negative': (1, 0), 'nan': (1, 0), 'constant': (3, 1), 'blob': (0, 1),
            'two_equal': (0, 2), 'ell': (3, 1), 'blobs4': (0, 4), 'blobs5': (2, 5),
            'diagonal': (0, 2), 'plateau': (0, 1), 'serpentine': (3, 1)}
    for name, (error, features) in want.items():
        _, field, e, f, _ = ac.classify(m[name])
        assert (e, f) == (error, features), name
    assert np.array_equal(ac.classify(m['two_equal'])[1] > 0, m['two_equal'] == 0.9)
    assert int((ac.classify(m['ell'])[1] > 0).sum()) < 0.5 * 35 < ac.classify(m['ell'])[4]
    assert np.count_nonzero(ac.classify(m['plateau'])[1]) == 6          # a == thr stays
    big = ac.named_maps(32, 32, np.float32)
    assert ac.classify(big['checkerboard'])[3] == 512
    assert ac.classify(big['serpentine'])[3] == 1 and ac.classify(big['serpentine_t'])[3] == 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_process_restatement_is_the_reference_expression(dtype):
    rows = ac.process_rows(33, dtype)
    want = rows.copy()
    with np.errstate(all='ignore'):      # analysis/network_spatial.py:62-65 as written there
        want -= np.amin(want, axis=1).reshape((want.shape[0], 1))
        want /= np.amax(want, axis=1).reshape((want.shape[0], 1))
        want[want < 0.15] = 0.0
    got = ac.process(rows, 0.15)
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[2]).all() and np.isnan(got[3]).all()      # constant row; a row with a NaN
    assert np.isnan(got[5]).all()                                  # -inf meets itself


def test_layer_activity_restatement_against_torch():
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(3)
    stack = mc.draw_networks(rng, 2, 7, 4, np.float64)
    x = rng.standard_normal((9, 7))
    for hidden, act in (('relu', torch.relu), ('tanh', torch.tanh)):
        p = {k: torch.from_numpy(v[1]) for k, v in stack.items()}
        xt = torch.from_numpy(x)
        pre1 = xt @ p['w1'].T + p['b1']
        pre2 = act(pre1) @ p['w2'].T + p['b2']
        pre3 = act(pre2) @ p['w3'].T + p['b3']
        for layer, pre in enumerate((pre1, pre2, pre3)):
            for apply, f in (('none', lambda v: v), ('relu', torch.relu), ('tanh', torch.tanh)):
                got = ac.layer_activity(mc.one(stack, 1), x, layer, hidden, apply)
                assert np.allclose(got, f(pre).T.numpy(), rtol=1e-12, atol=1e-14)
    units = [3, 0, 3]
    full = ac.stack_activity(stack, x, 1, 'relu', 'relu')
    assert np.array_equal(ac.stack_activity(stack, x, 1, 'relu', 'relu', units), full[:, units])


# -- the library ----------------------------------------------------------------------------------------
def test_exports_and_struct_layout(tmp_path):
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    assert lib.cobel_abi_version() == 1017
    for name in NEW:
        m = re.search(r'COBEL_API\s+int\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert name in _lib.EXPORTS
        getattr(lib, name)
        args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(args.split(',')) == len(_lib._SIGNATURES[name][1]), name
    for cites in (r'network_torch\.py:331-388', r'network_spatial\.py:45-67',
                  r'network_spatial\.py:70-144'):
        assert re.search(cites, header), cites
    assert (_lib.APPLY_NONE, _lib.APPLY_RELU, _lib.APPLY_TANH) == (0, 1, 2)
    assert re.search(r'COBEL_APPLY_NONE = 0, COBEL_APPLY_RELU = 1, COBEL_APPLY_TANH = 2', header)
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc is not None, 'no C compiler'
    fields = [f for f, _ in _lib.MLPActivity._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\nprintf("%zu\\n", sizeof(cobel_mlp_activity_t));\n'
                   + ''.join('printf("%%zu\\n", offsetof(cobel_mlp_activity_t, %s));\n' % f
                             for f in fields) + 'return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    size, offsets = ac.sizeof_fields(_lib.MLPActivity)
    assert got[0] == size and got[1:] == offsets


def test_mlp_activity_refuses_before_a_launch():
    from cobel_amd import _lib
    lib = _lib.lib()
    dummy = np.zeros(64 * 64 + 64)
    params = {k: dummy for k in mc.KEYS}

    def call(run):
        _lib.check(lib.cobel_mlp_activity(None if run is None else C.byref(run), None))

    def run_of(D=7, O=4, n=2, P=5, layer=1, **kw):
        run = ac.fill_activity(_lib, params, dummy, dummy, n, P, D, O, layer, 'relu', 'relu')
        run.is_float64 = 1
        for k, v in kw.items():
            setattr(run, k, v)
        return run

    with pytest.raises(AssertionError, match='NULL run'):
        call(None)
    for D, O in ((0, 4), (33, 4), (7, 0), (7, 33)):
        with pytest.raises(NotImplementedError, match=r'got D %d, O %d' % (D, O)):
            call(run_of(D=D, O=O))
    run = run_of()
    run.w[1] = None
    with pytest.raises(AssertionError, match=r'NULL parameters \(layer 1\)'):
        call(run)
    run = run_of()
    run.b[2] = None
    with pytest.raises(AssertionError, match=r'NULL parameters \(layer 2\)'):
        call(run)
    for field in ('probes', 'out'):
        with pytest.raises(AssertionError, match='probes and out are required'):
            call(run_of(**{field: None}))
    with pytest.raises(IndexError, match='bad sizes'):
        call(run_of(n=-1))
    with pytest.raises(IndexError, match='0 probes'):
        call(run_of(P=0))
    for layer in (-1, 3):
        with pytest.raises(IndexError, match=r'layer = %d' % layer):
            call(run_of(layer=layer))
    for apply in (-1, 3):
        with pytest.raises(IndexError, match=r'apply = %d' % apply):
            call(run_of(apply=apply))
    with pytest.raises(AssertionError, match='hidden_activation = 2'):
        call(run_of(hidden_activation=2))
    with pytest.raises(IndexError, match='n_units = 0'):
        call(run_of(units=_lib.ptr(dummy), n_units=0))
    run = run_of()
    run.w[1] = _lib.ptr(dummy) + 8
    with pytest.raises(AssertionError, match='16-byte aligned'):
        call(run)
    call(run_of(n=0))            # nothing to do is no error and needs no device


def test_activity_process_and_place_fields_refuse_before_a_launch():
    from cobel_amd import _lib
    lib = _lib.lib()
    d = _lib.ptr(np.zeros(64))

    def process(rows=d, R=1, P=4, f64=1, thr=0.15):
        _lib.check(lib.cobel_activity_process(rows, R, P, f64, thr, None))

    with pytest.raises(AssertionError, match='NULL rows'):
        process(rows=None)
    with pytest.raises(IndexError, match='-1 rows'):
        process(R=-1)
    with pytest.raises(IndexError, match='of 0 elements'):
        process(P=0)
    process(R=0)

    out = (C.c_int32 * 4)()
    with pytest.raises(AssertionError, match='NULL out'):
        _lib.check(lib.cobel_place_fields_plan(5, 5, 0, None))
    for H, W in ((0, 5), (5, 0), (-1, 1)):
        with pytest.raises(IndexError, match=r'%d x %d cells' % (H, W)):
            _lib.check(lib.cobel_place_fields_plan(H, W, 0, C.byref(out)))
    with pytest.raises(NotImplementedError, match=r'at most 4096 cells .*got 64 x 65'):
        _lib.check(lib.cobel_place_fields_plan(64, 65, 0, C.byref(out)))
    for H, W, f64 in ((1, 1, 0), (32, 32, 0), (25, 25, 1), (64, 64, 0), (64, 64, 1), (1, 4096, 1)):
        _lib.check(lib.cobel_place_fields_plan(H, W, f64, C.byref(out)))
        lds, per_wg, per_map, threads = list(out)
        cells = H * W
        assert per_map >= cells * (8 if f64 else 4) + cells * 4 + 3 * 4 * ((cells + 1) // 2)
        assert per_map % 16 == 0 and lds == per_map * per_wg and threads == 64 * per_wg
        assert 1 <= per_wg <= 4 and (lds <= 64 * 1024 or per_wg == 1) and lds <= 160 * 1024

    def fields(maps=d, M=1, H=2, W=2, f64=1, cutoff=0.25, size=0.5, outs=(d, d, d, d, d)):
        _lib.check(lib.cobel_place_fields(maps, M, H, W, f64, cutoff, size, *outs, None))

    with pytest.raises(AssertionError, match='NULL maps or outputs'):
        fields(maps=None)
    for k in range(5):
        with pytest.raises(AssertionError, match='NULL maps or outputs'):
            fields(outs=tuple(None if i == k else d for i in range(5)))
    with pytest.raises(IndexError, match='0 x 2 cells'):
        fields(H=0)
    with pytest.raises(NotImplementedError, match='at most 4096 cells'):
        fields(H=4097, W=1)
    for size in (0.0, 1.0):
        with pytest.raises(AssertionError, match='The field size threshold is invalid!'):
            fields(size=size)
    for cutoff in (0.0, 1.0):
        with pytest.raises(AssertionError, match='The activity cutoff threshold is invalid!'):
            fields(cutoff=cutoff)
    with pytest.raises(IndexError, match='-1 maps'):
        fields(M=-1)
    fields(M=0)


# -- cobel_amd.analysis.network_spatial ------------------------------------------------------------------
def test_network_spatial_host_side():
    from cobel_amd.analysis import network_spatial as ns
    a = ac.named_maps(5, 7, np.float64)['blob']
    with pytest.raises(NotImplementedError, match='sigma'):
        ns.classify_place_field(a, sigma=1.0)
    with pytest.raises(NotImplementedError, match='sigma'):
        ns.classify_place_fields(a[None], sigma=0.5)
    with pytest.raises(AssertionError, match='The field size threshold is invalid!'):
        ns.classify_place_field(a, size_threshold=1.0)
    with pytest.raises(AssertionError, match='The activity cutoff threshold is invalid!'):
        ns.classify_place_field(a, cutoff=0.0)
    # calculate_pdist keeps the reference's literals: six head directions, rows of 25 cells
    rng = np.random.default_rng(0)
    sliced = rng.uniform(0, 1, (3, 6, 625))
    centers, vectors = ns.calculate_pdist(sliced, np.arange(3))
    assert centers.shape == (3, 15) and vectors.shape == (15,)
    want = np.array([[np.hypot(*np.subtract(divmod(int(np.argmax(sliced[i, p])), 25),
                                            divmod(int(np.argmax(sliced[i, q])), 25)))
                      for p in range(6) for q in range(p + 1, 6)] for i in range(3)])
    assert np.allclose(centers, want, rtol=0, atol=1e-12)
    spatial = pytest.importorskip('scipy.spatial.distance')
    assert np.array_equal(ns.pdist(sliced[0, :, :2]), spatial.pdist(sliced[0, :, :2]))


# -- the fixture recorded from the reference ------------------------------------------------------------
@pytest.fixture(scope='module')
def Z(golden):
    return golden('activity_traces')


def _close64(got, ref):      # mlp_gpu_common.agree's float64 rule
    return got.shape == ref.shape and np.allclose(got, ref, rtol=1e-9, atol=1e-12)


def test_restatement_equals_the_fixture(Z):
    torch = pytest.importorskip('torch')
    p, probes = ac.fixture_params(), ac.fixture_probes()
    for name, (_, _, _, hidden, requests) in ac.torch_models(torch, p).items():
        for k, (_, linear, apply) in enumerate(requests):
            assert _close64(ac.layer_activity(p, probes, linear, hidden, apply),
                            Z['activity/%s/%d' % (name, k)]), (name, k)
    for key, interval in ac.MONITOR_INTERVALS.items():
        # (monitor/network.py:103-115: ``last_update`` is reset at EVERY call, so an int interval
        #  above 1 records the first call and never again — kept as the reference has it)
        at, last = [], 1 + (interval if isinstance(interval, int) else 0)
        for t in range(ac.MONITOR_UPDATES):
            if isinstance(interval, tuple):
                record = t in interval
            else:
                record, last = last >= interval, 0
            at += [t] if record else []
            last += 1
        want = np.stack([ac.layer_activity(ac.monitor_params(t), probes[:5], 1, 'relu', 'none')
                         for t in at])
        assert _close64(want, Z['monitor/' + key]), key
    assert [len(Z['monitor/' + k]) for k in ('every', 'third', 'trials')] == [8, 1, 3]
    for dtype in (np.float32, np.float64):
        tag = np.dtype(dtype).name
        got = ac.process(ac.process_rows(33, dtype), 0.15)
        assert got.dtype == Z['process/' + tag].dtype
        assert np.array_equal(got, Z['process/' + tag], equal_nan=True)
        for H, W in ac.FIXTURE_SHAPES:
            named = ac.named_maps(H, W, dtype)
            has, _, _, _, fields = ac.classify_many(np.stack([named[k] for k in sorted(named)]))
            assert np.array_equal(has.astype(bool), Z['classify/%s/%dx%d/has' % (tag, H, W)])
            want = Z['classify/%s/%dx%d/fields' % (tag, H, W)]
            assert fields.dtype == want.dtype and np.array_equal(fields, want, equal_nan=True)
    for case, count in (('several', 2), ('one', 0), ('none', 0)):
        got = ac.place_like(ac.place_like_fields(case), (25, 25))
        for k, a in zip(('f', 'ids', 'pd', 'v'), got):
            want = Z['place_like/%s/%s' % (case, k)]
            assert np.asarray(a).shape == want.shape and np.array_equal(a, want), (case, k)
        assert len(got[1]) == count      # (exactly one qualifying unit: the reference drops it)


def test_generator_reruns_bit_identically(Z, tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_activity.py')],
                          env=env)
    fresh = np.load(tmp_path / 'activity_traces.npz')
    assert sorted(fresh.files) == sorted(Z.files)
    for k in Z.files:
        assert fresh[k].dtype == Z[k].dtype and fresh[k].tobytes() == Z[k].tobytes(), k


def test_representation_monitor_equals_the_recorded_traces(Z):
    torch = pytest.importorskip('torch')
    import types
    from cobel_amd.monitor import RepresentationMonitor
    from cobel_amd.network import TorchNetwork
    assert 'PyQt6' not in sys.modules and 'pyqtgraph' not in sys.modules
    probes = ac.fixture_probes()
    for key, interval in ac.MONITOR_INTERVALS.items():
        model, names, activations, _, _ = ac.torch_models(torch, ac.fixture_params())['custom_relu']
        agent = types.SimpleNamespace(model_online=TorchNetwork(model, activations=activations))
        monitor = RepresentationMonitor('model_online', 'fc2', probes[:5], interval)
        for t in range(ac.MONITOR_UPDATES):
            ac.load_params(torch, model, names, ac.monitor_params(t))
            monitor.update({'agent': agent, 'trial': t})
        got = monitor.get_trace()
        assert _close64(got, Z['monitor/' + key]), key
        monitor.clear_plots()
    for bad in (-1, (-1, 2)):
        with pytest.raises(AssertionError):
            RepresentationMonitor('model_online', 'fc2', probes, bad)


def test_single_network_activity_equals_the_fixture(Z):
    torch = pytest.importorskip('torch')
    from cobel_amd.analysis import network_spatial as ns
    from cobel_amd.network import TorchNetwork
    probes = ac.fixture_probes()
    for name, (model, _, activations, _, requests) in ac.torch_models(torch, ac.fixture_params()).items():
        net = TorchNetwork(model, activations=activations)
        for k, (layer, _, _) in enumerate(requests):
            want = Z['activity/%s/%d' % (name, k)]
            assert _close64(net.get_layer_activity(probes, layer), want)
            assert _close64(ns.get_activity_maps(probes, net, layer), want[[0]])
            assert _close64(ns.get_activity_maps(probes, net, layer, np.array([2, 0])), want[[2, 0]])


def test_routing_table():
    """Which requests the stack hands to cobel_mlp_activity, and as what."""
    torch = pytest.importorskip('torch')
    from cobel_amd import _lib
    from cobel_amd.network import TorchNetwork
    apply = {'none': _lib.APPLY_NONE, 'relu': _lib.APPLY_RELU, 'tanh': _lib.APPLY_TANH}
    nn, F = torch.nn, torch.nn.functional
    for name, (model, _, activations, hidden, requests) in ac.torch_models(torch, ac.fixture_params()).items():
        stack = TorchNetwork(model, activations=activations).replicate(3)
        assert stack.activations is not activations and len(stack.activations) == len(activations)
        for layer, linear, how in requests:
            assert stack._activity_route(layer) == (linear, apply[how], hidden), (name, layer)
        stack.fused_mlp = False
        assert all(stack._activity_route(layer) is None for layer, _, _ in requests)
    # the other spellings of the two activations
    model, _, _, _, _ = ac.torch_models(torch, ac.fixture_params())['custom_relu']
    spellings = {'fc1': F.relu, 'fc2': nn.Tanh(), 'fc3': nn.ReLU()}
    stack = TorchNetwork(model, activations=spellings).replicate(2)
    assert [stack._activity_route(k)[1] for k in ('fc1', 'fc2', 'fc3')] == \
        [_lib.APPLY_RELU, _lib.APPLY_TANH, _lib.APPLY_RELU]
    # fallbacks: another function, a network the kernels do not cover, a module of a custom forward
    stack = TorchNetwork(model, activations={'fc1': torch.sigmoid, 'fc2': None}).replicate(2)
    assert stack._activity_route('fc1') is None and stack._activity_route('fc2') is not None
    with pytest.raises(AssertionError, match='Key not in activation dict!'):
        stack._activity_route('fc3')
    wide = nn.Sequential(nn.Linear(7, 48), nn.ReLU(), nn.Linear(48, 48), nn.ReLU(), nn.Linear(48, 4))
    stack = TorchNetwork(wide.double(), activations=[None] * 5).replicate(2)
    assert all(stack._activity_route(k) is None for k in range(5))
    stack = TorchNetwork(wide.double(), activations=(None,) * 5).replicate(2)
    with pytest.raises(AssertionError, match='String layerkeys not compatible'):
        stack._activity_route('0')
    stack = TorchNetwork(wide.double(), activations=[None]).replicate(2)
    with pytest.raises(AssertionError, match='Index not in activation list!'):
        stack._activity_route(3)
    # the PyTorch path serves what the kernel does not, with the reference's semantics (CPU stack)
    model, _, _, _, _ = ac.torch_models(torch, ac.fixture_params())['custom_relu']
    stack = TorchNetwork(model, activations={'fc1': torch.sigmoid}).replicate(2)
    probes = ac.fixture_probes()
    got = stack.get_layer_activity(probes, 'fc1', units=[3, 1])
    pre = ac.layer_activity(ac.fixture_params(), probes, 0, 'relu', 'none')
    assert got.shape == (2, 2, ac.FIXTURE_P)
    assert _close64(got[1], (1.0 / (1.0 + np.exp(-pre)))[[3, 1]])
