"""Layer activity and place-field classification at scale (docs/MEASUREMENTS.md section 23).

cobel_mlp_activity: N networks of 32-64-64-4, P probe rows shared by all, layer 1 through ReLU, in
both dtypes, against (a) PyTorch on the same stacked parameters — two batched GEMMs with bias and
ReLU, then the transpose to units-major — and (b) P / 32 calls of cobel_mlp_forward (which computes
one layer more and returns the outputs, not the layer: what a caller had before).

cobel_place_fields: M maps of 32 x 32 in float32, random sparse maps and the serpentine (the longest
single component) in every slot, against the NumPy restatement of tests/activity_common.py — and
scipy.ndimage, where it is installed — on one host core for 1 000 of the random maps.

Times are medians over --repeats launches between device events, after one warm-up.  Prints one
JSON line.

    python scripts/bench_activity.py [--n 8192] [--probes 1024] [--maps 524288] [--repeats 7]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import activity_common as ac  # noqa: E402
import mlp_common as mc  # noqa: E402


def _median_ms(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def bench_activity(torch, _lib, n, P, dtype, repeats):
    D, O = 32, 4
    rng = np.random.default_rng(1)
    stack = {k: torch.from_numpy(v).cuda() for k, v in mc.draw_networks(rng, n, D, O, dtype).items()}
    probes = torch.from_numpy(rng.standard_normal((P, D)).astype(dtype)).cuda()
    out = torch.empty((n, 64, P), dtype=probes.dtype, device='cuda')
    run = ac.fill_activity(_lib, stack, probes, out, n, P, D, O, 1, 'relu', 'relu')
    lib = _lib.lib()

    def kernel():
        _lib.check(lib.cobel_mlp_activity(C.byref(run), None))

    w1t, w2t = stack['w1'].transpose(1, 2).contiguous(), stack['w2'].transpose(1, 2).contiguous()
    x = probes.unsqueeze(0).expand(n, P, D)

    def pytorch():
        h1 = torch.relu(torch.baddbmm(stack['b1'].unsqueeze(1), x, w1t))
        h2 = torch.relu(torch.baddbmm(stack['b2'].unsqueeze(1), h1, w2t))
        return h2.transpose(1, 2).contiguous()

    dense = probes[:32].unsqueeze(0).expand(n, 32, D).contiguous()
    q = torch.empty((n, 32, O), dtype=probes.dtype, device='cuda')
    fwd = mc.fill_forward(_lib, stack, q, n, D, O, in_dense=dense)

    def forwards():
        for _ in range(P // 32):
            _lib.check(lib.cobel_mlp_forward(C.byref(fwd), None))

    kernel()
    ref = pytorch()
    worst = float((out - ref).abs().max())
    res = {'kernel_ms': _median_ms(torch, kernel, repeats),
           'pytorch_ms': _median_ms(torch, pytorch, repeats),
           'forward_calls_ms': _median_ms(torch, forwards, repeats),
           'max_abs_diff_to_pytorch': worst, 'out_gib': out.numel() * out.element_size() / 2 ** 30}
    res['pytorch_over_kernel'] = res['pytorch_ms'][0] / res['kernel_ms'][0]
    res['forward_calls_over_kernel'] = res['forward_calls_ms'][0] / res['kernel_ms'][0]
    return res


def bench_place_fields(torch, _lib, M, repeats):
    H = W = 32
    rng = np.random.default_rng(2)
    base = (rng.uniform(0, 1, (4096, H, W)) * (rng.random((4096, H, W)) < 0.4)).astype(np.float32)
    random_maps = torch.from_numpy(base).cuda().repeat((M + 4095) // 4096, 1, 1)[:M].contiguous()
    serp = torch.from_numpy(ac.serpentine(H, W).astype(np.float32)).cuda()
    serpentines = serp.unsqueeze(0).expand(M, H, W).contiguous()
    has = torch.empty(M, dtype=torch.uint8, device='cuda')
    ints = [torch.empty(M, dtype=torch.int32, device='cuda') for _ in range(3)]
    fields = torch.empty_like(random_maps)
    lib = _lib.lib()

    def launch(maps):
        def fn():
            _lib.check(lib.cobel_place_fields(_lib.ptr(maps), M, H, W, 0, 0.25, 0.5, _lib.ptr(has),
                                              *[_lib.ptr(t) for t in ints], _lib.ptr(fields), None))
        return fn

    res = {}
    for key, maps in (('random', random_maps), ('serpentine', serpentines)):
        ms = _median_ms(torch, launch(maps), repeats)
        res[key + '_ms'] = ms
        res[key + '_maps_per_s'] = M / (ms[0] * 1e-3)
    proc = random_maps.reshape(M, H * W).clone()
    res['process_ms'] = _median_ms(
        torch, lambda: _lib.check(lib.cobel_activity_process(_lib.ptr(proc), M, H * W, 0, 0.15, None)),
        repeats)
    t0 = time.perf_counter()
    ac.classify_many(base[:1000])
    res['host_restatement_maps_per_s'] = 1000 / (time.perf_counter() - t0)
    try:
        import scipy.ndimage as nd
    except ImportError:
        nd = None
    if nd is not None:
        t0 = time.perf_counter()
        for a in base[:1000]:
            field = np.where(a < 0.25 * np.max(a), 0, a)
            labels, features = nd.label(field > 0)
            if features:
                area = np.prod([field[s].shape for s in nd.find_objects(labels)], axis=1)
                field = np.where(labels == int(np.argmax(area)) + 1, field, 0)
        res['host_scipy_maps_per_s'] = 1000 / (time.perf_counter() - t0)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--probes', type=int, default=1024)
    ap.add_argument('--maps', type=int, default=524288)
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args()
    import torch
    from cobel_amd import _lib
    assert args.probes % 32 == 0
    out = {'n': args.n, 'probes': args.probes, 'maps': args.maps, 'repeats': args.repeats,
           'times': 'ms: [median, min, max]'}
    for name, dtype in (('f32', np.float32), ('f64', np.float64)):
        out['activity_' + name] = bench_activity(torch, _lib, args.n, args.probes, dtype, args.repeats)
        torch.cuda.empty_cache()
    out['place_fields'] = bench_place_fields(torch, _lib, args.maps, args.repeats)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
