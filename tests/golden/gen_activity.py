"""Golden records of the reference's network-representation tooling — TorchNetwork.get_layer_activity
(network/network_torch.py), RepresentationMonitor (monitor/network.py) and
analysis/network_spatial.py (on scipy) — recorded from the real reference:

  activity/<model>/<k>   get_layer_activity of the seeded 7-64-64-4 network of
                         tests/activity_common.py (``torch_models``: a custom-forward module with an
                         ``activations`` dict and an nn.Sequential with a list, ReLU and tanh) for
                         every request of its table, on 40 probe rows
  monitor/<interval>     RepresentationMonitor('model_online', 'fc2', probes[:5], interval).get_trace()
                         after eight ``update`` calls (trials 0 .. 7) with the network of
                         ``monitor_params(t)`` at call t, for interval 0, 3 and (0, 2, 5)
  process/<dtype>        process_activity_maps of ``process_rows(33, dtype)`` (a constant row, rows
                         with NaN and infinities among them), threshold 0.15
  classify/<dtype>/<H>x<W>/{has,fields}   classify_place_field over ``named_maps(H, W, dtype)`` in
                         sorted order
  place_like/<case>/{f,ids,pd,v}          place_like on ``place_like_fields(case)`` at (25, 25)

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_activity.py

Reuses the shim of gen_golden.py (the reference's monitor imports pyqtgraph).  Writes
activity_traces.npz.
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import activity_common as ac  # noqa: E402


def main() -> None:
    import torch
    from cobel.analysis import network_spatial as ns
    from cobel.monitor.network import RepresentationMonitor
    from cobel.network import TorchNetwork
    torch.set_num_threads(1)
    warnings.simplefilter('ignore', RuntimeWarning)
    Z = {}
    probes = ac.fixture_probes()
    for name, (model, _, activations, _, requests) in ac.torch_models(torch, ac.fixture_params()).items():
        net = TorchNetwork(model, activations=activations)
        for k, (layer, _, _) in enumerate(requests):
            Z['activity/%s/%d' % (name, k)] = np.asarray(net.get_layer_activity(probes, layer))
    for key, interval in ac.MONITOR_INTERVALS.items():
        model, names, activations, _, _ = ac.torch_models(torch, ac.fixture_params())['custom_relu']
        agent = types.SimpleNamespace(model_online=TorchNetwork(model, activations=activations))
        monitor = RepresentationMonitor('model_online', 'fc2', probes[:5], interval)
        for t in range(ac.MONITOR_UPDATES):
            ac.load_params(torch, model, names, ac.monitor_params(t))
            monitor.update({'agent': agent, 'trial': t})
        Z['monitor/' + key] = monitor.get_trace()
    for dtype in (np.float32, np.float64):
        tag = np.dtype(dtype).name
        Z['process/' + tag] = ns.process_activity_maps(ac.process_rows(33, dtype).copy(), 0.15)
        for H, W in ac.FIXTURE_SHAPES:
            named = ac.named_maps(H, W, dtype)
            got = [ns.classify_place_field(named[k]) for k in sorted(named)]
            Z['classify/%s/%dx%d/has' % (tag, H, W)] = np.array([g[0] for g in got])
            Z['classify/%s/%dx%d/fields' % (tag, H, W)] = np.stack([g[1] for g in got])
    for case in ('several', 'one', 'none'):
        got = ns.place_like(ac.place_like_fields(case), (25, 25))
        for k, a in zip(('f', 'ids', 'pd', 'v'), got):
            Z['place_like/%s/%s' % (case, k)] = np.asarray(a)
    np.savez_compressed(G._out('activity_traces.npz'), **Z)
    print('activity_traces.npz: %d arrays' % len(Z))


if __name__ == '__main__':
    main()
