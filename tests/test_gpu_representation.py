"""The Python surface of the representation tooling on the GPU: StackedTorchNetwork's layer
activity by kernel against its PyTorch path, RepresentationMonitor on a DQN that trains one network
per instance, and the chain activity -> process -> classify on the device, each stage compared
with the NumPy restatement applied to the previous stage's device output (a cutoff is
discontinuous: end to end, last-bit differences of the activity would flip cells)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activity_common as ac  # noqa: E402

from mlp_gpu_common import _dev, _host, agree  # noqa: E402

pytestmark = pytest.mark.gpu

FIGURES = {}


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def _stack(torch, name, n, dtype):
    """A stack of n different networks of the fixture's architecture ``name`` on the GPU."""
    from cobel_amd.network import TorchNetwork
    model, names, activations, hidden, requests = ac.torch_models(torch, ac.fixture_params())[name]
    if dtype == 'f32':
        model = model.float()
    stack = TorchNetwork(model, activations=activations, device='cuda').replicate(n)
    rng = np.random.default_rng(n)
    with torch.no_grad():
        for k, v in stack.params.items():
            v.mul_(_dev(torch, rng.uniform(0.5, 1.5, (n,) + (1,) * (v.dim() - 1))).to(v.dtype))
    return stack, requests


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['custom_relu', 'custom_tanh', 'sequential_relu',
                                  'sequential_tanh'])
def test_kernel_path_against_the_pytorch_path(torch_cuda, name, dtype):
    torch = torch_cuda
    n, P = 3, 37
    stack, requests = _stack(torch, name, n, dtype)
    np_dtype = np.float64 if dtype == 'f64' else np.float32
    rng = np.random.default_rng(5)
    shared = rng.standard_normal((P, ac.FIXTURE_D)).astype(np_dtype)
    own = rng.standard_normal((n, P, ac.FIXTURE_D)).astype(np_dtype)
    names = ac.torch_models(torch, ac.fixture_params())[name][1]
    hidden = ac.torch_models(torch, ac.fixture_params())[name][3]
    params = {}
    for i, key in enumerate(names):
        params['w%d' % (i + 1)] = _host(stack.params[key + '.weight'])
        params['b%d' % (i + 1)] = _host(stack.params[key + '.bias'])
    for layer, linear, how in requests:
        assert stack._activity_route(layer) is not None
        for probes in (shared, own):
            for units in (None, [5, 0, 5] if linear < 2 else [3, 0, 3]):
                stack.fused_mlp = True
                got = stack.get_layer_activity(probes, layer, units)
                on_device = stack.layer_activity_on_device(_dev(torch, probes), layer, units)
                assert on_device.is_cuda and _host(on_device).tobytes() == got.tobytes()
                stack.fused_mlp = False
                ref = stack.get_layer_activity(probes, layer, units)
                stack.fused_mlp = True
                rows = len(units) if units else (ac.FIXTURE_O if linear == 2 else 64)
                assert got.shape == ref.shape == (n, rows, P)
                assert got.dtype == ref.dtype == np_dtype
                if dtype == 'f64':
                    agree(FIGURES, (name, layer), dtype, got, ref)
                else:       # the PyTorch path is torch's float32: the yardstick of the rule
                    ref64 = ac.stack_activity(params, probes, linear, hidden, how, units)
                    agree(FIGURES, (name, layer), dtype, got, ref64, torch.from_numpy(ref))


def _train_dqn(torch, n_envs, monitor, trains, trials):
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Topology
    from cobel_amd.misc.topology_tools import linear_track
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    nodes, starts = linear_track(10, 2, 1., 20., 'right')
    torch.manual_seed(3)
    env = Topology(nodes, starts, n_envs=n_envs, seed=7)
    D, A = int(np.prod(env.observation_space.shape)), int(env.action_space.n)
    nn = torch.nn

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.layer_dense_1, self.layer_dense_2 = nn.Linear(D, 64), nn.Linear(64, 64)
            self.layer_output = nn.Linear(64, A)
            self.double()

        def forward(self, x):
            x = torch.relu(self.layer_dense_1(torch.reshape(x, (len(x), -1))))
            return self.layer_output(torch.relu(self.layer_dense_2(x)))

    net = TorchNetwork(Model(), activations={'layer_dense_2': torch.relu}, device='cuda')
    agent = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.3), net, gamma=0.8,
                custom_callbacks={'on_trial_end': [monitor.update]})
    for _ in range(trains):
        agent.train(env, trials, 20, 32)
    torch.cuda.synchronize()
    return agent, D


def test_monitor_records_every_instance(torch_cuda):
    torch = torch_cuda
    from cobel_amd.monitor import RepresentationMonitor
    observations = np.random.default_rng(0).uniform(0, 1, (9, 6))
    monitor = RepresentationMonitor('model_online', 'layer_dense_2', observations)
    agent, D = _train_dqn(torch, 4, monitor, trains=2, trials=1)
    assert D == observations.shape[1]
    trace = monitor.get_trace()
    assert trace.shape == (2, 4, 64, 9) and trace.dtype == np.float64
    after = agent.model_online.get_layer_activity(observations, 'layer_dense_2')
    assert np.allclose(trace[1, 0], after, rtol=1e-9, atol=1e-12)
    assert (trace >= 0).all() and not np.array_equal(trace[0], trace[1])
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(trace[1, a], trace[1, b]), (a, b)


def test_monitor_single_instance_at_given_trials(torch_cuda):
    torch = torch_cuda
    from cobel_amd.monitor import RepresentationMonitor
    observations = np.random.default_rng(0).uniform(0, 1, (9, 6))
    monitor = RepresentationMonitor('model_online', 'layer_dense_2', observations, interval=(0, 2))
    agent, _ = _train_dqn(torch, 1, monitor, trains=1, trials=4)
    trace = monitor.get_trace()
    assert trace.shape == (2, 64, 9)
    assert not np.array_equal(trace[0], trace[1])


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_chain_on_the_device(torch_cuda, dtype):
    torch = torch_cuda
    from cobel_amd.analysis import network_spatial as ns
    n, H, W = 3, 9, 11
    stack, _ = _stack(torch, 'custom_tanh', n, dtype)
    np_dtype = np.float64 if dtype == 'f64' else np.float32
    ys, xs = np.meshgrid(np.linspace(-2, 2, H), np.linspace(-2, 2, W), indexing='ij')
    probes = np.zeros((H * W, ac.FIXTURE_D), dtype=np_dtype)
    probes[:, 0], probes[:, 1] = ys.ravel(), xs.ravel()
    units = np.arange(0, 64, 3)
    activity = stack.layer_activity_on_device(_dev(torch, probes), 'fc2', units)
    assert tuple(activity.shape) == (n, len(units), H * W)
    stage1 = _host(activity)
    assert np.array_equal(ns.get_activity_maps(probes, stack, 'fc2', units), stage1)
    assert ns.process_activity_maps(activity, 0.6) is activity
    stage2 = _host(activity)
    want2 = ac.process(stage1.reshape(-1, H * W), 0.6).reshape(stage1.shape)
    assert np.array_equal(stage2, want2, equal_nan=True)
    has, fields, info = ns.classify_place_fields(activity.view(n, len(units), H, W))
    want = ac.classify_many(stage2.reshape(-1, H, W))
    assert np.array_equal(_host(has).reshape(-1), want[0].astype(bool))
    for k, w in (('error', want[1]), ('features', want[2]), ('largest_area', want[3])):
        assert np.array_equal(_host(info[k]).reshape(-1), w), k
    assert np.array_equal(_host(fields).reshape(-1, H, W), want[4], equal_nan=True)
    assert len(set(want[1].tolist())) > 1          # (the maps do not all end the same way)
