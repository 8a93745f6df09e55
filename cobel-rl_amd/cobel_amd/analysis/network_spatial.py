"""The reference's ``analysis/network_spatial.py`` with the per-map work on the device: activity
maps are normalised by ``cobel_activity_process`` and classified by ``cobel_place_fields``, any
number of them in one launch.  Plumbing only: NumPy arrays are moved to the device and back,
device tensors stay where they are.  There is no host fall-back for the kernels."""
from __future__ import annotations

import numpy as np

from .. import _lib

_ERRORS = {0: '', 1: 'no blobs found', 2: 'too many blobs', 3: 'too large'}


def _device():
    import torch
    assert torch.cuda.is_available(), 'the activity analysis runs on the GPU'
    return torch.device('cuda', torch.cuda.current_device())


def _is_tensor(x) -> bool:
    return hasattr(x, 'data_ptr')


def get_activity_maps(observations, model, layer, units=None):
    """The unit activations of ``layer`` for a set of observations: ``[K, P]`` for a single network
    (``units`` None: unit 0, as the reference), ``[n, K, P]`` for a stack of networks."""
    if hasattr(model, 'layer_activity_on_device'):
        return np.copy(model.get_layer_activity(observations, layer, units))
    return np.copy(model.get_layer_activity(observations, layer)[
        np.array([0]) if units is None else units, :])


def process_activity_maps(activity_maps, threshold: float = 0.15):
    """Normalise every map (the last axis) to 0 .. 1 and zero what lies below ``threshold``, in
    place; the argument is returned.  An ndarray or a device tensor with any leading axes."""
    import torch
    tensor = _is_tensor(activity_maps)
    if tensor:
        assert activity_maps.is_cuda and activity_maps.is_contiguous(), \
            'a contiguous device tensor (or an ndarray) is expected'
        dev = activity_maps
    else:
        assert activity_maps.dtype in (np.float32, np.float64), 'float32 or float64 maps are covered'
        dev = torch.from_numpy(np.ascontiguousarray(activity_maps)).to(_device())
    assert dev.dtype in (torch.float32, torch.float64), 'float32 or float64 maps are covered'
    cols = int(dev.shape[-1])
    rows = int(dev.numel() // cols) if cols else 0
    _lib.check(_lib.lib().cobel_activity_process(
        _lib.ptr(dev), rows, cols, int(dev.dtype == torch.float64), float(threshold),
        _lib.current_stream(dev.device)))
    if not tensor:
        activity_maps[...] = dev.cpu().numpy()
    return activity_maps


def classify_place_fields(maps, sigma: float = 0., size_threshold: float = 0.5,
                          cutoff: float = 0.25):
    """``classify_place_field`` for maps ``[..., H, W]`` in one launch: ``(has_field [...] bool,
    fields [..., H, W], info)`` with ``info`` the ``error`` code (0 none, 1 no blobs found, 2 too
    many blobs, 3 too large), the number of ``features`` and the bounding-box area
    ``largest_area`` of the largest one, each ``[...]``.  NumPy in, NumPy out; tensors stay on the
    device."""
    import torch
    if sigma != 0:
        raise NotImplementedError('sigma = %r: Gaussian smoothing of the field (sigma > 0) is not '
                                  'covered, only sigma = 0' % (sigma,))
    assert size_threshold > 0 and size_threshold < 1, 'The field size threshold is invalid!'
    assert cutoff > 0 and cutoff < 1, 'The activity cutoff threshold is invalid!'
    tensor = _is_tensor(maps)
    if tensor:
        assert maps.is_cuda, 'a device tensor (or an ndarray) is expected'
        dev = maps.contiguous()
    else:
        maps = np.asarray(maps)
        assert maps.dtype in (np.float32, np.float64), 'float32 or float64 maps are covered'
        dev = torch.from_numpy(np.ascontiguousarray(maps)).to(_device())
    assert dev.dtype in (torch.float32, torch.float64), 'float32 or float64 maps are covered'
    assert dev.dim() >= 2, 'maps [..., H, W]'
    lead, (H, W) = tuple(dev.shape[:-2]), (int(dev.shape[-2]), int(dev.shape[-1]))
    M = int(np.prod(lead, dtype=np.int64))
    has = torch.empty(lead, dtype=torch.uint8, device=dev.device)
    info = {k: torch.empty(lead, dtype=torch.int32, device=dev.device)
            for k in ('error', 'features', 'largest_area')}
    fields = torch.empty_like(dev)
    _lib.check(_lib.lib().cobel_place_fields(
        _lib.ptr(dev), M, H, W, int(dev.dtype == torch.float64), float(cutoff),
        float(size_threshold), _lib.ptr(has), _lib.ptr(info['error']), _lib.ptr(info['features']),
        _lib.ptr(info['largest_area']), _lib.ptr(fields), _lib.current_stream(dev.device)))
    has = has.bool()
    if tensor:
        return has, fields, info
    return has.cpu().numpy(), fields.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}


def classify_place_field(activity_map, sigma: float = 0., size_threshold: float = 0.5,
                         cutoff: float = 0.25, verbose: bool = False):
    """Whether a 2-d map of spatial activations contains a place field, and the (thresholded)
    field of its largest blob."""
    has, fields, info = classify_place_fields(np.asarray(activity_map)[None], sigma, size_threshold,
                                              cutoff)
    has_field = bool(has[0])
    print(('%s, not place like' % _ERRORS[int(info['error'][0])]) * (not has_field) * verbose,
          end='\n' * (not has_field) * verbose)
    return has_field, fields[0]


def pdist(points):
    """Euclidean distances between the rows of ``points`` [m, k] in the order (0, 1), (0, 2), ...,
    (m - 2, m - 1) — scipy.spatial.distance.pdist's."""
    points = np.asarray(points, dtype=np.float64)
    i, j = np.triu_indices(points.shape[0], k=1)
    return np.sqrt(((points[i] - points[j]) ** 2).sum(axis=1))


def calculate_pdist(fields_sliced, place_indices):
    """The pairwise distances between the field centers of each unit's six head directions, and
    between the six direction vectors."""
    centers = np.zeros((max(1, len(place_indices)), 6, 2))
    for i, field in enumerate(fields_sliced):
        for j, angle in enumerate(field):
            centers[i, j] = divmod(np.argmax(angle), 25)
    pdist_centers = np.array([pdist(centers[i]) for i in range(len(centers))])
    angles = np.deg2rad(np.arange(0, 360, 60, dtype='int32').reshape(-1, 1))
    vectors = np.squeeze(np.array([(np.cos(a), np.sin(a)) for a in angles]))
    return pdist_centers, pdist(vectors)


def place_like(fields, resolution: tuple, sigma: float = 0., size_threshold: float = 0.5,
               cutoff: float = 0.25, verbose: bool = False):
    """The place-like units of ``fields`` [trials, area, units]: every trial's map and the mean map
    of a unit must hold a place field, and the field centers must not move with head direction.
    All maps are classified in one launch; the rest is the reference's host code in its order."""
    area, n_units = np.prod(resolution), fields.shape[2]
    mean_fields = np.mean(fields, axis=0).reshape((1, area, n_units))
    stacked = np.vstack((fields, mean_fields))
    maps = np.ascontiguousarray(np.rollaxis(stacked, 2)).reshape(
        (n_units, stacked.shape[0]) + tuple(resolution))
    has, big, info = classify_place_fields(maps, sigma, size_threshold, cutoff)
    is_field = np.zeros((stacked.shape[0], n_units))
    largest_field = np.zeros((stacked.shape[0], area, n_units))
    print('Place' * verbose, end='\n' * verbose)
    for i in range(n_units):
        print(('Unit %d' % i) * verbose, end='\n' * verbose)
        for j in range(stacked.shape[0]):
            print(('Head direction %d' % j) * verbose, end='\n' * verbose)
            isit = bool(has[i, j])
            print(('%s, not place like' % _ERRORS[int(info['error'][i, j])]) * (not isit) * verbose,
                  end='\n' * (not isit) * verbose)
    is_field[:, :] = has.T
    largest_field[:, :, :] = np.moveaxis(big.reshape(n_units, stacked.shape[0], area), 0, 2)
    # if all fields and the mean are classified, it may be a place like representation
    ids = np.squeeze(np.array(np.where(np.all(is_field, axis=0))))
    if ids.shape != () and ids.size > 0:
        f = np.array([largest_field[:, :, p] for p in ids])
        pd, v = calculate_pdist(f[:, :6, :], ids)
    else:
        f = np.array([largest_field[:, :, ids]])
        pd, v = np.full((1, 15), 15), np.full((1, 15), 15)
        print(('no slice found--' + str(ids)) * verbose, end='\n' * verbose)
    # if there is too much directional modulation, not field
    x_all = np.all(np.array(pd) < 10, axis=1)
    ids = np.where(x_all, ids, -1)
    ids = ids[ids != -1]
    f = np.array([largest_field[:, :, p] for p in ids])
    if ids.size > 0:
        pd, v = calculate_pdist(f[:, :6, :], ids)
    else:
        print(('no slice found--' + str(ids)) * verbose, end='\n' * verbose)
        pd = np.full((1, 15), 15)
    return f, ids, pd, v
