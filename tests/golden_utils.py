"""Load the committed golden vectors (tests/golden/*.npz, produced by tests/golden/make_golden.py)."""
import os

import numpy as np
import torch

from cartnet_amd.data import Batch, Data
from cartnet_amd.model import make_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_FIXTURES = ["tiny_adp", "tiny_scalar", "tiny_invariant", "tiny_noatom", "tiny_nothing", "config1", "config2",
                  "tiny_radius6", "tiny_radius4"]

# Cells (a, b, c, alpha, beta, gamma) away from the nearly cubic ones of cartnet_amd.synthetic: the radius-graph tests and
# the radius_graph_radii fixture share them.
CELLS = {"hexagonal": (4.1, 4.1, 9.7, 90.0, 90.0, 120.0), "rhombohedral": (5.3, 5.3, 5.3, 50.0, 50.0, 50.0),
         "triclinic": (3.4, 6.2, 8.8, 67.0, 104.0, 118.0), "small": (2.6, 2.9, 3.3, 85.0, 95.0, 100.0)}
# (radius, y): cell 20 I, atoms at (0, 0, 0) and (3, y, 0).  The pair's fp32 d^2 equals fp32(radius) * fp32(radius) and lies
# one ulp above fp32(radius * radius), the reference's threshold (dataset/utils.py:202 takes the product in double).
THRESHOLD_PAIRS = [(3.7, 2.1656408309936523), (4.3, 3.0805845260620117)]


def lattice(a, b, c, alpha, beta, gamma):
    """fp32 [3,3] cell (rows = lattice vectors) in the standard setting: a1 along x, a2 in the xy plane."""
    al, be, ga = (np.deg2rad(v) for v in (alpha, beta, gamma))
    cy = (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    m = np.array([[a, 0.0, 0.0], [b * np.cos(ga), b * np.sin(ga), 0.0],
                  [c * np.cos(be), c * cy, c * np.sqrt(1.0 - np.cos(be) ** 2 - cy ** 2)]])
    return torch.from_numpy(m).to(torch.float32)


def crystal(name, n, seed, rotate=False):
    """(pos [n,3], cell [3,3]) fp32: ``n`` atoms at uniform fractional coordinates in CELLS[name], optionally rotated."""
    from cartnet_amd.synthetic import random_rotation
    gen = torch.Generator().manual_seed(seed)
    cell = lattice(*CELLS[name])
    if rotate:
        cell = cell @ random_rotation(gen)
    return torch.rand(n, 3, generator=gen, dtype=torch.float32) @ cell, cell


def threshold_pair(y):
    return torch.tensor([[0.0, 0.0, 0.0], [3.0, y, 0.0]], dtype=torch.float32), 20.0 * torch.eye(3)


def geometry(pos, cell):
    """A crystal without edges: what a geometry-only shard is packed from."""
    n = pos.shape[0]
    return Data(x=torch.full((n,), 6, dtype=torch.int64), pos=pos.clone(), cell=cell.reshape(1, 3, 3).clone(),
                y=torch.zeros(1))


def ragged():
    """1, 2, 3, 40, 64, 65 and 70 atoms (more than one 64-source round; 251 atoms in all, no multiple of 4), a sheared
    cell, a cell edge shorter than the radius, and a two-atom crystal in a 30 A cell (no edges) first, in the middle, last."""
    far = (torch.tensor([[1.0, 2.0, 3.0], [16.0, 17.0, 14.0]]), 30.0 * torch.eye(3))
    sheared = torch.tensor([[9.0, 0.0, 0.0], [6.5, 8.0, 0.0], [-4.0, 3.0, 10.0]])
    gen = torch.Generator().manual_seed(11)
    geo = [far, crystal("hexagonal", 1, 1), crystal("triclinic", 2, 2), crystal("small", 3, 3),
           (torch.rand(40, 3, generator=gen) @ sheared, sheared), far, crystal("rhombohedral", 64, 4, rotate=True),
           (torch.rand(65, 3, generator=gen) @ (1.4 * sheared), 1.4 * sheared), crystal("triclinic", 70, 5), far]
    assert sum(p.shape[0] for p, _ in geo) == 251
    return [geometry(p, c) for p, c in geo]


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp_")}
    b = Batch()
    for k in z.files:
        if k.startswith("in_") and k != "in_num_graphs":
            setattr(b, k[3:], torch.from_numpy(z[k]))
    b.num_graphs = int(z["in_num_graphs"])
    if any(k.startswith("w_") for k in z.files):
        sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w_")}
    else:
        sd = make_state_dict(hp["dim_in"], hp["dim_rbf"], hp["num_layers"], seed=int(z["weights_seed"]),
                             cholesky=hp["cholesky"], temperature=hp["temperature"], atom_types=hp["atom_types"],
                             invariant=hp["invariant"], radius=hp["radius"])
    abs_sum = sum(v.double().abs().sum().item() for v in sd.values())
    assert abs(abs_sum - float(z["weights_abs_sum"])) <= 1e-9 * abs(float(z["weights_abs_sum"])), \
        "regenerated weights differ from the ones the fixture was made with"
    return z, hp, b, sd


def clone_batch(b):
    c = b.clone()
    c.num_graphs = b.num_graphs
    return c


def oracle_kwargs(hp):
    return dict(num_layers=hp["num_layers"], radius=hp["radius"], envelope_radius=hp.get("env_radius", hp["radius"]),
                invariant=hp["invariant"],
                use_temperature=hp["temperature"], use_envelope=hp["use_envelope"], atom_types=hp["atom_types"],
                cholesky=hp["cholesky"])
