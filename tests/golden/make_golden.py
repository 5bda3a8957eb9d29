"""Generate the golden vectors under tests/golden/ from the REFERENCE ITSELF (build container only).

Runs the reference's own ``models/cartnet.py`` (CartNet forward + autograd backward) and ``dataset/utils.py``
(radius_graph_pbc) imported read-only from /root/reference (see _ref_import.py for how its absent third-party
imports are stood in), on synthetic crystals from cartnet_amd.synthetic and weights from
cartnet_amd.model.make_state_dict, and stores inputs + outputs as plain arrays (.npz).  The reference's source
never enters the repo; only tensors do.

    python tests/golden/make_golden.py          # rewrites tests/golden/*.npz

Fixtures (all fp32 unless suffixed _f64):
  tiny_*      D=16, R=8, L=2, 2 crystals of 7/9 atoms, five model variants (all four Encoder branches of
              models/cartnet.py:111-121 + the scalar head); weights stored in the fixture
  config1     D=64, R=64, L=2, 4 crystals of 30..70 atoms (BASELINE.json configs[0] shape); weights from seed
  config2     D=256, R=64, L=4, 2 crystals of 194 atoms (configs[1] shape); weights from seed
  radius_graph  reference radius_graph_pbc output for 3 crystals (integers compared bit-exactly)
  tiny_radius6 / tiny_radius4   tiny_adp's shape under ``--radius 6`` / ``--radius 4`` as models/master.py runs it: the
              graph and every layer's envelope (cfg.radius) use the flag, the encoder's RBF keeps its default cutoff 5.0
  radius_graph_radii  reference radius_graph_pbc on a hexagonal and a triclinic cell at radius 3.7 and 6.0 (uncapped and
              cap 8), and on two pairs whose fp32 d^2 lies between fp32(radius^2) and fp32(radius)^2
  icomformer_tiny / icomformer_c32   the reference's iComformer (models/comformer.py) at C=16 / C=32
  train_epoch   the reference's own ``train_epoch`` (train/train.py:148-199) run for two epochs of five micro-batches
              with accumulation 3 (optimiser steps after micro-batches 3 and 5: the last-iteration flush), torch Adam as
              main.py:208 builds it and OneCycleLR as train/train.py:59 builds it: per optimiser step the accumulated
              gradient, the parameters after the step, the learning rate after ``scheduler.step()``; per iteration the
              logged loss / lr; BatchNorm buffers after each epoch
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))      # golden_utils: the cells and threshold pairs shared with the tests
sys.path.insert(0, HERE)

import golden_utils as gu  # noqa: E402
from _ref_import import import_reference  # noqa: E402

from cartnet_amd.data import Batch, Data  # noqa: E402
from cartnet_amd.model import make_state_dict  # noqa: E402
from cartnet_amd.synthetic import make_crystal, radius_graph_pbc_single  # noqa: E402

ref_cfg, ref_cartnet, ref_dutils = import_reference()


def to_np(t):
    return t.detach().cpu().numpy()


def batch_inputs(batch):
    out = {}
    for k in ("x", "batch", "ptr", "edge_index", "cart_dist", "cart_dir", "temperature", "non_H_mask", "y", "cell"):
        if hasattr(batch, k):
            out["in_" + k] = to_np(getattr(batch, k))
    out["in_num_graphs"] = np.int64(batch.num_graphs)
    return out


def clone_batch(batch, dtype=None):
    b = batch.clone()
    b.num_graphs = batch.num_graphs
    if dtype is not None:
        for k, v in list(b.__dict__.items()):
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(b, k, v.to(dtype))
    return b


def run_reference(sd, batch, hp, training, dtype=torch.float32, want_grads=False, trace=False):
    """One forward (+ backward) of the reference CartNet.  Returns dict of outputs."""
    ref_cfg.invariant = hp["invariant"]
    ref_cfg.radius = hp["env_radius"]            # models/cartnet.py:201: every layer's envelope reads the global
    torch.manual_seed(0)
    m = ref_cartnet.CartNet(dim_in=hp["dim_in"], dim_rbf=hp["dim_rbf"], num_layers=hp["num_layers"],
                            radius=hp["radius"], invariant=hp["invariant"], temperature=hp["temperature"],
                            use_envelope=hp["use_envelope"], atom_types=hp["atom_types"], cholesky=hp["cholesky"])
    missing = m.load_state_dict(sd, strict=True)     # also proves key / shape parity of make_state_dict
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.to(dtype)
    m.train(training)
    b = clone_batch(batch, dtype)
    out = {}
    if trace:
        b2 = clone_batch(batch, dtype)
        bb = m.encoder(b2)
        out["x0"], out["e0"] = to_np(bb.x), to_np(bb.edge_attr)
        for l, layer in enumerate(m.layers):
            bb = layer(bb)
            out[f"x{l + 1}"], out[f"e{l + 1}"] = to_np(bb.x), to_np(bb.edge_attr)
        # the trace pass updated running stats once; rebuild the module so the measured pass starts clean
        return {**out, **run_reference(sd, batch, hp, training, dtype, want_grads, trace=False)}
    pred, true = m(b)
    out["pred"] = to_np(pred)
    mae = torch.nn.functional.l1_loss(pred, true)          # train/metrics.py:26
    mse = torch.nn.functional.mse_loss(pred, true)         # train/metrics.py:27
    out["mae"], out["mse"] = to_np(mae), to_np(mse)
    if want_grads:
        mae.mean().backward()                              # train/train.py:183
        out["grads"] = {k: to_np(p.grad) for k, p in m.named_parameters()}
        out["new_state"] = {k: to_np(v) for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    return out


def hp_dict(dim_in, dim_rbf, num_layers, **kw):
    hp = dict(dim_in=dim_in, dim_rbf=dim_rbf, num_layers=num_layers, radius=5.0, invariant=False, temperature=True,
              use_envelope=True, atom_types=True, cholesky=True)
    hp.update(kw)
    hp.setdefault("env_radius", hp["radius"])    # cfg.radius (the layers' envelope); "radius" is the encoder's RBF cutoff
    return hp


def save_model_fixture(name, hp, batch, seed, store_weights, full_grads, trace):
    sd = make_state_dict(hp["dim_in"], hp["dim_rbf"], hp["num_layers"], seed=seed, cholesky=hp["cholesky"],
                         temperature=hp["temperature"], atom_types=hp["atom_types"], invariant=hp["invariant"],
                         radius=hp["radius"])
    arrays = batch_inputs(batch)
    for k, v in hp.items():
        arrays["hp_" + k] = np.array(v)
    arrays["weights_seed"] = np.int64(seed)
    arrays["weights_abs_sum"] = np.float64(sum(v.double().abs().sum().item() for v in sd.values()))
    if store_weights:
        for k, v in sd.items():
            arrays["w_" + k] = to_np(v)
    tr = run_reference(sd, batch, hp, True, torch.float32, want_grads=True, trace=trace)
    ev = run_reference(sd, batch, hp, False, torch.float32)
    tr64 = run_reference({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, batch, hp, True,
                         torch.float64, want_grads=True)
    ev64 = run_reference({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, batch, hp, False,
                         torch.float64)
    arrays["train_pred"], arrays["train_mae"], arrays["train_mse"] = tr["pred"], tr["mae"], tr["mse"]
    arrays["eval_pred"], arrays["eval_mae"] = ev["pred"], ev["mae"]
    arrays["train_pred_f64"], arrays["eval_pred_f64"] = tr64["pred"], ev64["pred"]
    if trace:
        for k, v in tr.items():
            if k[0] in "xe" and k[1:].isdigit():
                arrays["trace_" + k] = v
    for k, v in tr["new_state"].items():
        arrays["state_" + k] = v
    rng = np.random.default_rng(12345)
    for k, g in tr["grads"].items():
        g64 = tr64["grads"][k]
        if full_grads:
            arrays["grad_" + k] = g
            arrays["grad64_" + k] = g64.astype(np.float64)
        else:
            probe = rng.standard_normal(g.size)
            arrays["gradnorm_" + k] = np.float64(np.linalg.norm(g64.ravel()))
            arrays["gradprobe_" + k] = np.float64(np.dot(g64.ravel(), probe))
            arrays["gradhead_" + k] = g64.ravel()[:64].astype(np.float64)
            arrays["gradnorm32_" + k] = np.float64(np.linalg.norm(g.ravel().astype(np.float64)))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    err = np.abs(tr["pred"] - tr64["pred"]).max() / np.abs(tr64["pred"]).max()
    print(f"{name}: N={batch.x.shape[0]} E={batch.edge_index.shape[1]} fp32-vs-fp64 train err {err:.2e} "
          f"-> {os.path.getsize(path) / 1024:.0f} KiB")


def icomformer_fixture(name, dim, batch, seed, store_weights):
    """iComformer (BASELINE.json configs[4]) golden vectors from the reference's models/comformer.py."""
    import importlib
    import types
    for modname in ("e3nn", "e3nn.o3"):
        sys.modules.setdefault(modname, types.ModuleType(modname))
    sys.modules["e3nn"].o3 = sys.modules["e3nn.o3"]
    ref_cf = importlib.import_module("models.comformer")
    from cartnet_amd.comformer import make_icomformer_state_dict
    sd = make_icomformer_state_dict(dim, seed=seed)

    def run(training, dtype, want_grads):
        torch.manual_seed(0)
        m = ref_cf.iComformer(dim)
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        m = m.to(dtype)
        m.train(training)
        b = clone_batch(batch, dtype)
        pred, true = m(b)
        out = {"pred": to_np(pred), "x_final": to_np(b.x)}
        mae = torch.nn.functional.l1_loss(pred, true)
        out["mae"] = to_np(mae)
        if want_grads:
            mae.mean().backward()
            out["grads"] = {k: (to_np(p.grad) if p.grad is not None else None) for k, p in m.named_parameters()}
            out["new_state"] = {k: to_np(v) for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
        return out

    arrays = batch_inputs(batch)
    arrays["hp_dim_in"] = np.array(dim)
    arrays["weights_seed"] = np.int64(seed)
    arrays["weights_abs_sum"] = np.float64(sum(v.double().abs().sum().item() for v in sd.values()))
    if store_weights:
        for k, v in sd.items():
            arrays["w_" + k] = to_np(v)
    tr, ev = run(True, torch.float32, True), run(False, torch.float32, False)
    tr64, ev64 = run(True, torch.float64, True), run(False, torch.float64, False)
    arrays["train_pred"], arrays["train_mae"], arrays["eval_pred"] = tr["pred"], tr["mae"], ev["pred"]
    arrays["train_pred_f64"], arrays["eval_pred_f64"] = tr64["pred"], ev64["pred"]
    arrays["train_x_final_f64"] = tr64["x_final"]
    for k, v in tr["new_state"].items():
        arrays["state_" + k] = v
    unused = []
    for k, g in tr64["grads"].items():
        if g is None:
            unused.append(k)
            continue
        arrays["grad64_" + k] = g.astype(np.float64)
    arrays["unused_params"] = np.array(unused)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    err = np.abs(tr["pred"] - tr64["pred"]).max() / np.abs(tr64["pred"]).max()
    print(f"{name}: N={batch.x.shape[0]} E={batch.edge_index.shape[1]} fp32-vs-fp64 train err {err:.2e}, unused params "
          f"{unused} -> {os.path.getsize(path) / 1024:.0f} KiB")


def tiny_batch(adp=True, radius=5.0):
    items = [make_crystal(100, 7, radius=radius, adp=adp), make_crystal(101, 9, radius=radius, adp=adp)]
    return Batch.from_data_list(items)


def radius_batch(radius):
    """tiny_batch built with another cutoff, and the condition that makes the fixture tell the two radii apart."""
    b = tiny_batch(radius=radius)
    d, E = b.cart_dist, b.edge_index.shape[1]
    if radius > 5.0:
        far = int((d >= 5.0).sum())
        assert far >= 0.2 * E and bool((d < radius).all()), (far, E)      # RBF exactly 0, envelope positive
        print(f"radius {radius}: {far} of {E} edges ({100 * far / E:.0f} %) have 5 <= d < {radius}")
    else:
        assert E >= 50 and bool((d < radius).all()), E                   # envelope narrower than the RBF
        print(f"radius {radius}: {E} edges, none with d >= {radius}")
    return b


def _reference_graph(pos, cell, radius, cap):
    """The reference's radius_graph_pbc on one crystal; asserts that the host builder restates it bit for bit."""
    data = type("D", (), {})()
    data.pos, data.cell, data.natoms = pos, cell.view(1, 3, 3), torch.tensor([pos.shape[0]])
    data.pbc = torch.tensor([[True, True, True]])
    ei, _, _, vec = ref_dutils.radius_graph_pbc(data, radius, cap)
    dist = torch.norm(vec, p=2, dim=-1)                     # dataset/figshare_dataset.py:67
    dirn = torch.nn.functional.normalize(vec, p=2, dim=-1)  # dataset/figshare_dataset.py:68
    mine_ei, mine_dist, mine_dir = radius_graph_pbc_single(pos, cell, radius, max_neighbors=cap)
    assert torch.equal(ei, mine_ei), "edge_index differs from the reference"
    assert torch.equal(dist, mine_dist) and torch.equal(dirn, mine_dir), "edge geometry differs"
    return ei, dist, dirn


def radius_graph_radii_fixture():
    arrays = {"radii": np.array([3.7, 6.0])}
    for name, seed in (("hexagonal", 41), ("triclinic", 42)):
        pos, cell = gu.crystal(name, 12, seed)
        arrays[f"{name}_pos"], arrays[f"{name}_cell"] = to_np(pos), to_np(cell)
        for r in (3.7, 6.0):
            full = _reference_graph(pos, cell, r, None)
            cap = _reference_graph(pos, cell, r, 8)
            assert cap[0].shape[1] < full[0].shape[1]
            for tag, (ei, dist, dirn) in (("", full), ("cap8_", cap)):
                key = f"{name}_r{r}_{tag}"
                arrays[key + "edge_index"], arrays[key + "dist"], arrays[key + "dir"] = to_np(ei), to_np(dist), to_np(dirn)
            print(f"radius_graph_radii[{name}, {r}]: E={full[0].shape[1]}, cap 8 -> {cap[0].shape[1]}, identical to reference")
    for i, (r, y) in enumerate(gu.THRESHOLD_PAIRS):
        pos, cell = gu.threshold_pair(y)
        d2 = (pos[1] ** 2).sum().numpy()                   # fp32: 9 + y^2, the sum the reference forms for this pair
        assert d2 == np.float32(r) * np.float32(r) and d2 > np.float32(r * r), (r, d2)
        up = float(np.nextafter(np.float32(r), np.float32(10)))
        at, above = _reference_graph(pos, cell, r, None), _reference_graph(pos, cell, up, None)
        assert at[0].shape[1] == 0 and above[0].shape[1] == 2
        arrays[f"pair{i}_pos"], arrays[f"pair{i}_cell"] = to_np(pos), to_np(cell)
        arrays[f"pair{i}_radius"], arrays[f"pair{i}_radius_up"] = np.float64(r), np.float64(up)
        arrays[f"pair{i}_edge_index"] = to_np(at[0])
        arrays[f"pair{i}_up_edge_index"], arrays[f"pair{i}_up_dist"], arrays[f"pair{i}_up_dir"] = (to_np(t) for t in above)
        print(f"radius_graph_radii[pair {i}]: d2 = {d2!r}: 0 edges at {r}, 2 at {up!r}, identical to reference")
    np.savez_compressed(os.path.join(HERE, "radius_graph_radii.npz"), **arrays)


def radius_graph_fixture():
    arrays = {}
    for i, (g, n) in enumerate([(200, 12), (201, 25), (202, 40)]):
        d = make_crystal(g, n)
        data = type("D", (), {})()
        data.pos, data.cell, data.natoms = d.pos, d.cell, torch.tensor([n])
        data.pbc = torch.tensor([[True, True, True]])
        ei, _, _, vec = ref_dutils.radius_graph_pbc(data, 5.0, None)
        dist = torch.norm(vec, p=2, dim=-1)                     # dataset/figshare_dataset.py:67
        dirn = torch.nn.functional.normalize(vec, p=2, dim=-1)  # dataset/figshare_dataset.py:68
        mine_ei, mine_dist, mine_dir = radius_graph_pbc_single(d.pos, d.cell[0], 5.0)
        assert torch.equal(ei, mine_ei), "edge_index differs from the reference"
        assert torch.equal(dist, mine_dist) and torch.equal(dirn, mine_dir), "edge geometry differs"
        assert bool((ei[1][1:] >= ei[1][:-1]).all()), "reference edge_index[1] is expected to be sorted"
        arrays[f"pos{i}"], arrays[f"cell{i}"] = to_np(d.pos), to_np(d.cell[0])
        arrays[f"edge_index{i}"], arrays[f"dist{i}"], arrays[f"dir{i}"] = to_np(ei), to_np(dist), to_np(dirn)
        print(f"radius_graph[{i}]: n={n} E={ei.shape[1]} identical to reference")
        # neighbour cap as figshare_dataset.py:65 passes it for iComformer (main.py:141 uses 25; these sparse synthetic
        # crystals have ~14 neighbours per atom, so 8 is what actually drops edges here)
        ei_c, _, _, vec_c = ref_dutils.radius_graph_pbc(data, 5.0, 8)
        mine_ei, mine_dist, mine_dir = radius_graph_pbc_single(d.pos, d.cell[0], 5.0, max_neighbors=8)
        assert torch.equal(ei_c, mine_ei), "capped edge_index differs from the reference"
        assert torch.equal(torch.norm(vec_c, p=2, dim=-1), mine_dist)
        assert ei_c.shape[1] < ei.shape[1]
        arrays[f"cap8_edge_index{i}"], arrays[f"cap8_dist{i}"] = to_np(ei_c), to_np(mine_dist)
        arrays[f"cap8_dir{i}"] = to_np(mine_dir)
        print(f"radius_graph[{i}]: cap 8 -> E={ei_c.shape[1]} identical to reference")
    # degenerate shells: simple cubic, one atom, a = 2.5 -> 6 + 12 + 8 + 6 neighbours inside 5 A; the tolerance keeps
    # whole shells (26 edges for a cap of 25, 18 for a cap of 10)
    data = type("D", (), {})()
    data.pos, data.cell = torch.tensor([[0.3, 0.4, 0.5]]), (2.5 * torch.eye(3)).view(1, 3, 3)
    data.natoms, data.pbc = torch.tensor([1]), torch.tensor([[True, True, True]])
    arrays["cubic_pos"], arrays["cubic_cell"] = to_np(data.pos), to_np(data.cell[0])
    for k in (10, 25):
        ei_c, _, _, vec_c = ref_dutils.radius_graph_pbc(data, 5.0, k)
        mine_ei, mine_dist, mine_dir = radius_graph_pbc_single(data.pos, data.cell[0], 5.0, max_neighbors=k)
        assert torch.equal(ei_c, mine_ei) and torch.equal(torch.norm(vec_c, p=2, dim=-1), mine_dist)
        arrays[f"cubic_cap{k}_edge_index"], arrays[f"cubic_cap{k}_dist"] = to_np(ei_c), to_np(mine_dist)
        arrays[f"cubic_cap{k}_dir"] = to_np(mine_dir)
        print(f"radius_graph[cubic]: cap {k} -> E={ei_c.shape[1]} identical to reference")
    np.savez_compressed(os.path.join(HERE, "radius_graph.npz"), **arrays)


def random_adp(m, seed, spread):
    """[m,3,3] fp32 SPD matrices in the range of real ADPs (eigenvalues ~0.005..0.1 A^2) and a perturbed copy."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, 3, 3, generator=g, dtype=torch.float64)
    q, _ = torch.linalg.qr(a)
    ev = 0.005 + 0.1 * torch.rand(m, 3, generator=g, dtype=torch.float64) ** 2
    true = q @ torch.diag_embed(ev) @ q.transpose(1, 2)
    b = torch.randn(m, 3, 3, generator=g, dtype=torch.float64) * spread
    l = torch.linalg.cholesky(true) @ (torch.eye(3, dtype=torch.float64) + torch.tril(b))
    pred = l @ l.transpose(1, 2)
    sym = lambda x: (0.5 * (x + x.transpose(1, 2))).float()
    return sym(pred), sym(true)


def metrics_fixture():
    """train/metrics.py run as is (its only third-party import is the GraphGym cfg stand-in)."""
    import importlib
    ref_metrics = importlib.import_module("train.metrics")
    from oracle import metrics_ref as om
    arrays = {}
    for name, m, seed, spread in (("close", 48, 31, 0.05), ("far", 48, 32, 0.6)):
        pred, true = random_adp(m, seed, spread)
        vol = ref_metrics.get_error_volume(pred, true)
        sim = ref_metrics.get_similarity_index(pred, true)
        iou = ref_metrics.compute_3D_IoU(pred, true)
        vol64 = ref_metrics.get_error_volume(pred.double(), true.double())
        sim64 = ref_metrics.get_similarity_index(pred.double(), true.double())
        assert torch.allclose(om.get_error_volume(pred, true), vol, rtol=1e-5, atol=1e-7)
        assert torch.allclose(om.get_similarity_index(pred, true), sim, rtol=1e-4, atol=1e-3)
        assert torch.allclose(om.compute_3d_iou(pred, true), iou, rtol=0, atol=1e-4)
        arrays.update({f"{name}_pred": to_np(pred), f"{name}_true": to_np(true), f"{name}_volume_error": to_np(vol),
                       f"{name}_similarity_index": to_np(sim), f"{name}_iou": to_np(iou),
                       f"{name}_volume_error64": to_np(vol64), f"{name}_similarity_index64": to_np(sim64)})
        print(f"adp_metrics[{name}]: vol {vol.mean():.4f} S12 {sim.mean():.4f} IoU {iou.mean():.4f} | fp32-vs-fp64 "
              f"vol {(vol - vol64).abs().max():.2e} S12 {(sim - sim64).abs().max():.2e}")
    np.savez_compressed(os.path.join(HERE, "adp_metrics.npz"), **arrays)


def train_epoch_fixture():
    """the reference's training loop, run as is on the tiny model.  What the loop decides -- unscaled
    accumulation (train/train.py:183), the boundary rule with its last-iteration flush (:186), Adam (main.py:208), the
    OneCycleLR total-steps formula (:59), scheduler.step() per optimiser step (:188) -- lands in the stored numbers."""
    import types
    from _ref_import import import_reference_train
    cfg, ref_train = import_reference_train()
    hp = hp_dict(16, 8, 2)
    cfg.invariant, cfg.radius = hp["invariant"], hp["radius"]
    cfg.loss = "MAE"
    cfg.dataset = types.SimpleNamespace(name="ADP")
    cfg.params_count = 0
    EPOCHS, ACCUM, LR, WARMUP = 2, 3, 1e-3, 0.4
    sd = make_state_dict(16, 8, 2, seed=51)

    class HostBatch(Batch):
        def to(self, *a, **k):            # `batch.to("cuda:0")` (train/train.py:169): a device move, no arithmetic; no GPU here
            return self
    sizes = [(5, 7), (6, 9), (8, 5), (7, 6), (9, 8)]           # five micro-batches of two crystals each
    micro = [HostBatch.from_data_list([make_crystal(700 + 10 * i, a), make_crystal(701 + 10 * i, b)])
             for i, (a, b) in enumerate(sizes)]

    class Loader:                         # torch_geometric.loader.DataLoader stand-in: fresh batches every epoch, fixed order
        def __len__(self):
            return len(micro)

        def __iter__(self):
            for b in micro:
                c = b.clone()
                c.num_graphs = b.num_graphs
                yield c

    torch.manual_seed(0)
    m = ref_cartnet.CartNet(dim_in=16, dim_rbf=8, num_layers=2)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    names = [k for k, _ in m.named_parameters()]
    opt = torch.optim.Adam(m.parameters(), lr=LR)                                  # main.py:208
    loader = Loader()
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=EPOCHS * len(loader) // ACCUM + EPOCHS,
                                                pct_start=WARMUP)                   # train/train.py:59
    flat = lambda ts: np.concatenate([to_np(t).ravel() for t in ts])
    steps = []
    opt.register_step_pre_hook(lambda o, a, k: steps.append({"grad": flat([p.grad for p in m.parameters()])}))
    opt.register_step_post_hook(lambda o, a, k: steps[-1].update(param=flat(list(m.parameters()))))

    class Logger:                         # GraphGym Logger stand-in: keeps what compute_metrics_and_logging hands over
        def __init__(self):
            self.rows = []

        def update_stats(self, **kw):
            self.rows.append((float(kw["loss"]), float(kw["MAE"]), float(kw["MSE"]), float(kw["lr"])))
    logger = Logger()
    arrays = {}
    for ep in range(EPOCHS):
        ref_train.train_epoch(logger, loader, m, opt, ACCUM, sched)
        for k, v in m.state_dict().items():
            if "running" in k or "num_batches" in k:
                arrays[f"state_ep{ep}_{k}"] = to_np(v).copy()      # (a view of the live buffer otherwise)
    assert len(steps) == 4 and len(logger.rows) == EPOCHS * len(micro)
    # the learning rate AFTER the scheduler step that follows optimiser step k is what iteration k's row logged (:195)
    rows = np.array(logger.rows, dtype=np.float64)
    arrays["iter_loss"], arrays["iter_mae"], arrays["iter_mse"], arrays["iter_lr"] = rows.T
    for k, st in enumerate(steps):
        arrays[f"step{k}_grad"], arrays[f"step{k}_param"] = st["grad"], st["param"]
    arrays["param_names"] = np.array(names)
    arrays["param_sizes"] = np.array([p.numel() for p in m.parameters()], dtype=np.int64)
    for k, v in hp.items():
        arrays["hp_" + k] = np.array(v)
    arrays["epochs"], arrays["accum"], arrays["lr"], arrays["warmup"] = (np.int64(EPOCHS), np.int64(ACCUM),
                                                                         np.float64(LR), np.float64(WARMUP))
    for k, v in sd.items():
        arrays["w_" + k] = to_np(v)
    for i, b in enumerate(micro):
        for k, v in batch_inputs(b).items():
            arrays[f"b{i}_{k}"] = v
    path = os.path.join(HERE, "train_epoch.npz")
    np.savez_compressed(path, **arrays)
    print(f"train_epoch: {len(steps)} optimiser steps over {len(logger.rows)} iterations, lr per iteration "
          f"{[f'{x:.3e}' for x in rows[:, 3]]} -> {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    """All fixtures, or only those named on the command line (``python tests/golden/make_golden.py tiny_nothing``)."""
    torch.set_num_threads(4)
    b1 = lambda: Batch.from_data_list([make_crystal(300 + g, None, n_range=(30, 70)) for g in range(4)])
    b5 = lambda: Batch.from_data_list([make_crystal(500 + g, None, n_range=(20, 40)) for g in range(3)])
    b2 = lambda: Batch.from_data_list([make_crystal(400 + g, 194) for g in range(2)])
    jobs = {
        "radius_graph": radius_graph_fixture,
        "radius_graph_radii": radius_graph_radii_fixture,
        "adp_metrics": metrics_fixture,
        "train_epoch": train_epoch_fixture,
        "tiny_adp": lambda: save_model_fixture("tiny_adp", hp_dict(16, 8, 2), tiny_batch(), seed=11,
                                               store_weights=True, full_grads=True, trace=True),
        "tiny_scalar": lambda: save_model_fixture("tiny_scalar", hp_dict(16, 8, 2, temperature=False, cholesky=False),
                                                  tiny_batch(adp=False), seed=12, store_weights=True, full_grads=True,
                                                  trace=False),
        "tiny_invariant": lambda: save_model_fixture("tiny_invariant",
                                                     hp_dict(16, 8, 2, invariant=True, use_envelope=False),
                                                     tiny_batch(), seed=13, store_weights=True, full_grads=True,
                                                     trace=False),
        "tiny_noatom": lambda: save_model_fixture("tiny_noatom", hp_dict(16, 8, 2, atom_types=False), tiny_batch(),
                                                  seed=14, store_weights=True, full_grads=True, trace=False),
        # scripts/run_no_atom_type.sh:16-27 ("CartNet_nothing"): --disable_atom_types --disable_temp, i.e. the fourth
        # Encoder branch (models/cartnet.py:115-116,150-151): one learned row for every atom, no atom MLP
        "tiny_nothing": lambda: save_model_fixture("tiny_nothing",
                                                   hp_dict(16, 8, 2, atom_types=False, temperature=False),
                                                   tiny_batch(), seed=15, store_weights=True, full_grads=True,
                                                   trace=True),
        # main.py --radius 6 / 4: models/master.py never hands the flag to CartNet, so the RBF cutoff stays 5.0 while
        # the graph and the envelopes follow cfg.radius
        "tiny_radius6": lambda: save_model_fixture("tiny_radius6", hp_dict(16, 8, 2, env_radius=6.0), radius_batch(6.0),
                                                   seed=16, store_weights=True, full_grads=True, trace=True),
        "tiny_radius4": lambda: save_model_fixture("tiny_radius4", hp_dict(16, 8, 2, env_radius=4.0), radius_batch(4.0),
                                                   seed=17, store_weights=True, full_grads=True, trace=True),
        "config1": lambda: save_model_fixture("config1", hp_dict(64, 64, 2), b1(), seed=21, store_weights=False,
                                              full_grads=True, trace=False),
        "icomformer_tiny": lambda: icomformer_fixture("icomformer_tiny", 16, tiny_batch(), seed=31,
                                                      store_weights=True),
        "icomformer_c32": lambda: icomformer_fixture("icomformer_c32", 32, b5(), seed=32, store_weights=False),
        "config2": lambda: save_model_fixture("config2", hp_dict(256, 64, 4), b2(), seed=22, store_weights=False,
                                              full_grads=False, trace=False),
    }
    only = sys.argv[1:]
    for name in only:
        if name not in jobs:
            raise SystemExit(f"unknown fixture {name!r}; known: {', '.join(jobs)}")
    for name, job in jobs.items():
        if not only or name in only:
            job()


if __name__ == "__main__":
    main()
