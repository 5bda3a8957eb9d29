"""The bytes of the prediction pass: ``predict.predict_adps`` with ``pass_statistics`` and ``evaluate.inference`` on a
fixed set of small inputs, as sha256 digests.  The pass promises "the same call gives the same bytes", so the digests of
one commit are an oracle for the next: ``tests/golden/predict_bytes.json`` holds those of the commit before the pass was
restated over one record of options, one table of key groups and one stage, and tests/test_gpu_predict_bytes.py holds
every later one to them, case by case.

Only the public API is used (``predict_adps``, ``pass_statistics``, ``entry``, ``load_input``, ``evaluate.inference``,
``main.shard_recipe``), so this file runs on either side of such a change.  The model is a fresh CartNet
``--dim_in 64 --num_layers 2`` after ``torch.manual_seed(0)``, the loaders hold two crystals per batch.  A prediction
case records the ordered keys of the result, one digest over dtype, shape and bytes of every tensor of every entry
(anything else by its ``repr``) and the digest of ``json.dumps(pass_statistics(...))`` without key sorting; an inference
case the pickle's ordered keys, a digest per crystal and the digest of the result without ``output``.

usage: python tools/predict_bytes.py [--out tests/golden/predict_bytes.json]"""
import argparse
import hashlib
import json
import os
import pickle
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

MODEL = ["--dim_in", "64", "--num_layers", "2"]
EVAL_BATCH = 2
ALL = dict(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
           aniso_h=(0.005, 0.020))
# case -> (input, the keywords of predict_adps).  "three": the crystals mixed, polymer and face of
# tests/test_gpu_main_aniso_h.py (49, 16 and 14 atoms: every hydrogen source, a periodic molecule, bonds through a cell
# face) as a shard file; "cif": the P-1 methanol of tests/test_gpu_main_riding_h.py as a CIF file, so ``sym`` is set
PREDICT = {"a_plain": ("three", {}),
           "b_rotations": ("three", dict(rotations=3)),
           "c_analyses": ("three", ALL),
           "d_analyses_series_frames": ("three", dict(ALL, temperatures=(100.0, 180.5, 300.0), rotations=2)),
           "e_one_temperature": ("three", dict(temperatures=(150.0,))),
           "f_aniso_without_molecules": ("three", dict(riding_h=ALL["riding_h"], aniso_h=ALL["aniso_h"])),
           "g_cif_analyses": ("cif", ALL),
           "h_cif_riding_series": ("cif", dict(riding_h=ALL["riding_h"], temperatures=(100.0, 200.0)))}
# case -> the keywords of evaluate.inference, on tests/predict_utils.six_crystals(labeled=True)
INFERENCE = {"i_inference": {},
             "j_inference_analyses": dict(rotations=2, rigid_bond=(0.4, 1e-3), rigid_molecule=(0.4, 1e-3), tls_fit=True)}


def _update(h, value) -> None:
    """Feeds ``value`` to the hash ``h``: a tensor as dtype, shape and bytes, a dict or list by its members in order,
    anything else by its ``repr``."""
    import torch
    if torch.is_tensor(value):
        a = value.detach().cpu().contiguous().numpy()
        h.update(f"{a.dtype} {a.shape} ".encode() + a.tobytes())
    elif isinstance(value, dict):
        for k, v in value.items():
            h.update(f"<{k}>".encode())
            _update(h, v)
    elif isinstance(value, (list, tuple)):
        h.update(f"[{len(value)}]".encode())
        for v in value:
            _update(h, v)
    else:
        h.update(repr(value).encode())


def digest(value) -> str:
    h = hashlib.sha256()
    _update(h, value)
    return h.hexdigest()


def _methanol_cif(path: str) -> None:
    import numpy as np

    import cif_utils as cu
    from test_gpu_main_riding_h import METHANOL
    cell = (8.1, 8.6, 9.2, 85.0, 95.0, 100.0)
    inv = np.linalg.inv(cu.cell_reference(*cell))
    atoms, symbol = [], {1: "H", 6: "C", 8: "O"}
    for k, (z, pos, _, _) in enumerate(METHANOL):
        f = (np.array(pos) + np.array([2.0, 2.4, 1.9])) @ inv
        atoms.append((f"{symbol[z]}{k + 1}", symbol[z], float(f[0]), float(f[1]), float(f[2]),
                      None if z == 1 else (0.03, 0.03, 0.03, 0.0, 0.0, 0.0)))
    had = cu.CRYSTALS.get("ride")
    cu.CRYSTALS["ride"] = dict(cell=cell, ops=cu.close_group([cu.INVERSION]), temp=120.0, atoms=atoms)
    try:
        with open(path, "w") as f:
            f.write(cu.cif_text("ride", name="ride", labeled=False))
    finally:
        if had is None:
            del cu.CRYSTALS["ride"]
        else:
            cu.CRYSTALS["ride"] = had


def run() -> dict:
    """name of the case -> what the module docstring says it records."""
    import torch

    import main as entry
    import predict_utils as pu
    from cartnet_amd import evaluate, predict as pr, shard
    from cartnet_amd.config import cfg, set_cfg
    from cartnet_amd.master import create_model
    from test_gpu_main_aniso_h import NAMES, _crystals
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    out = {}
    try:
        torch.manual_seed(0)
        model = create_model()
        with tempfile.TemporaryDirectory() as d:
            paths = {"three": os.path.join(d, "three.cnshard"), "cif": os.path.join(d, "ride.cif")}
            shard.write_shard(paths["three"], _crystals(), names=list(NAMES))
            _methanol_cif(paths["cif"])
            for name, (source, kw) in PREDICT.items():
                src, sym, rejected = pr.load_input(paths[source], cfg.device)
                (s,), (mean, std) = entry.shard_recipe([src])
                res = pr.predict_adps(model, shard.ShardLoader(s, EVAL_BATCH, temp_mean=mean, temp_std=std), cfg.device,
                                      sym=sym, **kw)
                temps = list(kw["temperatures"]) if "temperatures" in kw else None
                line = pr.pass_statistics(res, None, None, rejected, kw.get("rotations", 1), temps)
                whole = {k: v for k, v in res.items() if k != "series"}
                assert all(pr.entry(res, i).keys() == whole.keys() for i in range(len(res["name"])))
                out[name] = {"keys": list(res), "entries": digest(res), "statistics": digest(json.dumps(line))}
            (s,), (mean, std) = entry.shard_recipe([shard.DeviceShard.from_data_list(pu.six_crystals(labeled=True), cfg.device)])
            for name, kw in INFERENCE.items():
                path = os.path.join(d, name + ".pkl")
                res = evaluate.inference(model, shard.ShardLoader(s, EVAL_BATCH, temp_mean=mean, temp_std=std), cfg.device,
                                         path, **kw)
                with open(path, "rb") as f:
                    pickled = pickle.load(f)
                crystals = len(pickled["pred"])
                out[name] = {"keys": list(pickled),
                             "entries": [digest({k: v[i] for k, v in pickled.items() if len(v) == crystals})
                                         for i in range(crystals)],
                             "result": digest(json.dumps({k: v for k, v in res.items() if k != "output"}))}
    finally:
        set_cfg()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    text = json.dumps(run(), indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
