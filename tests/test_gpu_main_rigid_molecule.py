"""``main.py --rigid_molecule`` end to end on four hand-built molecular crystals with a small CartNet whose checkpoint the
test saves: ``--predict`` carries the molecules and the pair test of a direct ``metrics.molecules`` /
``metrics.molecule_test`` call per crystal, bit for bit, beside everything it carried before; the flag composes with
``--rigid_bond``, ``--rotations``, ``--predict_temperatures`` and CIF input; ``--inference`` tests prediction and truth on
molecules found once; without the flag nothing changes."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import cif_utils as cu
import molecule_utils as mu
import predict_utils as pu

pytestmark = pytest.mark.gpu

MODEL = ["--dim_in", "64", "--num_layers", "2"]
PREDICT_JSON = {"crystals", "rows", "u_eq_mean", "non_positive_rows", "output", "cif_dir"}
MOL_JSON = {"molecules", "molecules_tested", "molecules_periodic", "molecules_open", "molecule_atoms_max",
            "rigid_molecule_pairs", "rigid_molecule_mean", "rigid_molecule_max", "rigid_molecule_over"}
INFERENCE_JSON = {"iou_mean", "iou_std", "mae_mean", "mae_std", "similarity_index_mean", "similarity_index_std", "output"}
INFERENCE_PICKLE = {"pred", "true", "temp", "cell", "refcode", "pos", "atoms", "iou", "mae", "similarity_index"}
MOL_DTYPES = {"mol": torch.int32, "mol_size": torch.int32, "mol_status": torch.int32, "mol_pos": torch.float32,
              "mol_pairs": torch.int32, "mol_delta_mean": torch.float32, "mol_delta_max": torch.float32,
              "mol_worst": torch.int64, "mol_over": torch.int32, "mol_stats": torch.float64}
METHANOL = ((1, (-0.36, 1.03, 0.0)), (6, (0.0, 0.0, 0.0)), (1, (-0.36, -0.51, 0.89)), (8, (1.43, 0.0, 0.0)),
            (1, (-0.36, -0.51, -0.89)), (1, (1.75, 0.90, 0.0)))
NAMES = ("methanols", "chain", "polymer", "mixed")
# per crystal: (molecules, tested, periodic, open, largest size)
COUNTS = ([2.0, 2.0, 0.0, 0.0, 2.0], [1.0, 1.0, 0.0, 0.0, 6.0], [1.0, 0.0, 1.0, 0.0, 8.0], [3.0, 1.0, 0.0, 0.0, 6.0])


def _crystals(labeled: bool):
    """Two methanol molecules with their hydrogens; a chain of six carbons through a cell face; the polymer; a ring, a
    lone oxygen and a lone iodine.  Labeled: with ``y`` and ``non_H_mask``."""
    from cartnet_amd.data import Data
    m = np.array([a[1] for a in METHANOL])
    zm = [a[0] for a in METHANOL]
    made = [(np.concatenate([m + [2.1, 2.7, 2.3], m + [5.2, 6.1, 5.9]]), mu.cubic(9.0), np.array(zm + zm)),
            (mu.chain(6, (6.0, 3.0, 3.0), mu.cubic(9.0))[0], mu.cubic(9.0), np.full(6, 6)),
            mu.polymer(8),
            (np.concatenate([mu.ring([4.0, 4.0, 4.0]), [[8.0, 8.0, 8.0]], [[1.0, 8.5, 2.0]]]), mu.cubic(11.0),
             np.array([6] * 6 + [8, 53]))]
    out = []
    for g, (pos, cell, z) in enumerate(made):
        d = Data(x=torch.tensor(z, dtype=torch.int64), pos=torch.tensor(pos, dtype=torch.float32),
                 cell=torch.tensor(cell, dtype=torch.float32).unsqueeze(0), natoms=torch.tensor([len(z)]),
                 temperature=torch.tensor([0.25]))
        if labeled:
            d.non_H_mask = d.x != 1
            d.y = pu.spd_rows(int(d.non_H_mask.sum()), 200 + g)
        out.append(d)
    return out


ROWS = (4, 6, 8, 8)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard of the four crystals)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("rigid_molecule")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "four.cnshard")
    shard.write_shard(src, _crystals(False), names=list(NAMES))
    yield d, ckpt, src
    set_cfg()


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _same(p, q) -> bool:
    if torch.is_tensor(p):
        return p.dtype == q.dtype and p.shape == q.shape and p.numpy().tobytes() == q.numpy().tobytes()
    return p == q or (p != p and q != q)


def _graphed(path):
    """The shard of ``path`` as main.py's recipe leaves it (cfg is the one of the run before)."""
    import main as entry
    from cartnet_amd.shard import DeviceShard
    (s,), _ = entry.shard_recipe([DeviceShard.from_file(path, "cuda:0")])
    return s


def _check_entries(out, res, n_entries):
    """What holds for every entry of a flag-on result: shapes and dtypes, ``mol_stats`` against the row keys, the JSON
    line against the sums over the entries."""
    assert all(len(out[k]) == n_entries for k in MOL_DTYPES)
    for k in range(n_entries):
        n = int(out["u_cart"][k].shape[0])
        for key, dtype in MOL_DTYPES.items():
            t = out[key][k]
            assert t.dtype == dtype and tuple(t.shape) == {"mol_pos": (n, 3), "mol_stats": (9,)}.get(key, (n,)), (key, k)
        stats, size, status = out["mol_stats"][k], out["mol_size"][k], out["mol_status"][k]
        first = torch.tensor([bool((out["mol"][k][:i] != out["mol"][k][i]).all()) for i in range(n)], dtype=torch.bool)
        tested = (status == 0) & (size >= 2)
        assert stats[0] == first.sum() == (int(out["mol"][k].max()) + 1 if n else 0)
        assert stats[1] == (first & tested).sum() and stats[2] == (first & (status & 1 > 0)).sum()
        assert stats[3] == (first & (status & 2 > 0)).sum() and stats[4] == (int(size.max()) if n else 0)
        assert torch.equal(out["mol_pairs"][k], torch.where(tested, size - 1, torch.zeros_like(size)))
        assert stats[5] == out["mol_pairs"][k].sum() and stats[8] == out["mol_over"][k].sum()
        assert stats[7] == out["mol_delta_max"][k].double().max()
        total = (out["mol_delta_mean"][k].double() * out["mol_pairs"][k]).sum()
        assert abs(float(stats[6] - total)) <= 1e-6 * float(total) + 1e-30            # the mean is rounded to fp32 once
        assert bool((torch.isnan(out["mol_pos"][k]).all(1) == (status != 0)).all())
        assert bool(((out["mol_worst"][k] >= 0) == tested).all()) and int(out["mol_worst"][k].max()) < len(out["z"][k])
    ms = torch.stack(out["mol_stats"])
    assert [res[k] for k in ("molecules", "molecules_tested", "molecules_periodic", "molecules_open")] == \
        [int(ms[:, c].sum()) for c in range(4)]
    assert res["molecule_atoms_max"] == int(ms[:, 4].max()) and res["rigid_molecule_pairs"] == int(ms[:, 5].sum()) > 0
    assert res["rigid_molecule_over"] == int(ms[:, 8].sum()) and res["rigid_molecule_max"] == float(ms[:, 7].max())
    assert res["rigid_molecule_mean"] == pytest.approx(float(ms[:, 6].sum()) / res["rigid_molecule_pairs"], rel=1e-12)
    assert 0 < res["rigid_molecule_mean"] <= res["rigid_molecule_max"]


def test_predict_carries_the_direct_result_and_changes_nothing_else(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd.metrics import molecule_test, molecules, target_row_ptr
    from cartnet_amd.predict import KEYS, MOL_KEYS
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "3"] + MODEL
    plain = entry.main(common + ["--predict_output", "plain.pkl", "--rigid_molecule_threshold", "5e-4"])
    capsys.readouterr()
    res = entry.main(common + ["--predict_output", "mol.pkl", "--rigid_molecule"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    old, out = _load("plain.pkl"), _load("mol.pkl")
    assert set(plain) == PREDICT_JSON and tuple(old) == KEYS                  # without the flag: as it always was
    assert set(res) == PREDICT_JSON | MOL_JSON and list(out) == list(KEYS) + list(MOL_KEYS)
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    for k in old:                                                             # every old key: the same bits
        assert len(old[k]) == len(out[k]) == 4 and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 4)
    assert [t.tolist() for t in out["mol_stats"]] == [c + t.tolist()[5:] for c, t in zip(COUNTS, out["mol_stats"])]
    assert [int(t.shape[0]) for t in out["mol"]] == list(ROWS)
    s = _graphed(src)
    for k in range(4):                                                        # crystal k alone: its own batch, its own graph
        b = s.collate([k])
        rp = target_row_ptr(b)
        mo = molecules(b, rp, 0.4, rows=ROWS[k])
        mt = molecule_test(out["u_cart"][k].cuda(), b, rp, mo, 1e-3)
        pos = mo.x[b.non_H_mask].float().cpu()
        want = {"mol": mo.mol, "mol_size": mo.size, "mol_status": mo.status, "mol_pairs": mt.pairs,
                "mol_delta_max": mt.delta_max, "mol_worst": mt.worst, "mol_over": mt.over,
                "mol_stats": torch.cat([mo.crystal_counts[0], mt.crystal_stats[0]]),
                "mol_delta_mean": mt.delta_sum / mt.pairs.clamp(min=1).float()}
        for key, t in want.items():
            assert _same(out[key][k], t.cpu()), (key, k)
        ok = (mo.status == 0).cpu()
        assert torch.equal(out["mol_pos"][k][ok], pos[ok]) and bool(torch.isnan(out["mol_pos"][k][~ok]).all())
    # the chain through the face comes out unwrapped: consecutive atoms one zig-zag step apart
    step = out["mol_pos"][1][1:] - out["mol_pos"][1][:-1]
    assert float((step.norm(dim=1) - float(np.hypot(mu.STEP, mu.ZIG))).abs().max()) < 1e-3


@pytest.mark.parametrize("extra", [["--rigid_bond"], ["--rotations", "2"], ["--predict_temperatures", "100,200"]],
                         ids=["rigid_bond", "rotations", "temperatures"])
def test_the_flag_composes(work, monkeypatch, capsys, extra):
    import main as entry
    from cartnet_amd.predict import MOL_KEYS
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "3"] + MODEL + extra
    plain = entry.main(common + ["--predict_output", "c_plain.pkl"])
    res = entry.main(common + ["--predict_output", "c_mol.pkl", "--rigid_molecule"])
    old, out = _load("c_plain.pkl"), _load("c_mol.pkl")
    assert set(res) == set(plain) | MOL_JSON and not set(plain) & MOL_JSON
    assert [k for k in out if k != "series"] == [k for k in old if k != "series"] + list(MOL_KEYS)
    for k in old:
        if k != "series":
            assert len(old[k]) == len(out[k]) and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    T = 2 if extra[0] == "--predict_temperatures" else 1
    _check_entries(out, res, 4 * T)
    assert [t.tolist()[:5] for t in out["mol_stats"]] == [c for c in COUNTS for _ in range(T)]
    if T == 2:                                                                # molecules do not depend on U
        assert {k: [_same(p, q) for p, q in zip(old["series"][k], out["series"][k])] for k in old["series"]} == \
            {k: [True] * 4 for k in old["series"]}
        for g in range(4):
            for key in ("mol", "mol_size", "mol_status", "mol_pos"):
                assert _same(out[key][2 * g], out[key][2 * g + 1]), (key, g)
        assert any(not _same(out["mol_delta_max"][2 * g], out["mol_delta_max"][2 * g + 1]) for g in range(4))


def test_cif_input_describes_the_rows_of_the_expanded_cell(work, monkeypatch, capsys):
    """P-1 with a methanol molecule as the asymmetric unit: two heavy atoms in the file, four rows in the cell, two
    molecules of two.  The CIF that is written does not change."""
    import main as entry
    from cartnet_amd.predict import KEYS, MOL_KEYS, SYM_KEYS
    d, ckpt, _ = work
    monkeypatch.chdir(d)
    cell = (8.1, 8.6, 9.2, 85.0, 95.0, 100.0)
    inv = np.linalg.inv(cu.cell_reference(*cell))
    atoms, sym = [], {1: "H", 6: "C", 8: "O"}
    for k, (z, pos) in enumerate(METHANOL):
        f = (np.array(pos) + np.array([2.0, 2.4, 1.9])) @ inv
        atoms.append((f"{sym[z]}{k + 1}", sym[z], float(f[0]), float(f[1]), float(f[2]),
                      None if z == 1 else (0.03, 0.03, 0.03, 0.0, 0.0, 0.0)))
    monkeypatch.setitem(cu.CRYSTALS, "mol", dict(cell=cell, ops=cu.close_group([cu.INVERSION]), temp=120.0, atoms=atoms))
    os.makedirs("cif_in", exist_ok=True)
    with open(os.path.join("cif_in", "mol.cif"), "w") as f:
        f.write(cu.cif_text("mol", name="mol", labeled=False))
    common = ["--predict", "--predict_input", "cif_in", "--checkpoint_path", ckpt] + MODEL
    plain = entry.main(common + ["--predict_output", "cif_plain.pkl", "--predict_cif_dir", "cif_plain"])
    res = entry.main(common + ["--predict_output", "cif_mol.pkl", "--predict_cif_dir", "cif_mol", "--rigid_molecule"])
    old, out = _load("cif_plain.pkl"), _load("cif_mol.pkl")
    assert tuple(old) == KEYS + SYM_KEYS and list(out) == list(old) + list(MOL_KEYS)
    assert set(res) == set(plain) | MOL_JSON
    for k in old:
        assert all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 1)
    assert tuple(out["u_cif_asym"][0].shape) == (2, 6) and tuple(out["mol"][0].shape) == (4,)     # sites against rows
    assert out["mol_stats"][0].tolist()[:5] == [2.0, 2.0, 0.0, 0.0, 2.0] and out["mol_size"][0].tolist() == [2] * 4
    assert sorted(out["mol"][0].tolist()) == [0, 0, 1, 1]
    with open(os.path.join("cif_plain", "mol.cif"), "rb") as f, open(os.path.join("cif_mol", "mol.cif"), "rb") as g:
        assert f.read() == g.read()


def test_inference_tests_prediction_and_truth_on_molecules_found_once(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import evaluate, metrics, shard
    d, ckpt, _ = work
    monkeypatch.chdir(d)

    def splits(name, crystals):
        os.makedirs(name, exist_ok=True)
        for part in ("train", "val", "test"):
            shard.write_shard(os.path.join(name, f"{part}.cnshard"), crystals)
        return ["--inference", "--shard_dir", name, "--checkpoint_path", ckpt, "--eval_batch", "3"] + MODEL
    common = splits("splits", _crystals(True))
    plain = entry.main(common + ["--inference_output", "inf_plain.pkl"])
    assert set(plain) == INFERENCE_JSON and set(_load("inf_plain.pkl")) == INFERENCE_PICKLE     # as it always was
    found = []
    find = metrics.molecules
    monkeypatch.setattr(evaluate, "molecules", lambda *a, **k: found.append(1) or find(*a, **k))
    capsys.readouterr()
    res = entry.main(common + ["--inference_output", "inf_mol.pkl", "--rigid_molecule"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    out = _load("inf_mol.pkl")
    assert len(found) == 2                                                    # once per batch, for prediction and truth
    assert line == res and set(res) == INFERENCE_JSON | {
        "molecules", "molecules_tested", "rigid_molecule_pairs", "rigid_molecule_mean", "rigid_molecule_max",
        "rigid_molecule_over", "rigid_molecule_mean_true", "rigid_molecule_max_true", "rigid_molecule_over_true"}
    assert set(out) == INFERENCE_PICKLE | set(evaluate.MOLECULE_KEYS)
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    assert (res["molecules"], res["molecules_tested"]) == (7, 4) and res["rigid_molecule_pairs"] == 2 * 2 + 6 * 5 + 6 * 5
    assert [t.tolist() for t in out["mol_size"]] == [[2] * 4, [6] * 6, [8] * 8, [6] * 6 + [1, 1]]
    for key in ("mol_pairs", "mol_delta_max", "mol_over"):
        assert all(int(t.shape[0]) == n for t, n in zip(out[key], ROWS)) and len(out[key + "_true"]) == 4
    assert all(_same(p, q) for p, q in zip(out["mol_pairs"], out["mol_pairs_true"]))
    assert any(not _same(p, q) for p, q in zip(out["mol_delta_max"], out["mol_delta_max_true"]))
    assert res["rigid_molecule_max"] == max(float(t.max()) for t in out["mol_delta_max"])
    assert res["rigid_molecule_max_true"] == max(float(t.max()) for t in out["mol_delta_max_true"])
    assert res["rigid_molecule_over"] == sum(int(t.sum()) for t in out["mol_over"])
    assert res["rigid_molecule_mean"] > 0 and res["rigid_molecule_mean_true"] > 0
    # the truth made equal to the prediction: the two sets agree bit for bit
    equal = _crystals(True)
    for c, pred in zip(equal, out["pred"]):
        c.y = pred.clone()
    res = entry.main(splits("splits_equal", equal) + ["--inference_output", "inf_equal.pkl", "--rigid_molecule"])
    same = _load("inf_equal.pkl")
    assert all(_same(p, q) for p, q in zip(same["pred"], same["true"]))
    for key in ("mol_pairs", "mol_delta_max", "mol_over"):
        assert all(_same(p, q) for p, q in zip(same[key], same[key + "_true"])), key
        assert all(_same(p, q) for p, q in zip(same[key], out[key])), key
    for key in ("mean", "max", "over"):
        assert res[f"rigid_molecule_{key}"] == res[f"rigid_molecule_{key}_true"]
