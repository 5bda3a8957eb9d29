"""``main.py --predict --angle_table`` end to end on the three crystals of the anisotropic-hydrogen test (molecules with
hydrogens, the polymer, a helix at a cell face) with a small CartNet whose checkpoint the test saves, in batches of two, so
the last batch is short: plain, beside ``--rigid_molecule --tls_fit``, at two temperatures and beside ``--bond_table``.
The ``angles_*`` and ``torsions_*`` entries come last, have one piece per crystal of the sizes their statistics name, hold
atom indices inside the crystal, are what a direct ``metrics.angle_table`` gives for the crystal alone, and the JSON line is
the sum over the pickle; without the flag there is no new key and no new field."""
import json

import pytest
import torch

from test_gpu_main_aniso_h import NAMES, ROWS, _crystals
from test_gpu_main_rigid_molecule import MODEL, _graphed, _load, _same

pytestmark = pytest.mark.gpu

AT_JSON = {"angles_listed", "angle_mean", "angle_libration_angles", "angle_libration_mean", "angle_libration_max"}
TT_JSON = {"torsions_listed", "torsions_undefined", "torsion_libration_torsions", "torsion_libration_mean",
           "torsion_libration_max"}
DTYPES = {"a": torch.int64, "b": torch.int64, "c": torch.int64, "d": torch.int64, "value": torch.float32,
          "libration": torch.float32, "tls_rank": torch.int32, "stats": torch.float64}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard of the three crystals)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("angle_table")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "three.cnshard")
    shard.write_shard(src, _crystals(), names=list(NAMES))
    yield d, ckpt, src
    set_cfg()


def _run(work, monkeypatch, capsys, name, *flags):
    """One ``main.py --predict`` pass with ``flags``: ``(result, pickle)``, the result checked against the printed line."""
    import main as entry
    d, ckpt, src = work
    monkeypatch.chdir(d)
    res = entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2",
                      "--predict_output", name, *flags] + MODEL)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    return res, _load(name)


def _check_entries(out, res, n_entries, tls):
    """What holds for every entry of a flag-on result, and the JSON line against the sums over the pickle."""
    from cartnet_amd.predict import AT_KEYS, TT_KEYS
    T = n_entries // len(NAMES)
    for k in range(n_entries):
        z = out["z"][k]
        n, row = int(z.shape[0]), torch.cumsum((z != 1).to(torch.int64), 0) - 1
        for prefix, keys, centre in (("angles", AT_KEYS, "b"), ("torsions", TT_KEYS, "c")):
            st = out[f"{prefix}_stats"][k]
            m = int(st[0])
            for key in keys:
                t = out[key][k]
                assert t.dtype == DTYPES[key.split("_", 1)[1]] and tuple(t.shape) == ((5,) if key.endswith("stats") else (m,)), (key, k)
            for key in keys[:4 if prefix == "torsions" else 3]:
                assert bool(((0 <= out[key][k]) & (out[key][k] < n)).all()) and bool((z[out[key][k]] != 1).all()), (key, k)
            value, lib = out[f"{prefix}_value"][k].double(), out[f"{prefix}_libration"][k].double()
            fin = torch.isfinite(lib)
            x = (lib - value).abs()[fin]
            if prefix == "torsions":
                x = torch.minimum(x, 360.0 - x)
                assert st[1] == int(torch.isnan(value).sum())
                assert bool((out["torsions_b"][k] < out["torsions_c"][k]).all())
            else:
                assert float(st[1]) == pytest.approx(float(value.sum()), rel=1e-12) and bool((value > 0).all())
            assert st[2] == int(fin.sum()) and float(st[3]) == pytest.approx(float(x.sum()), rel=1e-12, abs=1e-300)
            assert float(st[4]) == (float(x.max()) if bool(fin.any()) else 0.0)
            rank = out[f"{prefix}_tls_rank"][k]
            if tls:                                                           # finite exactly on the fitted molecules
                assert bool((rank == out["tls_rank"][k][row[out[f"{prefix}_{centre}"][k]]]).all()), (prefix, k)
                assert bool((fin == ((rank > 0) & ~torch.isnan(value))).all()), (prefix, k)
            else:
                assert not bool(fin.any()) and not bool(rank.any())
    sa, st = torch.stack(out["angles_stats"]), torch.stack(out["torsions_stats"])
    assert res["angles_listed"] == int(sa[:, 0].sum()) > 0 and res["torsions_listed"] == int(st[:, 0].sum()) > 0
    assert res["angle_mean"] == pytest.approx(float(sa[:, 1].sum()) / res["angles_listed"], rel=1e-12)
    assert res["torsions_undefined"] == int(st[:, 1].sum())
    assert res["angle_libration_angles"] == int(sa[:, 2].sum()) and res["torsion_libration_torsions"] == int(st[:, 2].sum())
    if tls:
        assert res["angle_libration_angles"] > 0 and res["torsion_libration_torsions"] > 0
        assert res["angle_libration_mean"] == pytest.approx(float(sa[:, 3].sum()) / res["angle_libration_angles"], rel=1e-12)
        assert res["torsion_libration_mean"] == pytest.approx(float(st[:, 3].sum()) / res["torsion_libration_torsions"], rel=1e-12)
        assert res["angle_libration_max"] == float(sa[:, 4].max()) and res["torsion_libration_max"] == float(st[:, 4].max())
    else:
        assert [res[k] for k in ("angle_libration_angles", "angle_libration_mean", "angle_libration_max",
                                 "torsion_libration_torsions", "torsion_libration_mean", "torsion_libration_max")] == [0, 0.0, 0.0] * 2


@pytest.mark.parametrize("extra", [[], ["--rigid_molecule", "--tls_fit"]], ids=["plain", "tls"])
def test_the_flag_adds_the_tables_and_changes_nothing_else(work, monkeypatch, capsys, extra):
    from cartnet_amd import metrics as gm
    from cartnet_amd.predict import AT_KEYS, TT_KEYS, angle_table_entries
    plain, old = _run(work, monkeypatch, capsys, "plain.pkl", *extra)
    res, out = _run(work, monkeypatch, capsys, "table.pkl", "--angle_table", *extra)
    assert set(res) == set(plain) | AT_JSON | TT_JSON and not set(plain) & (AT_JSON | TT_JSON)
    assert list(res)[-10:] == ["angles_listed", "angle_mean", "angle_libration_angles", "angle_libration_mean",
                               "angle_libration_max", "torsions_listed", "torsions_undefined", "torsion_libration_torsions",
                               "torsion_libration_mean", "torsion_libration_max"]
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    assert list(out) == list(old) + list(AT_KEYS) + list(TT_KEYS)             # the pickle's keys and their order
    assert not [k for k in old if k.startswith(("angles_", "torsions_"))]     # with the flag off: no new key
    for k in old:                                                             # every key of the pass without the flag: its bits
        assert len(old[k]) == len(out[k]) == 3 and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    tls = bool(extra)
    _check_entries(out, res, 3, tls)
    s = _graphed(work[2])
    for g in range(3):                                                        # crystal g alone, from the pickle's own u_cart
        b = s.collate([g])
        rp = gm.target_row_ptr(b)
        index = gm.angle_index(b, rp, 0.4, rows=ROWS[g])
        assert index.table_ptr_host[:, 1].tolist() == [int(out["angles_stats"][g][0]), int(out["torsions_stats"][g][0])]
        u = out["u_cart"][g].cuda()
        tf = gm.tls_fit(u, b, rp, gm.molecules(b, rp, 0.4, rows=ROWS[g])) if tls else None
        want = angle_table_entries(gm.angle_table(b, rp, index, tf), b)
        for key in AT_KEYS + TT_KEYS:
            t = want[key][0] if key.endswith("stats") else want[key]
            assert _same(out[key][g], t.cpu().contiguous()), (key, g)
    if tls:
        assert [sorted(set(t.tolist())) for t in out["angles_tls_rank"]][1] == [0]          # the polymer is not fitted
        assert any(bool((t > 0).any()) for t in out["angles_tls_rank"])


def test_at_two_temperatures_the_raw_columns_are_the_same_bytes(work, monkeypatch, capsys):
    from cartnet_amd.predict import AT_KEYS, TT_KEYS
    res, out = _run(work, monkeypatch, capsys, "temps.pkl", "--angle_table", "--predict_temperatures", "100,200",
                    "--rigid_molecule", "--tls_fit")
    assert res["entries"] == 6 and res["crystals"] == 3 and list(out)[-1] == "series"
    assert [k for k in out if k != "series"][-15:] == list(AT_KEYS) + list(TT_KEYS)
    for key in AT_KEYS + TT_KEYS:                                             # every entry carries the keys
        assert len(out[key]) == 6, key
    _check_entries(out, res, 6, True)
    for g in range(3):                                                        # what is listed does not depend on U
        for key in ("angles_a", "angles_b", "angles_c", "angles_value", "torsions_a", "torsions_b", "torsions_c",
                    "torsions_d", "torsions_value"):
            assert _same(out[key][2 * g], out[key][2 * g + 1]), (key, g)
    assert any(not _same(out["angles_libration"][2 * g], out["angles_libration"][2 * g + 1]) for g in range(3))


def test_beside_the_bond_table_its_keys_keep_their_bytes_and_the_index_is_built_once(work, monkeypatch, capsys):
    from cartnet_amd import predict as pr
    bonds, old = _run(work, monkeypatch, capsys, "bonds.pkl", "--bond_table")
    calls = {"bond_index": 0, "angle_index": 0, "angle_table_call": 0}
    shared = []
    for name in calls:
        def counted(*a, _f=getattr(pr, name), _k=name, **kw):
            calls[_k] += 1
            if _k == "angle_index":
                shared.append(kw.get("bonds") is not None)
            return _f(*a, **kw)
        monkeypatch.setattr(pr, name, counted)
    res, out = _run(work, monkeypatch, capsys, "both.pkl", "--bond_table", "--angle_table")
    assert calls == {"bond_index": 2, "angle_index": 2, "angle_table_call": 2} and shared == [True, True]   # two batches
    assert list(out) == list(old) + list(pr.AT_KEYS) + list(pr.TT_KEYS)       # after bonds_*
    for k in old:
        assert all(_same(p, q) for p, q in zip(old[k], out[k])), k
    assert {k: v for k, v in res.items() if k in bonds and k != "output"} == {k: v for k, v in bonds.items() if k != "output"}
    for g in range(3):                                                        # every torsion's bond is a row of the bond table
        rows = set(zip(out["bonds_a"][g].tolist(), out["bonds_b"][g].tolist()))
        assert set(zip(out["torsions_b"][g].tolist(), out["torsions_c"][g].tolist())) <= rows
