"""``main.py --rigid_molecule --tls_fit`` end to end on the four hand-built molecular crystals of the rigid-molecule test
(two methanols, a planar chain of six through a cell face, the polymer, a puckered ring with two lone atoms): the keys and
JSON fields with their shapes, ``tls_u`` against a direct ``metrics.tls_fit`` per crystal, the flag beside ``--rotations``
and ``--predict_temperatures``, ``--inference`` with the truth as the baseline, and nothing else changed by the flag."""
import json
import math

import pytest
import torch

from test_gpu_main_rigid_molecule import INFERENCE_JSON, MODEL, NAMES, ROWS, _crystals, _graphed, _load, _same

pytestmark = pytest.mark.gpu

TLS_JSON = {"tls_molecules", "tls_rank_deficient", "tls_nonphysical", "tls_r", "tls_resid_max"}
TLS_SHAPES = {"tls_u": (3, 3), "tls_resid": (), "tls_T": (3, 3), "tls_L": (3, 3), "tls_S": (3, 3), "tls_origin": (3,),
              "tls_T_principal": (3,), "tls_L_principal": (3,), "tls_rank": (), "tls_r": ()}
# per crystal: the rank on its rows -- only the chain (planar: 19) and the ring (20) have five or more atoms and status 0
RANKS = ([0] * 4, [19] * 6, [0] * 8, [20] * 6 + [0, 0])


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard of the four crystals)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("tls")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "four.cnshard")
    shard.write_shard(src, _crystals(False), names=list(NAMES))
    yield d, ckpt, src
    set_cfg()


def _check_entries(out, res, n_entries, suffix=""):
    """What holds for every entry of a flag-on result: shapes and dtypes, the neutral rows, ``tls_stats`` and the JSON line
    against the row keys."""
    r2 = s2 = 0.0
    for k in range(n_entries):
        n = int(out["tls_u" + suffix][k].shape[0])
        for key, tail in TLS_SHAPES.items():
            t = out[key + suffix][k]
            assert t.dtype == (torch.int32 if key == "tls_rank" else torch.float32) and tuple(t.shape) == (n,) + tail, (key, k)
        rank = out["tls_rank" + suffix][k]
        assert rank.tolist() == list(RANKS[k * len(RANKS) // n_entries])
        off = rank == 0
        for key in ("tls_u", "tls_T", "tls_L", "tls_S", "tls_origin", "tls_T_principal", "tls_L_principal"):
            t = out[key + suffix][k].reshape(n, -1)
            assert bool(torch.isnan(t[off]).all()) and not bool(torch.isnan(t[~off]).any()), (key, k)
        assert bool((out["tls_resid" + suffix][k][off] == 0).all()) and bool((out["tls_r" + suffix][k][off] == 0).all())
        assert bool((out["tls_resid" + suffix][k][~off] > 0).all())
        for key in ("tls_T", "tls_L"):                                        # symmetric, and the principal values are theirs
            t = out[key + suffix][k][~off]
            assert torch.equal(t, t.transpose(1, 2))
            if len(t):
                want = torch.linalg.eigvalsh(t.double())
                got = out[key + "_principal" + suffix][k][~off].double()
                assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        s = out["tls_S" + suffix][k][~off].double()
        assert float(s.diagonal(dim1=1, dim2=2).sum(1).abs().max() if len(s) else 0.0) <= 1e-6 * float(s.abs().max() if len(s) else 1.0)
        u = out["u_cart" if "u_cart" in out else "pred"][k] if not suffix else out["true"][k]
        sym = 0.5 * (u + u.transpose(1, 2)).double()
        fit = out["tls_u" + suffix][k].double()
        resid = (sym - fit)[~off].flatten(1).norm(dim=1)
        assert float((resid - out["tls_resid" + suffix][k][~off].double()).abs().max() if len(resid) else 0.0) <= 1e-6 * float(u.abs().max())
        r2 += float((out["tls_resid" + suffix][k][~off].double() ** 2).sum())
        s2 += float((sym[~off] ** 2).sum())
        if not suffix and "tls_stats" in out:
            st = out["tls_stats"][k]
            assert st.dtype == torch.float64 and tuple(st.shape) == (6,)
            assert st[0] == (1 if bool((~off).any()) else 0) and st[1] == (1 if 19 in rank.tolist() else 0)
            assert float(st[5]) == float(out["tls_resid"][k].max())
    assert res["tls_r" + suffix] == pytest.approx(math.sqrt(r2 / s2), rel=1e-9) and 0 < res["tls_r" + suffix] < 1
    assert res["tls_resid_max" + suffix] == max(float(t.max()) for t in out["tls_resid" + suffix])
    assert res["tls_rank_deficient" + suffix] == n_entries // 4 and res["tls_molecules"] == 2 * (n_entries // 4)
    assert 0 <= res["tls_nonphysical" + suffix] <= res["tls_molecules"]


def test_predict_carries_the_direct_result_and_changes_nothing_else(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd.metrics import molecules, target_row_ptr, tls_fit
    from cartnet_amd.predict import KEYS, MOL_KEYS, TLS_KEYS, tls_entries
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "3", "--rigid_molecule"] + MODEL
    plain = entry.main(common + ["--predict_output", "plain.pkl"])
    capsys.readouterr()
    res = entry.main(common + ["--predict_output", "tls.pkl", "--tls_fit"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    old, out = _load("plain.pkl"), _load("tls.pkl")
    assert not set(plain) & TLS_JSON and tuple(old) == KEYS + MOL_KEYS        # without the flag: as it was
    assert set(res) == set(plain) | TLS_JSON and list(out) == list(old) + list(TLS_KEYS)
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    for k in old:                                                             # every shared key: the same bits
        assert len(old[k]) == len(out[k]) == 4 and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 4)
    s = _graphed(src)
    for k in range(4):                                                        # crystal k alone: its own batch, its own graph
        b = s.collate([k])
        rp = target_row_ptr(b)
        mo = molecules(b, rp, 0.4, rows=ROWS[k])
        want = tls_entries(tls_fit(out["u_cart"][k].cuda(), b, rp, mo))
        for key in TLS_KEYS:
            t = want[key][0] if key == "tls_stats" else want[key]
            assert _same(out[key][k], t.cpu().contiguous()), (key, k)
    # the origin is the centroid in the frame of mol_pos
    for k in (1, 3):
        on = out["tls_rank"][k] > 0
        centre = out["mol_pos"][k][on].double().mean(0)
        assert float((out["tls_origin"][k][on].double() - centre).abs().max()) <= 1e-5


@pytest.mark.parametrize("extra", [["--rotations", "2"], ["--predict_temperatures", "100,200"]], ids=["rotations", "temperatures"])
def test_the_flag_composes(work, monkeypatch, capsys, extra):
    import main as entry
    from cartnet_amd.predict import TLS_KEYS
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "3", "--rigid_molecule"] + MODEL + extra
    plain = entry.main(common + ["--predict_output", "c_plain.pkl"])
    res = entry.main(common + ["--predict_output", "c_tls.pkl", "--tls_fit"])
    old, out = _load("c_plain.pkl"), _load("c_tls.pkl")
    assert set(res) == set(plain) | TLS_JSON and not set(plain) & TLS_JSON
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    assert [k for k in out if k != "series"] == [k for k in old if k != "series"] + list(TLS_KEYS)
    for k in old:
        if k != "series":
            assert len(old[k]) == len(out[k]) and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    T = 2 if extra[0] == "--predict_temperatures" else 1
    _check_entries(out, res, 4 * T)
    if T == 2:                                                                # fitted once per temperature, on that temperature's U
        assert {k: [_same(p, q) for p, q in zip(old["series"][k], out["series"][k])] for k in old["series"]} == \
            {k: [True] * 4 for k in old["series"]}
        for g in range(4):
            assert _same(out["tls_rank"][2 * g], out["tls_rank"][2 * g + 1]) and _same(out["tls_origin"][2 * g], out["tls_origin"][2 * g + 1])
        assert all(not _same(out["tls_u"][2 * g], out["tls_u"][2 * g + 1]) for g in (1, 3))


def test_inference_fits_prediction_and_truth(work, monkeypatch, capsys):
    import os
    import main as entry
    from cartnet_amd import evaluate, shard
    d, ckpt, _ = work
    monkeypatch.chdir(d)
    os.makedirs("splits", exist_ok=True)
    for part in ("train", "val", "test"):
        shard.write_shard(os.path.join("splits", f"{part}.cnshard"), _crystals(True))
    common = ["--inference", "--shard_dir", "splits", "--checkpoint_path", ckpt, "--eval_batch", "3", "--rigid_molecule"] + MODEL
    plain = entry.main(common + ["--inference_output", "inf_plain.pkl"])
    capsys.readouterr()
    res = entry.main(common + ["--inference_output", "inf_tls.pkl", "--tls_fit"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    old, out = _load("inf_plain.pkl"), _load("inf_tls.pkl")
    both = TLS_JSON | {k + "_true" for k in TLS_JSON if k != "tls_molecules"}
    assert line == res and set(res) == set(plain) | both and INFERENCE_JSON <= set(plain) and not set(plain) & both
    assert {k: v for k, v in res.items() if k in plain and k != "output"} == {k: v for k, v in plain.items() if k != "output"}
    keys = set(evaluate.TLS_ROW_KEYS)
    assert set(out) == set(old) | keys | {k + "_true" for k in keys} and keys == set(TLS_SHAPES)
    for k in old:
        assert len(old[k]) == len(out[k]) and all(_same(p, q) for p, q in zip(old[k], out[k])), k
    _check_entries(out, res, 4)
    _check_entries(out, res, 4, "_true")
    # the molecules are the same, the ADPs are not
    assert all(_same(p, q) for p, q in zip(out["tls_rank"], out["tls_rank_true"]))
    assert all(_same(p, q) for p, q in zip(out["tls_origin"], out["tls_origin_true"]))
    assert all(not _same(out["tls_u"][g], out["tls_u_true"][g]) for g in (1, 3))
    assert res["tls_r"] != res["tls_r_true"]
