"""``main.py --predict --predict_temperatures SPEC`` end to end with a small CartNet whose checkpoint the test saves: an
unlabeled shard of three crystals at 100:300:100 (JSON line, pickle, nine CIFs), one CIF file as the input (site-averaged
ADPs and the file's own setting per temperature), and the two refusals."""
import json
import math
import os
import pickle

import pytest
import torch

import cif_utils as cu
import predict_utils as pu

pytestmark = pytest.mark.gpu

MODEL = ["--dim_in", "32", "--num_layers", "2"]
NAMES = ["c12", "c13", "c14"]
PLAIN_JSON = {"crystals", "rows", "u_eq_mean", "non_positive_rows", "output", "cif_dir"}
SERIES_JSON = {"ueq_slope_mean", "non_increasing_rows", "rows_with_drops", "series_resid_max"}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(directory, checkpoint of a fresh small CartNet, the unlabeled shard of three crystals)."""
    import main as entry
    from cartnet_amd import shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    d = tmp_path_factory.mktemp("temperatures")
    entry.fill_cfg(entry.build_parser().parse_args(MODEL))
    torch.manual_seed(0)
    ckpt = str(d / "fresh.ckpt")
    torch.save({"model_state": create_model().state_dict()}, ckpt)
    src = str(d / "three.cnshard")
    shard.write_shard(src, pu.six_crystals(False)[1:4], names=NAMES)
    yield d, ckpt, src
    set_cfg()


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _temperature_line(path):
    (line,) = [l for l in open(path).read().splitlines() if l.startswith("_diffrn_ambient_temperature")]
    return line


def test_a_shard_at_three_temperatures(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd.predict import KEYS
    d, ckpt, src = work
    monkeypatch.chdir(d)
    common = ["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--eval_batch", "2"] + MODEL
    plain = entry.main(common + ["--predict_output", "plain.pkl"])
    assert set(plain) == PLAIN_JSON                                           # without the flag the line is as it was
    capsys.readouterr()
    res = entry.main(common + ["--predict_output", "series.pkl", "--predict_cif_dir", "cifs", "--predict_temperatures",
                               "100:300:100"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and set(res) == PLAIN_JSON | SERIES_JSON | {"entries", "temperatures"}
    assert res["crystals"] == 3 and res["entries"] == 9 and res["temperatures"] == [100, 200, 300]
    assert res["rows"] == 3 * plain["rows"]
    out = _load("series.pkl")
    assert tuple(out) == KEYS + ("series",) and tuple(_load("plain.pkl")) == KEYS
    assert out["name"] == [f"{n}_{t}K" for n in NAMES for t in (100, 200, 300)]
    assert out["temp"] == [100.0, 200.0, 300.0] * 3
    series = out["series"]
    assert series["name"] == NAMES and all(t.tolist() == [100.0, 200.0, 300.0] for t in series["temps"])
    stats = torch.stack(series["t_stats"])
    assert [int(t.shape[0]) for t in series["t_ueq_slope"]] == [int(t.shape[0]) for t in out["u_eq"][::3]]
    assert res["ueq_slope_mean"] == float(stats[:, 0].sum()) / plain["rows"]
    assert res["ueq_slope_mean"] == pytest.approx(torch.cat(series["t_ueq_slope"]).double().mean().item(), rel=1e-9)
    assert res["non_increasing_rows"] == int((~(torch.cat(series["t_ueq_slope"]) > 0)).sum()) == int(stats[:, 1].sum())
    assert res["rows_with_drops"] == int((torch.cat(series["t_drops"]) > 0).sum()) == int(stats[:, 2].sum())
    assert res["series_resid_max"] == torch.cat(series["t_resid"]).double().max().item()
    assert all(math.isfinite(res[k]) for k in SERIES_JSON)
    print(f"fresh weights: U_eq slope mean {res['ueq_slope_mean']:.3e} A^2/K, {res['non_increasing_rows']} of "
          f"{plain['rows']} rows not increasing, {res['rows_with_drops']} with a drop, largest residual "
          f"{res['series_resid_max']:.3e}")
    assert sorted(os.listdir("cifs")) == sorted(f"{n}_{t}K.cif" for n in NAMES for t in (100, 200, 300))
    for n in NAMES:
        for t in (100, 200, 300):
            path = os.path.join("cifs", f"{n}_{t}K.cif")
            assert _temperature_line(path) == f"_diffrn_ambient_temperature {t:.2f}"
            assert open(path).read().splitlines()[0] == f"data_{n}_{t}K"


def test_one_cif_file_at_two_temperatures(work, monkeypatch, capsys):
    import main as entry
    from cartnet_amd.cif import read_cif
    from cartnet_amd.predict import KEYS, SYM_KEYS
    d, ckpt, _ = work
    monkeypatch.chdir(d)
    (d / "b.cif").write_text(cu.cif_text("b", name="crystal_b", labeled=False))
    res = entry.main(["--predict", "--predict_input", "b.cif", "--checkpoint_path", ckpt, "--predict_output", "cif.pkl",
                      "--predict_cif_dir", "cif_out", "--predict_temperatures", "120,290.5"] + MODEL)
    assert res["crystals"] == 1 and res["entries"] == 2 and res["rejected"] == 0 and res["rows"] == 2 * cu.ATOMS["b"][1]
    out = _load("cif.pkl")
    assert tuple(out) == KEYS + SYM_KEYS + ("series",) and out["name"] == ["crystal_b_120K", "crystal_b_290.5K"]
    (src,) = read_cif(cu.cif_text("b"))
    heavy = [lab for lab, z in zip(src.labels, src.z) if z != 1]
    for k, t in enumerate((120.0, 290.5)):
        assert tuple(out["u_cif_asym"][k].shape) == (len(heavy), 6) and bool(torch.isfinite(out["u_cif_asym"][k]).all())
        path = os.path.join("cif_out", f"{out['name'][k]}.cif")
        assert _temperature_line(path) == f"_diffrn_ambient_temperature {t:.2f}"
        (back,) = read_cif(path)                                              # the file's own setting, per temperature
        assert back.labels == src.labels and len(back.symops) == len(src.symops) and sorted(back.u_aniso) == sorted(heavy)
        assert back.temperature == t
    assert not torch.equal(out["u_cif_asym"][0], out["u_cif_asym"][1])
    assert sorted(os.listdir("cif_out")) == ["crystal_b_120K.cif", "crystal_b_290.5K.cif"]


def test_refusals_come_before_the_device_is_touched(work, monkeypatch):
    import main as entry
    d, ckpt, src = work
    monkeypatch.chdir(d)

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry, "create_model", touched)
    common = ["--predict_input", src, "--checkpoint_path", ckpt, "--predict_temperatures", "100,200"] + MODEL
    with pytest.raises(SystemExit, match="--disable_temp"):
        entry.main(["--predict", "--disable_temp"] + common)
    with pytest.raises(SystemExit, match="--predict only"):
        entry.main(common)
    with pytest.raises(SystemExit, match="strictly increasing"):
        entry.main(["--predict", "--predict_input", src, "--checkpoint_path", ckpt, "--predict_temperatures", "200,100"])
