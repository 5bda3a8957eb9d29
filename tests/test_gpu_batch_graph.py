"""The batch graph is built once per batch: ``main.py --predict`` with all five bond-graph analyses on, two crystals in two
batches at two temperatures -- eleven analysis calls per batch -- builds the two lookups (``metrics._atom_lookups``) twice."""
import pytest
import torch

import aniso_utils as au
from test_gpu_main_rigid_molecule import MODEL, _load

pytestmark = pytest.mark.gpu


def test_the_lookups_are_built_once_per_batch(tmp_path, monkeypatch, capsys):
    import main as entry
    from cartnet_amd import metrics as gm, predict as pr, shard
    from cartnet_amd.config import set_cfg
    from cartnet_amd.data import Data
    from cartnet_amd.master import create_model
    crystals = [Data(x=torch.tensor(z, dtype=torch.int64), pos=torch.tensor(pos, dtype=torch.float32),
                     cell=torch.tensor(cell, dtype=torch.float32).unsqueeze(0), natoms=torch.tensor([len(z)]),
                     temperature=torch.tensor([0.25])) for pos, cell, z, _ in (au.methyl_crystal(), au.face_crystal())]
    try:
        entry.fill_cfg(entry.build_parser().parse_args(MODEL))
        torch.manual_seed(0)
        torch.save({"model_state": create_model().state_dict()}, str(tmp_path / "fresh.ckpt"))
        shard.write_shard(str(tmp_path / "two.cnshard"), crystals, names=["methyl", "face"])
        monkeypatch.chdir(tmp_path)
        calls = {"lookups": 0, "analyses": 0}

        def counted(*a, _f=gm._atom_lookups, **kw):
            calls["lookups"] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(gm, "_atom_lookups", counted)
        for name in ("bond_test", "molecule_test", "tls_fit_call", "riding_h_call", "aniso_h_call", "find_molecules"):
            def analysis(*a, _f=getattr(pr, name), **kw):
                calls["analyses"] += 1
                assert isinstance(a[0] if _f is gm.molecules else a[1], gm.BatchGraph)
                return _f(*a, **kw)
            monkeypatch.setattr(pr, name, analysis)
        res = entry.main(["--predict", "--predict_input", "two.cnshard", "--checkpoint_path", "fresh.ckpt", "--eval_batch", "1",
                          "--rigid_bond", "--riding_h", "--rigid_molecule", "--tls_fit", "--aniso_h",
                          "--predict_temperatures", "100:200:100", "--predict_output", "out.pkl"] + MODEL)
        capsys.readouterr()
    finally:
        set_cfg()
    out = _load("out.pkl")
    assert res["crystals"] == 2 and res["entries"] == 4 and len(out["h_source"]) == 4 and "bond_count" in out
    assert calls == {"lookups": 2, "analyses": 2 * (1 + 2 * 5)}               # per batch: the molecules, then five per temperature
