"""``write_cif`` / ``write_cif_symmetric`` against files written once by the writers as they were before they shared a line
builder (tests/golden/cif_writers/, tests/golden/make_golden_cif_writers.py): the entries of tests/test_predict_host.py,
tests/test_cif_host.py and tests/test_riding_host.py, each with and without ``u_iso`` / ``u_iso_asym``, byte for byte.  And
the table that says how every key of a ``predict_adps`` result is split on the host covers exactly the keys that travel as
tensors."""
import os

import pytest
import torch

import cif_utils as cu
import predict_utils as pu
from golden_utils import GOLDEN

DIR = os.path.join(GOLDEN, "cif_writers")


def _iso(z, seed):
    """One isotropic value per atom, the last hydrogen an orphan (NaN: written ``?``)."""
    u = torch.rand(len(z), generator=torch.Generator().manual_seed(seed)) * 0.05 + 0.01
    h = [i for i, v in enumerate(z) if int(v) == 1]
    if h:
        u[h[-1]] = float("nan")
    return u


def cases() -> dict:
    """file name -> (writer name, entry)."""
    from cartnet_amd import cif
    from test_predict_host import _entry as predict_entry
    from test_riding_host import _entry as riding_entry
    out = {}
    e = predict_entry(pu.cells()["triclinic_rotated"], [6, 1, 8, 17, 1, 26, 118])
    out["predict_p1.cif"] = ("write_cif", e)
    out["predict_p1_iso.cif"] = ("write_cif", dict(e, u_iso=_iso(e["z"].tolist(), 7)))
    out["riding_p1.cif"] = ("write_cif", riding_entry(False))
    out["riding_p1_iso.cif"] = ("write_cif", riding_entry(True))
    s = riding_entry(False)
    s.update(asym_z=s["z"], asym_labels=["C1", "O1", "H1", "H2"], asym_frac=s["frac"].double(), u_cif_asym=s["u_cif"],
             symops=["x, y, z", "-x, -y, -z"])
    out["riding_sym.cif"] = ("write_cif_symmetric", s)
    out["riding_sym_iso.cif"] = ("write_cif_symmetric", dict(s, u_iso_asym=torch.tensor([0.031, 0.041, 0.0465, float("nan")])))
    for key in ("b", "c"):
        (c,) = cif.read_cif(cu.cif_text(key, name=f"in_{key}"))
        heavy = [i for i, z in enumerate(c.z) if z != 1]
        u = (torch.rand(len(heavy), 6, generator=torch.Generator().manual_seed(5)) - 0.3) * 0.05
        s = {"name": c.name, "cell": torch.from_numpy(c.cell()).float(), "temp": c.temperature, "asym_labels": c.labels,
             "asym_frac": torch.tensor(c.frac, dtype=torch.float64), "asym_z": torch.tensor(c.z, dtype=torch.int32),
             "symops": c.symop_strings, "u_cif_asym": u, "spread": torch.zeros(len(heavy))}
        out[f"cif_{key}_sym.cif"] = ("write_cif_symmetric", s)
        out[f"cif_{key}_sym_iso.cif"] = ("write_cif_symmetric", dict(s, u_iso_asym=_iso(c.z, 8)))
    return out


def test_every_case_has_its_file_and_no_file_is_left_over():
    assert sorted(os.listdir(DIR)) == sorted(cases())


@pytest.mark.parametrize("name", sorted(cases()))
def test_writers_give_the_committed_bytes(tmp_path, name):
    from cartnet_amd import predict
    writer, entry = cases()[name]
    path = str(tmp_path / name)
    getattr(predict, writer)(path, entry)
    with open(path, "rb") as f, open(os.path.join(DIR, name), "rb") as g:
        assert f.read() == g.read()


def test_the_split_table_covers_exactly_the_keys_that_travel_as_tensors():
    from cartnet_amd import predict as p
    every = p.KEYS + p.SYM_KEYS + p.ROT_KEYS + p.BOND_KEYS + p.H_KEYS + p.H_SYM_KEYS
    host_only = {"name", "temp", "asym_labels", "asym_frac", "asym_z", "symops", "u_iso_asym", "h_parent_asym"}
    assert len(set(every)) == len(every) and host_only < set(every)
    assert set(p.SPLIT) == set(every) - host_only
    assert set(p.SPLIT.values()) == {"crystal", "atom", "row", "site"}
