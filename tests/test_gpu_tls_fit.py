"""``cartnet_adp_tls_fit`` (csrc/tls_ops.hip) against ``bonds.tls_fit_host`` on the arrays the kernel read: seven crystals
in one batch that hold every size class of the kernel's passes (below the minimum, 5, 17, past one and two strides of 64
interleaved in one cell), the rank-deficient shapes, a periodic molecule, rows that are not atoms, more molecules than
slots and a crystal without rows in the middle.  Both sides compute in fp64 and round once."""
import numpy as np
import pytest
import torch

import molecule_utils as mu
import tls_utils as tu
from test_gpu_bond_test import _make

pytestmark = pytest.mark.gpu

BLOCKS = {"T": slice(0, 6), "L": slice(6, 12), "S": slice(12, 21), "origin": slice(21, 24)}


@pytest.fixture(scope="module")
def fixture():
    """The batch, its molecules found on the GPU, one ``tls_fit`` and the numpy rule on the same arrays; computed once."""
    from cartnet_amd import metrics as gm
    from cartnet_amd.bonds import tls_fit_host
    crystals, rows = tu.gpu_crystals()
    batch, u, row_ptr = _make(crystals, 0, u=torch.from_numpy(rows))
    mo = gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
    res = gm.tls_fit(u, batch, row_ptr, mo)
    host = {k: getattr(mo, k).cpu().numpy() for k in ("label", "x", "size", "status")}
    mask = batch["non_H_mask"].cpu().numpy()
    ref = tls_fit_host(u.cpu().numpy(), host["label"], host["x"], mu.atom_rows(mask), host["status"], host["size"],
                       batch["ptr"].cpu().numpy())
    return batch, u, row_ptr, mo, res, host, ref


def _molecules(host, mask):
    """``{root atom: rows of its molecule}``"""
    row = mu.atom_rows(mask)
    return {int(r): row[host["label"] == r] for r in np.nonzero(host["label"] == np.arange(len(mask)))[0]}


def test_the_fixture_holds_every_kind(fixture):
    batch, u, row_ptr, mo, res, host, ref = fixture
    assert mo.crystal_counts[:, 0].tolist() == [4.0, 2.0, 3.0, 0.0, 1.0, 2.0, 11.0]
    assert mo.crystal_counts[:, 2].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0] and float(mo.crystal_counts[:, 3].sum()) == 0
    fits = ref["molecules"]
    assert sorted(len(f["resid"]) for f in fits.values()) == [5] * 13 + [6, 6, 7, 8, 17, 65, 130]
    assert sorted(f["rank"] for f in fits.values()) == [14, 19, 19] + [20] * 17
    sizes = host["size"][ref["rank"] == 0]
    assert sorted(set(sizes.tolist())) == [3, 4, 8]                           # below the minimum, and the polymer
    assert int(batch["ptr"][4] - batch["ptr"][3]) == 3 and int(row_ptr[4] - row_ptr[3]) == 0      # no rows in the middle
    assert int((~batch["non_H_mask"]).sum()) == 3 + 13                        # rows are not atoms
    for f in fits.values():                                                   # no decision hangs on a rounding
        ev = f["eigenvalues"]
        assert not ((ev > 1e-13) & (ev < 1e-9)).any() and 0 < f["sweeps"] <= 15
    label = host["label"][int(batch["ptr"][1]):int(batch["ptr"][2])]
    assert len(set(label.tolist())) == 2 and (label[1:] != label[:-1]).sum() > 50      # interleaved


def test_rows_against_the_numpy_rule(fixture):
    batch, u, row_ptr, mo, res, host, ref = fixture
    M = int(u.shape[0])
    got = {k: getattr(res, k).cpu().numpy() for k in res._fields}
    assert got["u_tls"].shape == (M, 3, 3) and got["params"].shape == (M, 24) and got["eig"].shape == (M, 6)
    assert all(got[k].shape == (M,) for k in ("resid", "rank", "rfac")) and got["rank"].dtype == np.int32
    assert all(got[k].dtype == np.float32 for k in ("u_tls", "resid", "params", "eig", "rfac"))
    assert np.array_equal(got["rank"], ref["rank"])
    neutral = ref["rank"] == 0
    assert neutral.sum() == 4 + 3 + 8
    for k in ("u_tls", "params", "eig"):
        assert np.isnan(got[k][neutral]).all() and not np.isnan(got[k][~neutral]).any(), k
    assert (got["resid"][neutral] == 0).all() and (got["rfac"][neutral] == 0).all()
    U = u.cpu().numpy().astype(np.float64)
    worst = {"u_tls": 0.0, "resid": 0.0, "rfac": 0.0, "params": 0.0, "eig": 0.0}
    for root, rows in _molecules(host, batch["non_H_mask"].cpu().numpy()).items():
        if root not in ref["molecules"]:
            continue
        fit = ref["molecules"][root]
        bound = tu.EPS22 * np.abs(U[rows]).max()
        e_u = np.abs(got["u_tls"][rows].astype(np.float64) - ref["u_tls"][rows]).max()
        e_r = np.abs(got["resid"][rows].astype(np.float64) - ref["resid"][rows]).max()
        e_f = np.abs(got["rfac"][rows].astype(np.float64) - ref["rfac"][rows]).max() / ref["rfac"][rows[0]]
        worst.update(u_tls=max(worst["u_tls"], e_u / bound), resid=max(worst["resid"], e_r / bound), rfac=max(worst["rfac"], e_f))
        assert e_u <= bound and e_r <= bound and e_f <= 1e-5, (root, len(rows), e_u, e_r, e_f, bound)
        assert (got["resid"][rows] > 0).all() and got["rfac"][rows[0]] > 5e-4  # the noise is there
        for k in ("params", "eig", "rank", "rfac"):                           # replicated on every row of the molecule
            assert (got[k][rows] == got[k][rows[0]]).all(), (root, k)
        kept = fit["eigenvalues"][fit["eigenvalues"] > 1e-10]
        if kept.min() < 1e-6 or fit["rank"] < 20:
            continue                                                          # compared through u_tls alone
        for name, sl in BLOCKS.items():
            e = np.abs(got["params"][rows[0], sl].astype(np.float64) - ref["params"][rows[0], sl]).max()
            b = tu.EPS22 * np.abs(ref["params"][rows[0], sl]).max()
            worst["params"] = max(worst["params"], e / b)
            assert e <= b, (root, name, e, b)
        for sl in (slice(0, 3), slice(3, 6)):
            e = np.abs(got["eig"][rows[0], sl].astype(np.float64) - ref["eig"][rows[0], sl]).max()
            b = tu.EPS22 * np.abs(ref["eig"][rows[0], sl]).max()
            worst["eig"] = max(worst["eig"], e / b)
            assert e <= b, (root, sl, e, b)
            assert (np.diff(got["eig"][rows[0], sl]) >= 0).all()              # ascending
        assert abs(float(got["params"][rows[0], [12, 16, 20]].astype(np.float64).sum())) <= 3 * 2.0 ** -24 * np.abs(
            got["params"][rows[0], 12:21]).max()                              # tr S = 0 up to the rounding of the store
    print("largest deviations, as fractions of their bounds (rfac: relative): "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    compared = [r for r, f in ref["molecules"].items() if f["rank"] == 20 and f["eigenvalues"].min() >= 1e-6]
    assert len(compared) == 15                                                # helices of 5 (12), 17, 7 and the ring


def test_crystal_stats_against_the_rows(fixture):
    batch, u, row_ptr, mo, res, host, ref = fixture
    stats = res.crystal_stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (7, 6)
    assert stats[:, 0].tolist() == [2.0, 2.0, 3.0, 0.0, 0.0, 2.0, 11.0] and stats[:, 1].tolist() == [0, 0, 3.0, 0, 0, 0, 0]
    assert stats[3].tolist() == [0.0] * 6 and stats[4].tolist() == [0.0] * 6
    rp = row_ptr.cpu().numpy()
    U = u.cpu().numpy().astype(np.float64)
    sym = 0.5 * (U + U.transpose(0, 2, 1))
    resid, rank, eig = (getattr(res, k).cpu().numpy() for k in ("resid", "rank", "eig"))
    mask = batch["non_H_mask"].cpu().numpy()
    root_row = mu.atom_rows(mask)[np.nonzero(host["label"] == np.arange(len(mask)))[0]]
    for g in range(7):
        rows = np.arange(rp[g], rp[g + 1])
        fitted = rows[rank[rows] != 0]
        roots = np.intersect1d(fitted, root_row)
        r = resid[fitted].astype(np.float64)
        assert stats[g, 0] == len(roots) and stats[g, 1] == (rank[roots] < 20).sum()
        assert stats[g, 2] == ((eig[roots, 0] < 0) | (eig[roots, 3] < 0)).sum()
        assert stats[g, 3] == pytest.approx((r * r).sum(), rel=1e-12) and stats[g, 5] == (r.max() if len(r) else 0.0)
        assert stats[g, 4] == pytest.approx((sym[fitted] ** 2).sum(), rel=1e-12)
    # the numpy rule's own figures; not the third: the sign of a vanishing principal value of a rank-deficient L is noise
    assert np.abs(stats[:, :2] - ref["crystal_stats"][:, :2]).max() == 0
    assert np.abs(stats[:, 3:] - ref["crystal_stats"][:, 3:]).max() <= 1e-5 * np.abs(ref["crystal_stats"][:, 3:]).max()


def test_two_calls_give_the_same_bytes_and_nothing_else_is_written(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, mo, res, host, ref = fixture
    again = gm.tls_fit(u, batch, row_ptr, mo)
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # a crystal alone gives its rows the values they have in the batch: the slots and the neighbours do not matter
    crystals, rows = tu.gpu_crystals()
    first = int(row_ptr[6])
    alone, v, rp = _make(crystals[6:], 0, u=torch.from_numpy(rows[first:]))
    one = gm.tls_fit(v, alone, rp, gm.molecules(alone, rp, mu.TOL, rows=int(v.shape[0])))
    for k in ("u_tls", "resid", "params", "eig", "rank", "rfac"):
        assert getattr(one, k).cpu().numpy().tobytes() == getattr(res, k)[first:].cpu().numpy().tobytes(), k


def test_argument_checks_and_no_rows():
    from cartnet_amd import metrics as gm
    pos = tu.helix(5, (3.0, 3.0, 3.0))
    batch, u, row_ptr = _make([(pos, mu.cubic(20.0), np.full(5, 6))], 14, u=torch.from_numpy(tu.rigid_rows(pos, 3, tu.NOISE)))
    mo = gm.molecules(batch, row_ptr, rows=5)
    assert gm.tls_fit(u, batch, row_ptr, mo).rank.tolist() == [20] * 5
    with pytest.raises(ValueError, match="u must be"):
        gm.tls_fit(u.double(), batch, row_ptr, mo)
    with pytest.raises(ValueError, match="does not belong"):
        gm.tls_fit(u[:1], batch, row_ptr, mo)
    with pytest.raises(ValueError, match="does not belong"):
        gm.tls_fit(u, batch, row_ptr, mo._replace(x=mo.x.float()))
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.tls_fit(u, {k: v for k, v in batch.items() if k != "ptr"}, row_ptr, mo)
    # all atoms of the molecule in one point (x is the caller's): rho == 0, not fitted
    point = gm.tls_fit(u, batch, row_ptr, mo._replace(x=torch.zeros_like(mo.x)))
    assert point.rank.tolist() == [0] * 5 and bool(torch.isnan(point.u_tls).all()) and point.resid.tolist() == [0.0] * 5
    assert point.crystal_stats.tolist() == [[0.0] * 6]
    # M == 0 and B == 0 return at once
    none = dict(batch, non_H_mask=torch.zeros(5, dtype=torch.bool, device="cuda:0"))
    zero = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    empty = gm.molecules(none, zero, rows=0)
    assert gm.tls_fit(u[:0], none, zero, empty).crystal_stats.tolist() == [[0.0] * 6]
    from cartnet_amd import lib
    assert lib.load().cartnet_adp_tls_fit(None, None, None, None, None, None, None, None, 0, 5, 5, None, None, None, None,
                                          None, None, None, None) == 0
    assert lib.load().cartnet_adp_tls_fit(None, None, None, None, None, None, None, None, 1, 5, 5, None, None, None, None,
                                          None, None, None, None) == 1          # null pointers are an error, not a fault
