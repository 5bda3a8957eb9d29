"""``cartnet_adp_molecule_test`` (csrc/molecule_ops.hip) against an fp64 numpy restatement on the arrays the kernel reads:
the per-row figures over all pairs of a molecule in atom order, the per-crystal sums of the values as stored, the neutral
rows of untested molecules, and the direction of the convention (a rigid body's amplitudes agree along every interatomic
vector, unwrapped through a cell face; independent ones do not)."""
import numpy as np
import pytest
import torch

import molecule_utils as mu
import predict_utils as pu
from test_gpu_bond_test import _make

pytestmark = pytest.mark.gpu

EPS23 = 2.0 ** -23


@pytest.fixture(scope="module")
def fixture():
    """The four crystals of ``pair_test_crystals`` as one batch, one direction of the last chain cut (its two halves are
    open), the molecules found on the GPU, and the reference on them; computed once."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _make(mu.pair_test_crystals(), 31)
    src, tgt = batch["edge_index"]
    first = int(batch["ptr"][3])
    keep = ~((src == first + 1) & (tgt == first + 2))
    assert int((~keep).sum()) == 1
    batch = dict(batch, edge_index=batch["edge_index"][:, keep], cart_dist=batch["cart_dist"][keep],
                 cart_dir=batch["cart_dir"][keep])
    mo = gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
    host = {k: getattr(mo, k).cpu().numpy() for k in ("label", "x", "size", "status")}
    ref, deltas = mu.pair_reference(u.cpu().numpy(), host["label"], host["x"], batch["non_H_mask"].cpu().numpy(),
                                    host["size"], host["status"], mu.THRESHOLD)
    return batch, u, row_ptr, mo, host, ref, deltas


def test_the_fixture_holds_the_sizes_and_the_untested_kinds(fixture):
    from cartnet_amd.bonds import MOLECULE_OPEN, MOLECULE_PERIODIC
    batch, u, row_ptr, mo, host, ref, deltas = fixture
    assert mo.crystal_counts.tolist() == [[3.0, 2.0, 0.0, 0.0, 17.0], [2.0, 2.0, 0.0, 0.0, 130.0],
                                          [1.0, 0.0, 1.0, 0.0, 8.0], [2.0, 0.0, 0.0, 2.0, 3.0]]
    tested = (host["status"] == 0) & (host["size"] >= 2)
    assert sorted(set(host["size"][tested].tolist())) == [2, 17, 65, 130] and (host["size"] == 1).sum() == 1
    assert (host["status"] == MOLECULE_PERIODIC).sum() == 8 and (host["status"] == MOLECULE_OPEN).sum() == 5
    # several molecules share a crystal and are interleaved: the label filter has work to do
    label = host["label"][int(batch["ptr"][1]):int(batch["ptr"][2])]
    assert len(set(label.tolist())) == 2 and (label[1:] != label[:-1]).sum() > 50
    assert np.array_equal(ref["pairs"], np.where(tested, host["size"] - 1, 0))           # no two atoms coincide
    assert np.abs(deltas - mu.THRESHOLD).min() > 1e-9                         # no decision hangs on a rounding
    assert 0 < ref["over"].sum() < ref["pairs"].sum()                         # the threshold splits the pairs


def test_rows_and_crystals_against_the_reference(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, mo, host, ref, _ = fixture
    res = gm.molecule_test(u, batch, row_ptr, mo, mu.THRESHOLD)
    M, B = int(u.shape[0]), 4
    got = {k: getattr(res, k).cpu().numpy() for k in ref}
    assert got["pairs"].dtype == np.int32 and got["worst"].dtype == np.int64 and got["over"].dtype == np.int32
    assert got["delta_sum"].dtype == np.float32 and got["delta_max"].dtype == np.float32
    for k in ("pairs", "worst", "over"):
        assert got[k].shape == (M,) and np.array_equal(got[k], ref[k]), k
    untested = ~((host["status"] == 0) & (host["size"] >= 2))
    assert untested.sum() == 14                                                # the single atom, the polymer, the open halves
    for k, neutral in (("pairs", 0), ("delta_sum", 0.0), ("delta_max", 0.0), ("worst", -1), ("over", 0)):
        assert (got[k][untested] == neutral).all(), k
    rp = row_ptr.cpu().numpy()
    U = u.cpu().numpy().astype(np.float64)
    stats = res.crystal_stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (B, 4)
    for g in range(B):
        sl = slice(rp[g], rp[g + 1])
        umax = np.abs(U[sl]).max()
        for k in ("delta_sum", "delta_max"):
            a, b = got[k][sl].astype(np.float64), ref[k][sl]
            err, bound = np.abs(a - b), EPS23 * np.abs(b) + 1e-12 * umax
            print(f"crystal {g} {k}: max error {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
            assert (err <= bound).all(), (g, k)
        # per crystal: the fp64 sums of the per-row values AS STORED
        assert stats[g, 0] == got["pairs"][sl].sum() and stats[g, 3] == got["over"][sl].sum()
        assert stats[g, 2] == got["delta_max"][sl].astype(np.float64).max()
        want = got["delta_sum"][sl].astype(np.float64).sum()
        assert abs(stats[g, 1] - want) <= 1e-12 * want                        # only the order differs
    assert stats[2].tolist() == [0.0] * 4 and stats[3].tolist() == [0.0] * 4
    # worst is an atom of the BATCH inside the row's own molecule
    rows = np.nonzero(got["worst"] >= 0)[0]
    atoms = np.nonzero(batch["non_H_mask"].cpu().numpy())[0]
    assert (host["label"][got["worst"][rows]] == host["label"][atoms[rows]]).all()
    again = gm.molecule_test(u, batch, row_ptr, mo, mu.THRESHOLD)
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # two runs, equal bytes


def test_direction_on_a_rigid_body_across_a_cell_face():
    """A chain of n = 17 through the x and the y face, ``U_i = T + [r_i]x L [r_i]x^T`` with r_i the TRUE unwrapped
    positions: rigid along every interatomic vector, so every |D| vanishes up to the rounding of the fp32 inputs.  The
    bound 32 n 2^-23 max|U|: up to n - 1 path edges each carry a relative direction error of at most 2 * 2^-23, pairs are
    no nearer than 0.8 bond lengths, the sensitivity to the direction is at most 2 |U_i - U_j|_2 <= 12 max|U|.  A wrong
    sign or a missed image would put an atom a cell away and break it by orders of magnitude, as independent random rows
    do: their mean |D| is at least 1000 times the bound."""
    from cartnet_amd import metrics as gm
    n, cell = 17, mu.cubic(30.0)
    pos, true = mu.chain(n, (20.0, 27.0, 5.0), cell, drift=(0.15, 0.0))
    assert (np.abs(pos - true).max(axis=0) > 10).tolist() == [True, True, False]
    U = torch.tensor(mu.rigid_body_rows(true, 41), dtype=torch.float32)
    batch, u, row_ptr = _make([(pos, cell, np.full(n, 6))], 41, u=U)
    mo = gm.molecules(batch, row_ptr, mu.TOL, rows=n)
    assert mo.crystal_counts.tolist() == [[1.0, 1.0, 0.0, 0.0, 17.0]]
    assert np.abs(mo.x.cpu().numpy() - (true - true[0])).max() < 1e-5
    res = gm.molecule_test(u, batch, row_ptr, mo, mu.THRESHOLD)
    bound = 32 * n * EPS23 * float(u.abs().max())
    print(f"rigid body: largest |D| {float(res.delta_max.max()):.3e}, bound {bound:.3e}")
    assert res.pairs.tolist() == [n - 1] * n and float(res.delta_max.max()) <= bound and res.over.tolist() == [0] * n
    loose, v, _ = _make([(pos, cell, np.full(n, 6))], 42)
    free = gm.molecule_test(v, loose, row_ptr, mo, mu.THRESHOLD)
    mean = float(free.crystal_stats[0, 1] / free.crystal_stats[0, 0])
    bound = 32 * n * EPS23 * float(v.abs().max())
    print(f"independent rows: mean |D| {mean:.3e}, 1000 x bound {1000 * bound:.3e}")
    assert mean >= 1000 * bound


def test_a_tie_keeps_the_lower_atom_and_a_coincident_pair_is_not_counted():
    """Three atoms in a line, the outer two with bit-identical U: from the middle atom the two vectors are exact negatives
    and the form is even, so the two |D| are one number and the lower atom stays.  Then the same test on positions of
    which two coincide (x is the caller's): r.r == 0 is not counted."""
    from cartnet_amd import metrics as gm
    c, v = np.array([10.0, 10.0, 10.0]), np.array([1.0, 0.75, 0.5])
    u = pu.spd_rows(3, 8)
    u[2] = u[0]
    batch, u, row_ptr = _make([(np.stack([c + v, c, c - v]), mu.cubic(20.0), np.array([6, 8, 6]))], 8, u=u)
    mo = gm.molecules(batch, row_ptr, mu.TOL, rows=3)
    assert mo.size.tolist() == [3, 3, 3] and torch.equal(mo.x[1] - mo.x[0], mo.x[2] - mo.x[1])
    res = gm.molecule_test(u, batch, row_ptr, mo)
    assert res.pairs.tolist() == [2, 2, 2] and res.worst[1].item() == 0 and float(res.delta_max[1]) > 0
    x = mo.x.clone()
    x[2] = x[0]
    res = gm.molecule_test(u, batch, row_ptr, mo._replace(x=x))
    assert res.pairs.tolist() == [1, 2, 1] and res.worst.tolist() == [1, 0, 1]


def test_argument_checks_and_no_rows():
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _make([(mu.chain(2, (3.0, 3.0, 3.0), mu.cubic(20.0))[0], mu.cubic(20.0), np.array([6, 6]))], 14)
    mo = gm.molecules(batch, row_ptr, rows=2)
    assert gm.molecule_test(u, batch, row_ptr, mo).pairs.tolist() == [1, 1]
    with pytest.raises(ValueError, match="u must be"):
        gm.molecule_test(u.double(), batch, row_ptr, mo)
    with pytest.raises(ValueError, match="does not belong"):
        gm.molecule_test(u[:1], batch, row_ptr, mo)
    with pytest.raises(ValueError, match="does not belong"):
        gm.molecule_test(u, batch, row_ptr, mo._replace(x=mo.x.float()))
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.molecule_test(u, {k: v for k, v in batch.items() if k != "ptr"}, row_ptr, mo)
    none = dict(batch, non_H_mask=torch.zeros(2, dtype=torch.bool, device="cuda:0"))
    zero = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    empty = gm.molecules(none, zero, rows=0)
    assert empty.label.tolist() == [-1, -1] and empty.crystal_counts.tolist() == [[0.0] * 5]
    assert gm.molecule_test(u[:0], none, zero, empty).crystal_stats.tolist() == [[0.0] * 4]
