"""The symmetry expansion on the GPU (csrc/symmetry_ops.hip) against its host statement, the reference's duplicate
mask, fp64 numpy and the symmetry of the result itself.  One batch of nine crystals, expanded once."""
import os

import numpy as np
import pytest
import torch

import cif_utils as cu
from cartnet_amd import cif, symmetry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INT_KEYS = ("z", "atom_ptr", "y_ptr", "non_h_mask")
ROW_KEYS = ("row_asym", "row_op", "orbit_row")


class Expanded:
    def __init__(self):
        self.crystals = cif.read_cif(cu.batch_text())
        self.arrays, self.sym = symmetry.expand(self.crystals, DEV, labeled=True)
        self.host, self.host_rows = symmetry.expand_host(self.crystals, labeled=True)
        self.G = len(self.crystals)
        self.cells = [cu.cell_reference(*cu.CRYSTALS[k]["cell"]) for k in cu.BATCH]
        self.ops = [cu.op_arrays(cu.CRYSTALS[k]["ops"] or [cu.IDENTITY]) for k in cu.BATCH]
        self.rows = {k: getattr(self.sym, k).cpu().numpy() for k in ROW_KEYS}
        self.orb_ptr = self.sym.orb_ptr.cpu().numpy()
        # the file's U of the non-hydrogen asymmetric atoms, per crystal
        self.u_file = [np.array([a[5] for a in cu.CRYSTALS[k]["atoms"] if a[5] is not None]) for k in cu.BATCH]

    def atoms(self, g):
        p = self.arrays["atom_ptr"]
        return slice(int(p[g]), int(p[g + 1]))

    def heavy(self, g):
        p = self.arrays["y_ptr"]
        return slice(int(p[g]), int(p[g + 1]))

    def frac(self, g):
        """fp64 fractions of the kept atoms of crystal g, from pos."""
        return self.arrays["pos"][self.atoms(g)].astype(np.float64) @ np.linalg.inv(self.cells[g])

    def orbit(self, g, site):
        m = len(self.ops[g][0])
        o = int(self.orb_ptr[g]) + site * m
        return self.rows["orbit_row"][o:o + m]

    def average(self, pred):
        """site_average over all crystals in one batch: (u [H,6], spread [H]) as numpy, and the per-crystal offsets."""
        u, spread = symmetry.site_average(pred, torch.from_numpy(self.arrays["y_ptr"]).to(DEV), list(range(self.G)), self.sym)
        return u.cpu().numpy(), spread.cpu().numpy(), np.concatenate([[0], np.cumsum(self.sym.site_count)])

    def reference_average(self, pred):
        out = []
        for g in range(self.G):
            p = pred[self.heavy(g)]
            for site in range(int(self.sym.site_count[g])):
                out.append(cu.site_average_reference(p, self.orbit(g, site), self.ops[g][0], self.cells[g]))
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


@pytest.fixture(scope="module")
def ex():
    return Expanded()


@pytest.fixture(scope="module")
def field(ex):
    """A random field without any symmetry, [Y,3,3] fp32 (not even symmetric matrices), and its site averages."""
    gen = torch.Generator().manual_seed(11)
    pred = (torch.randn(int(ex.arrays["y_ptr"][-1]), 3, 3, generator=gen) * 0.02).to(DEV)
    return pred, ex.average(pred), ex.reference_average(pred.cpu().numpy())


def test_kept_mask_equals_the_reference_bit_for_bit():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "cif_expand.npz"))
    n = int(golden["n_sets"])
    crystals = [cu.crystal_from_coords(f"set{i}", golden[f"coord{i}"]) for i in range(n)]
    arrays, _ = symmetry.expand(crystals, DEV, labeled=False)
    for i in range(n):
        z = arrays["z"][arrays["atom_ptr"][i]:arrays["atom_ptr"][i + 1]]
        assert np.array_equal(cu.kept_mask(z, len(golden[f"coord{i}"])), golden[f"keep{i}"]), i
        assert list(z) == sorted(z)


def test_expansion_equals_the_host_statement(ex):
    for k in INT_KEYS:
        assert ex.arrays[k].dtype == ex.host[k].dtype and np.array_equal(ex.arrays[k], ex.host[k]), k
    for k in ROW_KEYS:
        assert np.array_equal(ex.rows[k], ex.host_rows[k]), k
    assert np.array_equal(ex.orb_ptr, ex.host_rows["orb_ptr"])
    assert np.array_equal(ex.arrays["cell"], ex.host["cell"]) and ex.arrays["cell"].dtype == np.float32
    assert np.array_equal(ex.arrays["temperature"], ex.host["temperature"])
    assert np.array_equal(ex.arrays["non_h_mask"], (ex.arrays["z"] != 1).astype(np.uint8))
    for g in range(ex.G):                                              # one rounding of an fp64 result
        got, want = ex.arrays["pos"][ex.atoms(g)], ex.host["pos"][ex.atoms(g)]
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max(), g
    assert np.diff(ex.arrays["atom_ptr"]).tolist() == [cu.ATOMS[k][0] for k in cu.BATCH]
    assert np.diff(ex.arrays["y_ptr"]).tolist() == [cu.ATOMS[k][1] for k in cu.BATCH]
    assert (cu.ATOMS["a"][0], cu.ATOMS["b"][0], cu.ATOMS["d"][0]) == (5, 22, 8)
    # the asymmetric unit comes first, under the identity
    for g, key in enumerate(cu.BATCH):
        n = len(cu.CRYSTALS[key]["atoms"])
        assert ex.arrays["z"][ex.atoms(g)][:n].tolist() == ex.crystals[g].z
        h = ex.heavy(g)
        k = len(ex.u_file[g])
        assert ex.rows["row_op"][h][:k].tolist() == [0] * k
        assert ex.rows["row_asym"][h][:k].tolist() == [i for i, z in enumerate(ex.crystals[g].z) if z != 1]


def test_every_operator_maps_the_atoms_onto_themselves(ex):
    for g in range(ex.G):
        f, z = ex.frac(g), ex.arrays["z"][ex.atoms(g)]
        W, w = ex.ops[g]
        for s in range(len(W)):
            image = f @ W[s].T.astype(np.float64) + w[s]
            d = image[:, None, :] - f[None, :, :]
            d -= np.rint(d)
            dist = np.linalg.norm(d, axis=-1)
            j = dist.argmin(axis=1)
            assert (dist[np.arange(len(f)), j] < 1e-4).all(), (g, s)
            assert np.array_equal(z[j], z), (g, s)
            assert sorted(j.tolist()) == list(range(len(f))), (g, s)


def test_targets_against_fp64_numpy(ex):
    for g in range(ex.G):
        h = ex.heavy(g)
        a, s = ex.rows["row_asym"][h], ex.rows["row_op"][h]
        site = {atom: k for k, atom in enumerate(i for i, z in enumerate(ex.crystals[g].z) if z != 1)}
        u = cu.full(ex.u_file[g][[site[int(i)] for i in a]])
        want = cu.cart_from_cif(u, ex.cells[g], ex.ops[g][0][s])
        got = ex.arrays["y"][h].reshape(-1, 3, 3).astype(np.float64)
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max(), g


def test_targets_are_covariant(ex):
    """R_s y_i R_s^T = y_s(i) with R_s = A W A^-1 (A = cell^T): both sides carry one fp32 rounding of y, the left one
    multiplied by sum |R| |R| <= 3 (rows of a rotation): 2^-24 (3 + 1) max|y| = 2^-22 max|y|; bound 2^-21 max|y|."""
    for g in range(ex.G):
        f, y = ex.frac(g), ex.arrays["y"][ex.heavy(g)].reshape(-1, 3, 3).astype(np.float64)
        heavy = np.nonzero(ex.arrays["z"][ex.atoms(g)] != 1)[0]
        A = ex.cells[g].T
        W, w = ex.ops[g]
        for s in range(len(W)):
            R = A @ W[s] @ np.linalg.inv(A)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-4          # a rotation, up to the printed digits of the cell
            image = f[heavy] @ W[s].T.astype(np.float64) + w[s]
            d = image[:, None, :] - f[heavy][None, :, :]
            d -= np.rint(d)
            j = np.linalg.norm(d, axis=-1).argmin(axis=1)
            assert np.abs(R @ y @ R.T - y[j]).max() <= 2.0 ** -21 * np.abs(y).max(), (g, s)


def test_targets_round_trip_to_the_files_u(ex):
    for g in range(ex.G):
        k = len(ex.u_file[g])
        y = ex.arrays["y"][ex.heavy(g)][:k].reshape(-1, 3, 3)          # the identity's rows
        got = cu.six(cu.cif_from_cart(y, ex.cells[g]))
        bound = cu.round_trip_bound(ex.u_file[g], ex.cells[g])
        print(g, cu.BATCH[g], "round trip: worst error / bound", (np.abs(got - ex.u_file[g]) / bound).max())
        assert (np.abs(got - ex.u_file[g]) <= bound).all(), g


def test_site_average_of_the_targets_returns_the_files_u(ex):
    pred = torch.from_numpy(ex.arrays["y"]).view(-1, 3, 3).to(DEV)
    u, spread, ptr = ex.average(pred)
    for g in range(ex.G):
        got, sp = u[ptr[g]:ptr[g + 1]], spread[ptr[g]:ptr[g + 1]]
        bound = cu.round_trip_bound(ex.u_file[g], ex.cells[g])
        print(g, cu.BATCH[g], "site average of the targets: worst error / bound", (np.abs(got - ex.u_file[g]) / bound).max(),
              "spread / bound", (sp / bound.max(axis=1)).max())
        assert (np.abs(got - ex.u_file[g]) <= bound).all(), g
        assert (sp <= bound.max(axis=1)).all(), g


def test_site_average_of_a_random_field_against_fp64_numpy(ex, field):
    """2^-23 of the componentwise factor of the round trip, plus the fp64 floor of ``cu.fp64_floor``: a component that
    the site symmetry makes zero (the off-diagonal ones in Fm-3m, U13 and U23 on the 3-fold axis) is the sum of members
    that cancel, so it comes out as fp64 round-off of the members' size on either side, not as zero."""
    _, (u, spread, ptr), (u_ref, spread_ref) = field
    assert u.shape == u_ref.shape == (int(ex.sym.site_count.sum()), 6)
    for g in range(ex.G):
        s = slice(int(ptr[g]), int(ptr[g + 1]))
        bound = cu.round_trip_bound(u_ref[s], ex.cells[g]) + cu.fp64_floor(u_ref[s], spread_ref[s])
        assert (np.abs(u[s] - u_ref[s]) <= bound).all(), g
        assert np.abs(spread[s] - spread_ref[s]).max() <= 2.0 ** -23 * spread_ref[s].max(), g
    assert spread_ref.max() > 1e-3                                      # the field really has no symmetry


def test_special_positions_obey_their_site_symmetry(ex, field):
    """W beta W^T = beta for the stabiliser, to the round-trip bound of the stored fp32 values plus the fp64 floor (the
    components that the symmetry makes zero are stored as fp64 round-off, see above)."""
    _, (u, spread, ptr), _ = field
    seen = 0
    for g, key in enumerate(cu.BATCH):
        for crystal, atom in cu.SPECIAL:
            if crystal != key:
                continue
            orbit = ex.orbit(g, atom)                                    # the special atoms are the first, not hydrogen
            stabiliser = np.nonzero(orbit == orbit[0])[0]
            assert len(stabiliser) == {"b": 2, "c": 3}[key] and len(set(orbit.tolist())) * len(stabiliser) == len(orbit)
            n = cu.reciprocal_norms(ex.cells[g])
            u6 = u[ptr[g] + atom].astype(np.float64)
            beta = cu.full(u6) * n[:, None] * n[None, :]
            bound = cu.round_trip_bound(u6, ex.cells[g]) + cu.fp64_floor(u6, spread[ptr[g] + atom])
            for s in stabiliser:
                W = ex.ops[g][0][s].astype(np.float64)
                moved = cu.six((W @ beta @ W.T) / (n[:, None] * n[None, :]))
                assert (np.abs(moved - u6) <= bound).all(), (g, s)
            seen += 1
    assert seen == 3                                                    # (b) twice, (c) once


def test_p1_site_average_is_adp_export(ex, field):
    from cartnet_amd.metrics import adp_export
    pred, (u, _, ptr), _ = field
    checked = 0
    for g, key in enumerate(cu.BATCH):
        if len(ex.ops[g][0]) != 1:
            continue
        rows = pred[ex.heavy(g)].contiguous()
        row_ptr = torch.tensor([0, rows.shape[0]], dtype=torch.int64, device=DEV)
        cell = torch.from_numpy(ex.arrays["cell"][g]).view(1, 3, 3).to(DEV)
        want = adp_export(rows, row_ptr, cell).u_cif.cpu().numpy()
        got = u[ptr[g]:ptr[g + 1]]
        print(g, key, "P1 against adp_export: worst error / bound", np.abs(got - want).max() / (2.0 ** -22 * np.abs(want).max()))
        assert np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max(), g
        checked += 1
    assert checked == 3                                                 # (e) twice, (a) once


def test_two_runs_give_identical_bytes(ex):
    arrays, sym = symmetry.expand(ex.crystals, DEV, labeled=True)
    assert sorted(arrays) == sorted(ex.arrays)
    for k, v in arrays.items():
        assert v.tobytes() == ex.arrays[k].tobytes(), k
    for k in ROW_KEYS:
        assert getattr(sym, k).cpu().numpy().tobytes() == ex.rows[k].tobytes(), k
    pred = torch.from_numpy(ex.arrays["y"]).view(-1, 3, 3).to(DEV)
    (u1, s1, _), (u2, s2, _) = ex.average(pred), ex.average(pred)
    assert u1.tobytes() == u2.tobytes() and s1.tobytes() == s2.tobytes()


def test_a_subset_of_the_crystals_in_any_order(ex, field):
    pred, (u, spread, ptr), _ = field
    sel = [3, 1, 5]
    rp = ex.arrays["y_ptr"]
    rows = torch.cat([pred[int(rp[g]):int(rp[g + 1])] for g in sel])
    row_ptr = torch.tensor(np.concatenate([[0], np.cumsum([rp[g + 1] - rp[g] for g in sel])]), dtype=torch.int64, device=DEV)
    got_u, got_s = symmetry.site_average(rows, row_ptr, sel, ex.sym)
    assert got_u.cpu().numpy().tobytes() == np.concatenate([u[ptr[g]:ptr[g + 1]] for g in sel]).tobytes()
    assert got_s.cpu().numpy().tobytes() == np.concatenate([spread[ptr[g]:ptr[g + 1]] for g in sel]).tobytes()


def test_ambiguous_atoms_and_a_singular_cell_are_refused_by_name(ex):
    for key in ("ambiguous", "singular"):
        crystals = ex.crystals[:2] + cif.read_cif(cu.BAD[key]) + ex.crystals[2:4]
        with pytest.raises(ValueError, match=f"crystal {key}:"):
            symmetry.expand(crystals, DEV, labeled=True)
    with pytest.raises(ValueError, match="crystal isotropic_carbon:"):
        symmetry.expand(cif.read_cif(cu.BAD["isotropic_carbon"]), DEV, labeled=True)
