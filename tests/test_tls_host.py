"""The TLS rule of ``cartnet_amd.bonds`` in numpy (``tls_fit_host`` and what it is made of): the rank of the normal matrix
for the shapes that matter, each with its margin around the threshold; recovery of known T, L and S from fp32 rows; the
properties a crystallographer relies on (tr S = 0, independence of the root atom, covariance under rotation, an exact
rigid body leaves no residual); the row layout of ``tls_fit_host``; and ``main.py``'s refusal of the flag alone."""
import numpy as np
import pytest

import molecule_utils as mu
import tls_utils as tu

CASES = [("four on a helix", lambda: tu.helix(4), 18),
         ("four at random", lambda: np.random.default_rng(3).standard_normal((4, 3)), 18),
         ("planar chain of 5", lambda: tu.planar_chain(5), 19), ("planar chain of 8", lambda: tu.planar_chain(8), 19),
         ("planar chain of 17", lambda: tu.planar_chain(17), 19),
         ("six on a flat circle", lambda: tu.flat_circle((5.0, 5.0, 5.0)), 19),
         ("five collinear", lambda: tu.line(5, (3.0, 3.0, 3.0)), 14),
         ("puckered ring", lambda: mu.ring((5.0, 5.0, 5.0)), 20)] + \
        [(f"helix of {n}", (lambda n=n: tu.helix(n)), 20) for n in (5, 6, 7, 8, 17)]

# the worst relative errors (max |fit - known| / max |known|) over the seeds 0 ... 7 and the helices of 5 and 17 atoms,
# measured with this file: T 2.9e-8, L 1.8e-5, S 9.2e-6; the bounds are ten times that
RECOVERY = {"T": 2.9e-7, "L": 1.8e-4, "S": 9.2e-5}


@pytest.mark.parametrize("name,make,rank", CASES, ids=[c[0] for c in CASES])
def test_rank_table(name, make, rank):
    from cartnet_amd.bonds import TLS_MAX_SWEEPS, tls_solve_host
    pos = make()
    fit = tls_solve_host(pos, np.zeros((len(pos), 3, 3)))
    ev = fit["eigenvalues"]
    print(f"{name}: rank {fit['rank']}, {fit['sweeps']} sweeps, smallest kept {ev[ev > 1e-10].min():.2e}, "
          f"largest dropped {np.abs(ev[ev <= 1e-10]).max() if (ev <= 1e-10).any() else 0.0:.2e}")
    assert fit["rank"] == rank
    assert not ((ev > 1e-13) & (ev < 1e-7)).any()                             # the margin around TLS_RANK_EPS
    assert 0 < fit["sweeps"] <= TLS_MAX_SWEEPS // 2                           # far from the bound
    want = np.linalg.eigvalsh(_normal(pos))
    assert np.abs(ev - want / want[-1]).max() <= 1e-13                        # the Jacobi routine against LAPACK


def _normal(pos):
    from cartnet_amd.bonds import tls_design
    r = pos - pos.mean(axis=0)
    J = tls_design(r / np.sqrt((r * r).sum(1).mean()))
    return np.einsum("ioa,iob->ab", J, J)


def test_the_design_matrix_is_the_model():
    """``J p`` is the weighted vector of ``tls_model`` for random parameters, and S's trace never enters."""
    from cartnet_amd.bonds import TLS_PAIRS, TLS_S_ENTRIES, tls_design, tls_model
    rng = np.random.default_rng(11)
    r, p = rng.standard_normal((7, 3)), rng.standard_normal(20)

    def full(v):
        return np.array([[v[0], v[5], v[4]], [v[5], v[1], v[3]], [v[4], v[3], v[2]]])
    S = np.zeros((3, 3))
    for (a, b), v in zip(TLS_S_ENTRIES, p[12:]):
        S[a, b] = v
    S[2, 2] = -(S[0, 0] + S[1, 1])
    U = tls_model(r, full(p[:6]), full(p[6:12]), S)
    w = [1.0] * 3 + [np.sqrt(2.0)] * 3
    want = np.stack([w[o] * U[:, a, b] for o, (a, b) in enumerate(TLS_PAIRS)], axis=1)
    assert np.abs(tls_design(r) @ p - want).max() <= 1e-13
    assert np.abs(tls_model(r, full(p[:6]), full(p[6:12]), S + 0.37 * np.eye(3)) - U).max() <= 1e-13


def test_jacobi_against_lapack_and_its_bound():
    from cartnet_amd.bonds import jacobi_eigh
    rng = np.random.default_rng(2)
    for n in (3, 4, 7, 20):
        a = rng.standard_normal((n, n))
        a = a @ a.T
        w, V, sweeps = jacobi_eigh(a)
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(a)).max() <= 1e-13 * np.abs(w).max() and 0 < sweeps <= 12
        assert np.abs(a @ V - V * w).max() <= 1e-13 * np.abs(w).max() and np.abs(V.T @ V - np.eye(n)).max() <= 1e-14
    w, V, sweeps = jacobi_eigh(np.diag([3.0, 1.0, 2.0]))
    assert w.tolist() == [3.0, 1.0, 2.0] and sweeps == 0 and np.array_equal(V, np.eye(3))
    w, _, sweeps = jacobi_eigh(a, max_sweeps=1)                               # the bound is hard
    assert w is None and sweeps == 1
    w, _, _ = jacobi_eigh(np.full((3, 3), np.nan))
    assert w is None


@pytest.mark.parametrize("n", [5, 17])
def test_recovery_of_known_tensors_from_fp32_rows(n):
    from cartnet_amd.bonds import tls_solve_host
    pos = tu.helix(n)
    worst = dict.fromkeys(RECOVERY, 0.0)
    for seed in range(8):
        T, L, S = tu.known_tls(seed)
        fit = tls_solve_host(pos, tu.rigid_rows(pos, seed).astype(np.float32))
        assert fit["rank"] == 20
        for key, known in (("T", T), ("L", L), ("S", S)):
            worst[key] = max(worst[key], tu.rel(fit[key], known))
        assert np.abs(fit["origin"] - pos.mean(axis=0)).max() <= 1e-12
    print(f"helix of {n}: worst relative errors " + ", ".join(f"{k} {v:.2e} (bound {RECOVERY[k]:.1e})" for k, v in worst.items()))
    assert all(worst[k] <= RECOVERY[k] for k in RECOVERY)


def test_properties():
    from cartnet_amd.bonds import tls_solve_host
    pos = tu.helix(17, (2.0, 3.0, 4.0))
    U = tu.rigid_rows(pos, 21, tu.NOISE)
    fit = tls_solve_host(pos, U)
    assert fit["rank"] == 20 and fit["rfac"] > 1e-3 and fit["resid"].min() > 0
    assert abs(np.trace(fit["S"])) <= 4 * 2.0 ** -52 * np.abs(fit["S"]).max()
    assert fit["T_principal"].tolist() == sorted(fit["T_principal"].tolist())
    assert np.abs(fit["T_principal"] - np.linalg.eigvalsh(fit["T"])).max() <= 1e-15
    assert np.abs(fit["L_principal"] - np.linalg.eigvalsh(fit["L"])).max() <= 1e-17
    # against LAPACK's least squares on the same design matrix
    from cartnet_amd.bonds import TLS_PAIRS, tls_design
    r = pos - pos.mean(axis=0)
    rho = np.sqrt((r * r).sum(1).mean())
    sym = 0.5 * (U + U.transpose(0, 2, 1))
    w = [1.0] * 3 + [np.sqrt(2.0)] * 3
    y = np.stack([w[o] * sym[:, a, b] for o, (a, b) in enumerate(TLS_PAIRS)], axis=1)
    p = np.linalg.lstsq(tls_design(r / rho).reshape(-1, 20), y.reshape(-1), rcond=None)[0]
    assert tu.rel([fit["T"][a, b] for a, b in TLS_PAIRS], p[:6]) <= 1e-10
    assert tu.rel([fit["L"][a, b] * rho * rho for a, b in TLS_PAIRS], p[6:12]) <= 1e-9
    # another root atom and another atom order: x moves by a constant, the fit does not
    order = np.random.default_rng(4).permutation(17)
    moved = tls_solve_host((pos - pos[9])[order], U[order])
    assert np.abs(moved["u_tls"] - fit["u_tls"][order]).max() <= 1e-9 * np.abs(U).max()
    assert np.abs(moved["resid"] - fit["resid"][order]).max() <= 1e-9 * np.abs(U).max()
    assert tu.rel(moved["T"], fit["T"]) <= 1e-9 and tu.rel(moved["L"], fit["L"]) <= 1e-9 and tu.rel(moved["S"], fit["S"]) <= 1e-8
    assert np.abs(moved["origin"] - (fit["origin"] - pos[9])).max() <= 1e-12
    # rotating positions and tensors rotates T, L, S and u_tls
    R = tu.rotation(8)
    turned = tls_solve_host(pos @ R.T, R @ U @ R.T)
    for key in ("T", "L", "S"):
        assert tu.rel(turned[key], R @ fit[key] @ R.T) <= 1e-8, key
    assert np.abs(turned["u_tls"] - R @ fit["u_tls"] @ R.T).max() <= 1e-9 * np.abs(U).max()
    assert np.abs(turned["resid"] - fit["resid"]).max() <= 1e-9 * np.abs(U).max() and abs(turned["rfac"] - fit["rfac"]) <= 1e-9


@pytest.mark.parametrize("shape", ["helix", "planar", "line"])
def test_an_exact_rigid_body_leaves_no_residual(shape):
    """fp32 rows of an exact rigid body: the residual is the rounding of the rows, whatever the rank -- the fitted U is
    unique even where T, L and S are not."""
    from cartnet_amd.bonds import tls_solve_host
    pos = {"helix": tu.helix(17), "planar": tu.planar_chain(8), "line": tu.line(5, (0.0, 0.0, 0.0))}[shape]
    U = tu.rigid_rows(pos, 33).astype(np.float32)
    fit = tls_solve_host(pos, U)
    bound = tu.EPS22 * float(np.abs(U).max())
    print(f"{shape}: rank {fit['rank']}, largest resid {fit['resid'].max():.3e}, bound {bound:.3e}, R {fit['rfac']:.3e}")
    assert fit["rank"] == {"helix": 20, "planar": 19, "line": 14}[shape]
    assert fit["resid"].max() <= bound and abs(np.trace(fit["S"])) <= 1e-18


def test_rows_of_tls_fit_host():
    """Two crystals: a helix of 6 interleaved with a helix of 4 (below the minimum), then a helix of 5 with status 1 (not
    fitted), a point-like 'molecule' of 5 (rho == 0) and a planar chain of 5."""
    from cartnet_amd.bonds import tls_fit_host, tls_solve_host
    a, b = tu.helix(6), tu.helix(4, (0.0, 9.0, 9.0))
    first = np.empty((10, 3))
    ia, ib = np.array([0, 2, 3, 5, 7, 9]), np.array([1, 4, 6, 8])
    first[ia], first[ib] = a - a[0], b - b[0]
    label = np.empty(25, dtype=np.int64)
    label[ia], label[ib] = 0, 1
    second = [tu.helix(5), np.zeros((5, 3)), tu.planar_chain(5)]
    x = np.concatenate([first] + [m - m[0] for m in second])
    for k in range(3):
        label[10 + 5 * k:15 + 5 * k] = 10 + 5 * k
    size = np.array([6, 4, 6, 6, 4, 6, 4, 6, 4, 6] + [5] * 15, dtype=np.int32)
    status = np.array([0] * 10 + [1] * 5 + [0] * 10, dtype=np.int32)
    u = np.concatenate([tu.rigid_rows(x[:10], 1, tu.NOISE), tu.rigid_rows(x[10:], 2, tu.NOISE)]).astype(np.float32)
    got = tls_fit_host(u, label, x, np.arange(25), status, size, ptr=[0, 10, 25])
    assert sorted(got["molecules"]) == [0, 20] and got["rank"].tolist() == [20 if i in ia else 0 for i in range(10)] + [0] * 10 + [19] * 5
    neutral = got["rank"] == 0
    assert np.isnan(got["u_tls"][neutral]).all() and np.isnan(got["params"][neutral]).all() and np.isnan(got["eig"][neutral]).all()
    assert (got["resid"][neutral] == 0).all() and (got["rfac"][neutral] == 0).all()
    assert not np.isnan(got["u_tls"][~neutral]).any() and (got["resid"][~neutral] > 0).all()
    one = tls_solve_host(x[ia], u[ia])
    assert np.array_equal(got["u_tls"][ia], one["u_tls"].astype(np.float32))
    want = np.concatenate([[one["T"][p, q] for p, q in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))],
                           [one["L"][p, q] for p, q in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))],
                           one["S"].reshape(-1), x[ia].mean(axis=0)]).astype(np.float32)
    assert all(np.array_equal(got["params"][i], want) for i in ia)            # replicated on every row
    assert np.array_equal(got["eig"][0], np.concatenate([one["T_principal"], one["L_principal"]]).astype(np.float32))
    stats = got["crystal_stats"]
    assert stats.shape == (2, 6) and stats[:, :2].tolist() == [[1.0, 0.0], [1.0, 1.0]]
    for g, rows in enumerate((ia, np.arange(20, 25))):
        r = got["resid"][rows].astype(np.float64)
        s = 0.5 * (u[rows].astype(np.float64) + u[rows].astype(np.float64).transpose(0, 2, 1))
        assert stats[g, 3] == pytest.approx((r * r).sum(), rel=1e-12) and stats[g, 4] == pytest.approx((s * s).sum(), rel=1e-12)
        assert stats[g, 5] == r.max()
        assert got["rfac"][rows[0]] == pytest.approx(np.sqrt(stats[g, 3] / stats[g, 4]), rel=1e-5)


def test_the_flag_alone_is_refused():
    import main as entry
    with pytest.raises(SystemExit, match="--rigid_molecule"):
        entry.main(["--tls_fit"])
    with pytest.raises(SystemExit, match="--rigid_molecule"):
        entry.main(["--predict", "--tls_fit", "--predict_input", "none.cnshard", "--checkpoint_path", "none.ckpt"])
    args = entry.build_parser().parse_args(["--rigid_molecule", "--tls_fit"])
    assert entry.analysis_options(args, inference=True) == {"rigid_bond": None, "rigid_molecule": (0.4, 1e-3), "tls_fit": True}
    assert entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None, "rigid_molecule": (0.4, 1e-3), "tls_fit": True}
    assert "tls_fit" not in entry.analysis_options(entry.build_parser().parse_args(["--rigid_molecule"]))
    assert entry.build_parser().parse_args([]).tls_fit is False
