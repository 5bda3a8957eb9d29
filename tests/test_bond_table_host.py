"""The bond table of ``cartnet_amd.bonds`` in numpy (``bond_table_host``) on graphs built on the host: against a brute-force
double loop on the crystals of ``molecule_utils``, its closed forms (equal tensors, isotropic tensors, a libration about
one axis, exactly rigid rows), the counts of an asymmetric graph; then the surface around it: the two entry points'
declarations and bindings, the keys of a result and ``main.py``'s refusal."""
import os
import re

import numpy as np
import pytest

import aniso_utils as au
import bond_table_utils as bu
import molecule_utils as mu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _table(pos, cell, z, rows, radius=5.0, **kw):
    from cartnet_amd.bonds import bond_table_host
    z = np.asarray(z, dtype=np.int64)
    ei, dist, dirs = au.host_graph(pos, cell, radius)
    atom_row = mu.atom_rows(z != 1)
    return bond_table_host(rows, z, ei, dist, dirs, atom_row, **kw), (ei, dist, dirs, atom_row)


def _rows(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, 3, 3))
    return (0.01 * a @ a.transpose(0, 2, 1) + 0.02 * np.eye(3)).astype(np.float32)


@pytest.mark.parametrize("k", range(4))
def test_against_a_double_loop(k):
    pos, cell, z = mu.pair_test_crystals()[k]
    got, (ei, dist, dirs, atom_row) = _table(pos, cell, z, _rows(len(z), k))
    a, b, e = bu.brute_force(z, ei, dist, atom_row)
    assert len(e) == [17, 193, 8, 4][k]                           # chains of n atoms have n - 1 bonds, the polymer n
    assert got["a"].dtype == got["b"].dtype == np.int64 and got["tls_rank"].dtype == np.int32
    assert np.array_equal(got["a"], a) and np.array_equal(got["b"], b) and (a < b).all()
    assert (np.diff(b) >= 0).all()                                                        # target order
    assert got["length"].tobytes() == dist[e].tobytes() and got["dir"].tobytes() == dirs[e].tobytes()
    assert np.array_equal(got["counts"], np.bincount(b, minlength=len(z))) and got["counts"].dtype == np.int32
    assert np.array_equal(got["unlisted"], np.bincount(a, minlength=len(z)))              # a symmetric graph
    assert got["bond_ptr"].tolist() == [0, len(e)]
    # the columns against fp64 matrix algebra: only the order of the operations differs
    U = _rows(len(z), k).astype(np.float64)
    S = 0.5 * (U + U.transpose(0, 2, 1))
    d, l = dirs[e].astype(np.float64), dist[e].astype(np.float64)
    delta = np.einsum("np,npq,nq->n", d, S[b] - S[a], d)
    wa, wb = (np.sqrt(np.trace(S[x], axis1=1, axis2=2) - np.einsum("np,npq,nq->n", d, S[x], d)) for x in (a, b))
    tiny = 1e-12 * np.abs(U).max()
    assert np.abs(got["delta"] - delta).max() <= 2.0 ** -23 * np.abs(delta).max() + tiny
    assert np.abs(got["lower"] - (l + (wb - wa) ** 2 / (2 * l))).max() <= 2.0 ** -23 * l.max()
    assert np.abs(got["upper"] - (l + (wb + wa) ** 2 / (2 * l))).max() <= 2.0 ** -23 * l.max()
    assert (got["lower"] >= got["length"]).all() and (got["upper"] > got["lower"]).all()
    assert np.isnan(got["libration"]).all() and not got["tls_rank"].any()                 # no TLS results
    s = got["crystal_stats"]
    assert s.shape == (1, 9) and s[0, :2].tolist() == [len(e), len(e)] and s[0, 5:].tolist() == [0.0] * 4
    assert s[0, 2] == pytest.approx(l.sum(), rel=1e-12) and s[0, 4] == np.abs(got["delta"]).max()


def test_a_pair_through_two_images_is_two_entries_and_hydrogens_are_none():
    pos, cell, z = bu.two_images()
    got, (ei, dist, dirs, _) = _table(pos, cell, z, _rows(2, 7), radius=2.0)
    assert got["a"].tolist() == [0, 0] and got["b"].tolist() == [1, 1] and got["unlisted"].tolist() == [2, 0]
    assert np.array_equal(got["dir"][0], -got["dir"][1]) and got["length"].tolist() == [1.375] * 2
    got, _ = _table(pos, cell, np.array([1, 1]), np.zeros((0, 3, 3), np.float32), radius=2.0)
    assert len(got["a"]) == 0 and got["crystal_stats"].tolist() == [[0.0] * 9] and got["delta"].dtype == np.float32


def test_an_asymmetric_graph_is_told_by_its_counts():
    """The chain of 5 with the edges INTO atom 1 removed, as a cap on the neighbours can do: the bond 0 - 1 is then held
    only as 1 -> 0, which is not listed, and 1 - 2 only as 1 -> 2."""
    from cartnet_amd.bonds import bond_table_host
    pos, cell, z = mu.pair_test_crystals()[3]
    ei, dist, dirs = au.host_graph(pos, cell)
    keep = ei[1] != 1
    rows = _rows(5, 3)
    got = bond_table_host(rows, z, ei[:, keep], dist[keep], dirs[keep], np.arange(5))
    assert list(zip(got["a"].tolist(), got["b"].tolist())) == [(1, 2), (2, 3), (3, 4)]
    assert got["crystal_stats"][0, :2].tolist() == [3.0, 3.0] and got["unlisted"].tolist() == [1, 0, 1, 1, 0]
    keep = ei[1] != 0
    got = bond_table_host(rows, z, ei[:, keep], dist[keep], dirs[keep], np.arange(5))
    assert got["crystal_stats"][0, :2].tolist() == [4.0, 3.0]                             # listed against unlisted


def test_equal_tensors_give_zero_and_the_apparent_length():
    pos, cell, z = mu.pair_test_crystals()[0]
    rows = np.repeat(_rows(1, 11), len(z), axis=0)
    got, _ = _table(pos, cell, z, rows)
    assert len(got["a"]) == 17 and (got["delta"] == 0.0).all() and got["delta"].tobytes() == np.zeros(17, np.float32).tobytes()
    assert got["lower"].tobytes() == got["length"].tobytes() and (got["upper"] > got["length"]).all()


def test_isotropic_tensors_give_the_bounds_at_twice_u():
    """Bonds along the axes, so ``d`` has one component 1: ``w^2 = 3u - u`` is ``2u`` without a rounding, and both bounds
    are the formula's value rounded once."""
    c = np.array([10.0, 10.0, 10.0])
    pos = np.stack([c, c + [1.5, 0, 0], c + [0, 1.375, 0], c + [0, 0, -1.5]])             # the outer three: 2 A apart
    ua, ub = np.float32(0.021), np.float32(0.047)
    rows = np.stack([np.eye(3, dtype=np.float32) * u for u in (ua, ub, ub, ub)])
    got, _ = _table(pos, mu.cubic(20.0), np.full(4, 6), rows)
    assert got["a"].tolist() == [0, 0, 0] and np.abs(got["dir"]).sum(1).tolist() == [1.0] * 3
    l = got["length"].astype(np.float64)
    assert l.tolist() == [1.5, 1.375, 1.5]
    sa, sb = np.sqrt(2.0 * np.float64(ua)), np.sqrt(2.0 * np.float64(ub))
    assert got["lower"].tobytes() == (l + (sb - sa) ** 2 / (2 * l)).astype(np.float32).tobytes()
    assert got["upper"].tobytes() == (l + (sb + sa) ** 2 / (2 * l)).astype(np.float32).tobytes()
    assert got["delta"].tobytes() == np.full(3, np.float64(ub) - np.float64(ua)).astype(np.float32).tobytes()


def test_a_libration_about_z_lengthens_what_lies_across_it():
    c = np.array([10.0, 10.0, 10.0])
    pos = np.stack([c, c + [1.5, 0, 0], c + [0, 0, 1.25]])
    w = 0.01                                                                              # rad^2
    params = np.zeros((3, 24), dtype=np.float32)
    params[:, 8] = w                                                                      # L33
    params[:, 12:] = 7.0                                                                  # S and the origin do not enter
    kw = dict(params=params, rank=np.array([20, 19, 20], dtype=np.int32))
    got, _ = _table(pos, mu.cubic(20.0), np.full(3, 6), _rows(3, 5), **kw)
    assert list(zip(got["a"].tolist(), got["b"].tolist())) == [(0, 1), (0, 2)] and got["tls_rank"].tolist() == [19, 20]
    across, along = got["libration"].astype(np.float64)
    assert abs(across - 1.5 * (1.0 + np.float64(params[0, 8]) / 2)) <= 2.0 ** -24 * 1.5 and along == 1.25
    kw["rank"] = np.array([20, 0, -1], dtype=np.int32)                                    # the rank of row b decides
    got, _ = _table(pos, mu.cubic(20.0), np.full(3, 6), _rows(3, 5), **kw)
    assert np.isnan(got["libration"]).all() and got["tls_rank"].tolist() == [0, -1]
    with pytest.raises(ValueError, match="together"):
        _table(pos, mu.cubic(20.0), np.full(3, 6), _rows(3, 5), params=params)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rigid_rows_agree_along_every_bond(seed):
    """Rows of an exactly rigid body, stored in fp32: every ``D`` is the rounding of the eighteen entries that enter."""
    pos, true = mu.chain(17, (3.0, 3.0, 3.0), mu.cubic(30.0), drift=(0.1, 0.3))
    rows = mu.rigid_body_rows(true, seed).astype(np.float32)
    got, _ = _table(pos, mu.cubic(30.0), np.full(17, 6), rows)
    bound = 18 * 2.0 ** -24 * float(np.abs(rows).max())
    worst = float(np.abs(got["delta"]).max())
    print(f"seed {seed}: largest |D| {worst:.3e}, bound {bound:.3e}")
    assert len(got["delta"]) == 16 and worst <= bound
    loose, _ = _table(pos, mu.cubic(30.0), np.full(17, 6), _rows(17, seed))
    assert float(np.abs(loose["delta"]).max()) > 100 * bound                              # independent rows are not rigid


def test_a_bad_row_gives_nan_bounds_and_is_still_listed():
    pos, cell, z = mu.pair_test_crystals()[3]
    rows = _rows(5, 9)
    rows[1] = np.nan
    rows[3] = -rows[3]                                                                    # negative definite
    got, _ = _table(pos, cell, z, rows)
    assert list(zip(got["a"].tolist(), got["b"].tolist())) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert np.isnan(got["lower"]).all() and np.isnan(got["upper"]).all()                  # every bond has a bad end
    assert np.isnan(got["delta"]).tolist() == [True, True, False, False]
    s = got["crystal_stats"][0]
    assert s[0] == 4 and s[8] == 4 and np.isnan(s[3]) and np.isnan(s[4])                  # the largest |D| keeps the NaN


def test_the_entry_points_are_declared_bound_and_built():
    from cartnet_amd import lib
    from cartnet_amd.build import EXTRA_FLAGS, SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    block = hdr[:hdr.index("int cartnet_bond_table_count(")].rsplit("/*", 1)[1]
    assert "Busing & Levy" in block and "cartnet_adp_bond_table " in block and "libration" in block
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, count in (("cartnet_bond_table_count", 14), ("cartnet_adp_bond_table", 31)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == count == len(lib.PROTOTYPES[name][1]), name
        assert "struct" not in m.group(1)                                                 # plain arguments
    assert "bond_table_ops.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "cartnet_amd", "csrc", "bond_table_ops.hip"))
    assert "-ffp-contract=off" not in EXTRA_FLAGS.get("bond_table_ops.hip", []) + EXTRA_FLAGS.get("bond_ops.hip", [])
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()                      # no struct changed
    count, fill = lib.load().cartnet_bond_table_count, lib.load().cartnet_adp_bond_table
    assert count(*[None] * 6, 97, 0.4, 0, 5, 50, None, None, None) == 0                   # no atoms
    assert count(*[None] * 6, 97, 0.4, 10, 5, 50, None, None, None) == 1                  # null pointers: an error, no fault
    assert count(*[None] * 6, 97, float("nan"), 10, 5, 50, None, None, None) == 1
    nul, out = [None] * 9, [None] * 11
    assert fill(*nul, 97, 0.4, *[None] * 4, 0, 10, 5, 50, 3, *out) == 0                   # no crystals
    assert fill(*nul, 97, 0.4, *[None] * 4, 2, 0, 5, 50, 3, *out) == 0                    # no atoms
    assert fill(*nul, 97, 0.4, *[None] * 4, 2, 10, 5, 50, 3, *out) == 1
    assert fill(*nul, 97, 0.4, *[None] * 4, 2, 10, 5, 50, -1, *out) == 1


def test_the_keys_of_a_result():
    from cartnet_amd import predict as p
    from cartnet_amd.predict import Analyses, result_keys
    keys = ("bonds_a", "bonds_b", "bonds_dir", "bonds_length", "bonds_delta", "bonds_lower", "bonds_upper",
            "bonds_libration", "bonds_tls_rank", "bonds_stats")
    assert p.BT_KEYS == keys and list(p.BT_SPLIT.items()) == [(k, "bond") for k in keys[:-1]] + [("bonds_stats", "crystal")]
    names = list(p.GROUPS)
    assert names.index("bond_table") == names.index("aniso_h_symmetry") + 1 == names.index("series") - 1
    every = Analyses(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
                     aniso_h=(0.005, 0.020))
    for a, sym, K in ((Analyses(), False, 1), (every, True, 2), (every, False, 1)):
        off = result_keys(a, sym, K)
        assert result_keys(a, sym, K, None) == off and not [k for k in off if k.startswith("bonds_")]
        assert result_keys(a, sym, K, 0.4) == off + keys                                  # last, in the stated order
    assert p.result_keys(Analyses(), False, 1) == p.KEYS
    figures = p.STATISTICS["bonds_stats"][1]([12.0, 10.0, 18.0, 0.02, 0.0, 4.0, 0.008, 0.0, 1.0], [0.0] * 7 + [0.003, 0.0])
    assert figures == {"bonds_listed": 12, "bonds_unlisted": 10, "bond_length_mean": 1.5, "bond_libration_bonds": 4,
                       "bond_libration_mean": 0.002, "bond_libration_max": 0.003, "bond_bounds_nan": 1}


def test_the_flag_is_refused_before_the_device_is_touched(monkeypatch):
    import main as entry

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    with pytest.raises(SystemExit, match="--bond_table serves --predict only"):
        entry.main(["--bond_table"])
    with pytest.raises(SystemExit, match="--bond_table serves --predict only"):
        entry.main(["--bond_table", "--inference", "--rigid_molecule", "--tls_fit"])
    args = entry.build_parser().parse_args([])
    assert args.bond_table is False and entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None}
    args = entry.build_parser().parse_args(["--bond_table", "--bond_tolerance", "0.3"])
    assert entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None, "bond_table": 0.3}
    assert entry.analysis_options(args, inference=True) == {"rigid_bond": None}
