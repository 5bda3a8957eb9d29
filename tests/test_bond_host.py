"""The rigid-bond test on the host: the radii table, the bond rule in numpy fp32, the flags, the entry point's declaration
and binding and its returns that need no launch (no GPU)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radii_table_is_the_one_written_down():
    from cartnet_amd.bonds import BOND_TOLERANCE, COVALENT_RADII, RIGID_BOND_THRESHOLD
    assert isinstance(COVALENT_RADII, tuple) and len(COVALENT_RADII) == 97 and COVALENT_RADII[0] == 0.0
    want = {1: 0.31, 6: 0.76, 7: 0.71, 8: 0.66, 16: 1.05, 17: 1.02, 26: 1.32, 53: 1.39, 96: 1.69}     # H C N O S Cl Fe I Cm
    assert {z: COVALENT_RADII[z] for z in want} == want
    assert all(0.2 < r < 2.7 for r in COVALENT_RADII[1:])
    assert (BOND_TOLERANCE, RIGID_BOND_THRESHOLD) == (0.4, 1e-3)


def test_parser_defaults_and_old_defaults_stay():
    import main as entry
    p = entry.build_parser()
    d = p.parse_args([])
    assert (d.rigid_bond, d.bond_tolerance, d.rigid_bond_threshold) == (False, 0.4, 1e-3)
    assert (d.rotations, d.eval_batch, d.predict, d.inference, d.predict_output) == (1, 1, False, False, "./predictions.pkl")
    a = p.parse_args(["--rigid_bond", "--bond_tolerance", "0.25", "--rigid_bond_threshold", "5e-4"])
    assert (a.rigid_bond, a.bond_tolerance, a.rigid_bond_threshold) == (True, 0.25, 5e-4)
    from cartnet_amd.predict import BOND_KEYS, KEYS
    assert BOND_KEYS == ("bond_count", "bond_delta_mean", "bond_delta_max", "bond_worst", "bond_over", "bond_ueq_ratio",
                         "bond_stats")
    assert not set(BOND_KEYS) & set(KEYS)


def test_entry_point_is_declared_bound_and_built():
    from cartnet_amd import lib
    from cartnet_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "Hirshfeld" in hdr and "main.py:47-49" in hdr                      # the reference-site comment of its neighbours
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_bond_test\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 24 == len(lib.PROTOTYPES["cartnet_adp_bond_test"][1])
    assert "struct" not in m.group(1)                                         # plain arguments
    assert "bond_ops.hip" in SOURCES
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed


def test_no_launch_and_refusal_returns():
    from cartnet_amd import lib
    l = lib.load()
    f = l.cartnet_adp_bond_test
    nul = [None] * 9
    out = [None] * 8
    assert f(*nul, 97, 0.4, 1e-3, 4, 10, 0, 50, *out) == 0                    # no rows
    assert f(*nul, 97, 0.4, 1e-3, 0, 10, 5, 50, *out) == 0                    # no crystals
    assert f(*nul, 97, 0.4, 1e-3, 4, 0, 5, 50, *out) == 0                     # no atoms
    for bad in ((-1, 10, 5, 50), (4, -1, 5, 50), (4, 10, -1, 50), (4, 10, 5, -1)):
        assert f(*nul, 97, 0.4, 1e-3, *bad, *out) != 0
        assert b"bad sizes" in l.cartnet_last_error()
    assert f(*nul, 97, float("nan"), 1e-3, 4, 10, 5, 50, *out) != 0
    assert b"must be numbers" in l.cartnet_last_error()
    assert f(*nul, 97, 0.4, 1e-3, 4, 10, 5, 50, *out) != 0                    # before any launch
    assert b"null pointer" in l.cartnet_last_error()


def test_bond_rule_in_numpy_fp32_on_a_hand_checked_pair():
    """C-C at 1.54 A against (0.76 + 0.76) + 0.4 = 1.92 A: a bond; C...C at 2.40 A: none; either with a hydrogen end, an
    atom's own image, Z = 0 or a Z beyond the table: none."""
    from cartnet_amd.bonds import COVALENT_RADII, is_bond
    r = np.float32(COVALENT_RADII[6])
    limit = (r + r) + np.float32(0.4)
    assert limit.dtype == np.float32 and abs(float(limit) - 1.92) < 1e-6
    assert np.float32(1.54) <= limit < np.float32(2.40)
    got = is_bond(np.float32([1.54, 2.40, 1.54, 1.54, 1.54, 1.54]), [6, 6, 6, 1, 0, 6], [6, 6, 1, 6, 6, 97], 0.4)
    assert got.tolist() == [True, False, False, False, False, False]
    assert not bool(is_bond(1.54, 6, 6, 0.4, same_atom=True))
    assert bool(is_bond(float(limit), 6, 6, 0.4)) and not bool(is_bond(float(np.nextafter(limit, np.float32(9))), 6, 6, 0.4))
    assert bool(is_bond(2.40, 6, 6, 0.9))                                    # the tolerance is the caller's
    # C-Cl 1.77 A: (0.76 + 1.02) + 0.4; the sum is taken first, in fp32
    assert bool(is_bond(1.77, 6, 17)) and not bool(is_bond(2.19, 6, 17))


def test_bond_test_is_exported_from_metrics():
    from cartnet_amd import metrics
    assert metrics.BondTest._fields == ("bonds", "delta_sum", "delta_max", "worst", "over", "ueq_ratio", "crystal_stats")
    with pytest.raises(ValueError, match="u must be"):
        import torch
        metrics.bond_test(torch.zeros(2, 3, 3), {}, torch.zeros(2, dtype=torch.int64))
