"""The tables of cartnet_amd/predict.py, held to literals: every ``*_KEYS`` tuple, every ``*_SPLIT`` mapping and the key
order of a ``predict_adps`` result are derived from one table of key groups, and the order is in the pickle's bytes.
And ``pass_statistics`` on two hand-made results, against the dicts the commit before that table gave
(tests/golden/pass_statistics.json): the result line's figures and the order of its keys."""
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_statistics.json")

KEYS = {
    "KEYS": ("name", "atoms", "frac", "z", "cell", "temp", "u_cart", "u_cif", "u_eq", "principal", "axes", "stats"),
    "SYM_KEYS": ("asym_labels", "asym_frac", "asym_z", "u_cif_asym", "spread", "symops"),
    "ROT_KEYS": ("rot_spread", "frames", "rot_stats"),
    "BOND_KEYS": ("bond_count", "bond_delta_mean", "bond_delta_max", "bond_worst", "bond_over", "bond_ueq_ratio",
                  "bond_stats"),
    "H_KEYS": ("u_iso", "h_parent", "h_count", "h_mult", "h_stats"),
    "H_SYM_KEYS": ("u_iso_asym", "h_parent_asym"),
    "MOL_KEYS": ("mol", "mol_size", "mol_status", "mol_pos", "mol_pairs", "mol_delta_mean", "mol_delta_max", "mol_worst",
                 "mol_over", "mol_stats"),
    "TLS_KEYS": ("tls_u", "tls_resid", "tls_T", "tls_L", "tls_S", "tls_origin", "tls_T_principal", "tls_L_principal",
                 "tls_rank", "tls_r", "tls_stats"),
    "AH_KEYS": ("h_u_cart", "h_u_cif", "h_u_eq", "h_source", "h_aniso_stats"),
    "AH_SYM_KEYS": ("h_u_cif_asym",),
    "SERIES_KEYS": ("t_slope", "t_intercept", "t_ueq_slope", "t_ueq_intercept", "t_resid", "t_drops", "t_stats"),
}
SPLITS = {
    "SPLIT": {"atoms": "row", "frac": "atom", "z": "atom", "cell": "crystal", "u_cart": "row", "u_cif": "row",
              "u_eq": "row", "principal": "row", "axes": "row", "stats": "crystal",
              "u_cif_asym": "site", "spread": "site",
              "rot_spread": "row", "frames": "crystal", "rot_stats": "crystal",
              "bond_count": "row", "bond_delta_mean": "row", "bond_delta_max": "row", "bond_worst": "row",
              "bond_over": "row", "bond_ueq_ratio": "row", "bond_stats": "crystal",
              "u_iso": "atom", "h_parent": "atom", "h_count": "atom", "h_mult": "atom", "h_stats": "crystal"},
    "SERIES_SPLIT": {"t_slope": "row", "t_intercept": "row", "t_ueq_slope": "row", "t_ueq_intercept": "row",
                     "t_resid": "row", "t_drops": "row", "t_stats": "crystal"},
    "MOL_SPLIT": {"mol": "row", "mol_size": "row", "mol_status": "row", "mol_pos": "row", "mol_pairs": "row",
                  "mol_delta_mean": "row", "mol_delta_max": "row", "mol_worst": "row", "mol_over": "row",
                  "mol_stats": "crystal"},
    "TLS_SPLIT": {"tls_u": "row", "tls_resid": "row", "tls_T": "row", "tls_L": "row", "tls_S": "row", "tls_origin": "row",
                  "tls_T_principal": "row", "tls_L_principal": "row", "tls_rank": "row", "tls_r": "row",
                  "tls_stats": "crystal"},
    "AH_SPLIT": {"h_u_cart": "atom", "h_u_cif": "atom", "h_u_eq": "atom", "h_source": "atom", "h_aniso_stats": "crystal"},
}


def test_the_key_tuples_and_split_tables_are_these():
    from cartnet_amd import predict as p
    for name, want in KEYS.items():
        assert getattr(p, name) == want and isinstance(getattr(p, name), tuple), name
    for name, want in SPLITS.items():
        assert list(getattr(p, name).items()) == list(want.items()), name              # contents and order


def test_the_key_order_of_a_result():
    from cartnet_amd.predict import Analyses, result_keys
    k = KEYS
    every = Analyses(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
                     aniso_h=(0.005, 0.020))
    assert result_keys(every, sym=True, rotations=2) == (
        k["KEYS"] + k["SYM_KEYS"] + k["ROT_KEYS"] + k["BOND_KEYS"] + k["H_KEYS"] + k["H_SYM_KEYS"] + k["MOL_KEYS"]
        + k["TLS_KEYS"] + k["AH_KEYS"] + k["AH_SYM_KEYS"])
    assert result_keys(every, sym=False, rotations=2) == (
        k["KEYS"] + k["ROT_KEYS"] + k["BOND_KEYS"] + k["H_KEYS"] + k["MOL_KEYS"] + k["TLS_KEYS"] + k["AH_KEYS"])
    assert result_keys(Analyses(), sym=False, rotations=1) == k["KEYS"]
    assert Analyses() == (None, None, None, None, None)                                    # the defaults mean "off"


def results() -> dict:
    """name -> the arguments of ``pass_statistics``.  ``full``: two crystals at two temperatures (four entries of 3, 3,
    5 and 5 rows) with every stats key and a ``series``; ``empty``: a pass without crystals, with the same keys.  The
    figures are fixed fp64 values with no short binary expansion, so no sum is exact by accident."""
    def rows(table):
        return [torch.tensor(r, dtype=torch.float64) for r in table]
    full = {"name": ["a_100K", "a_200K", "b_100K", "b_200K"], "u_eq": [torch.zeros(n) for n in (3, 3, 5, 5)],
            "stats": rows([[0.0731, 0.0113, 0.0], [0.0917, 0.0127, 1.0], [0.1523, -0.0031, 2.0], [0.1871, 0.0093, 0.0]]),
            "rot_stats": rows([[0.00137, 0.00061], [0.00171, 0.00083], [0.00293, 0.00079], [0.00331, 0.00097]]),
            "bond_stats": rows([[4.0, 0.00213, 0.00071, 1.0], [4.0, 0.00257, 0.00093, 0.0], [8.0, 0.00611, 0.00127, 2.0],
                                [8.0, 0.00733, 0.00119, 3.0]]),
            "h_stats": rows([[5.0, 1.0, 0.1391, 0.0], [5.0, 1.0, 0.1717, 1.0], [7.0, 0.0, 0.2931, 0.0],
                             [7.0, 0.0, 0.3373, 2.0]]),
            "h_aniso_stats": rows([[4.0, 3.0, 0.1193, 0.0], [4.0, 3.0, 0.1471, 1.0], [7.0, 0.0, 0.2513, 0.0],
                                   [7.0, 0.0, 0.2891, 1.0]]),
            "mol_stats": rows([[2.0, 1.0, 1.0, 0.0, 3.0, 6.0, 0.00371, 0.00091, 1.0],
                               [2.0, 1.0, 1.0, 0.0, 3.0, 6.0, 0.00433, 0.00113, 2.0],
                               [3.0, 2.0, 0.0, 1.0, 5.0, 20.0, 0.01337, 0.00157, 4.0],
                               [3.0, 2.0, 0.0, 1.0, 5.0, 20.0, 0.01571, 0.00149, 5.0]]),
            "tls_stats": rows([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                               [1.0, 1.0, 0.0, 3.1e-7, 0.00471, 0.00033], [1.0, 1.0, 1.0, 4.3e-7, 0.00613, 0.00041]]),
            "series": {"name": ["a", "b"],
                       "t_stats": rows([[0.000213, 1.0, 0.0, 0.00017], [0.000371, 0.0, 2.0, 0.00029]])}}
    empty = {k: [] for k in full if k != "series"}
    empty["series"] = {"name": [], "t_stats": []}
    return {"full": (full, "out.pkl", "cifs", [("x", "why")], 2, [100.0, 200.0]),
            "empty": (empty, None, None, None, 2, [100.0, 200.0])}


def test_pass_statistics_gives_the_recorded_lines():
    from cartnet_amd.predict import pass_statistics
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = {name: json.dumps(pass_statistics(*args)) for name, args in results().items()}
    assert set(got) == set(golden)
    for name, line in got.items():
        assert line == golden[name], name                                                   # the figures' bits and the key order
