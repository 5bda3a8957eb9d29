"""The six bond-graph analyses against the bytes of the commit before their kernels moved onto csrc/bond_graph.h:
``tools/analysis_bytes.py`` on its fixed batches, every output array's sha256 against ``tests/golden/analysis_bytes.json``
(recorded with that commit's library on an MI355X).  The kernels give the same bytes on every run, so equality is the
bound: a helper that changed how a multiply-add is contracted, or the order of a fold, fails here."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("bond_test", "riding_h", "molecules", "molecule_test", "tls_fit", "aniso_h", "aniso_h_bare")


def test_every_output_array_has_the_bytes_of_the_parent_commit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import analysis_bytes
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "analysis_bytes.json")) as f:
        want = json.load(f)
    got = analysis_bytes.run()
    assert sorted(got) == sorted(want) == ["aniso", "dense_segment", "no_edges", "pairs", "ragged", "tls"]
    moved = []
    for case in sorted(want):
        assert sorted(got[case]) == sorted(want[case]) and {k.split(".")[0] for k in want[case]} == set(ENTRIES), case
        moved += [f"{case}: {key}" for key in sorted(want[case]) if got[case][key] != want[case][key]]
    print(f"{sum(len(v) for v in want.values())} arrays compared, {len(moved)} moved")
    assert not moved, moved
