"""The prediction pass gives the bytes it gave before it was restated over one record of options, one table of key
groups and one stage: tools/predict_bytes.py's digests of ``predict_adps`` (plain, in frames, with every analysis, over a
temperature series, at one temperature, from a CIF file), of ``pass_statistics`` and of ``evaluate.inference`` against
tests/golden/predict_bytes.json, which the commit before that change wrote (two runs of it agreed)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
with open(os.path.join(ROOT, "tests", "golden", "predict_bytes.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def digests():
    spec = importlib.util.spec_from_file_location("predict_bytes", os.path.join(ROOT, "tools", "predict_bytes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert set(GOLDEN) == set(tool.PREDICT) | set(tool.INFERENCE)
    return tool.run()


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_the_pass_gives_the_recorded_bytes(digests, case):
    got, want = digests[case], GOLDEN[case]
    assert got["keys"] == want["keys"]                                        # and their order: it is in the pickle
    assert got == want
