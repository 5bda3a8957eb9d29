"""``--predict_temperatures`` on the host: the parser of the flag, the binding of ``cartnet_adp_temp_series`` and the fp64
numpy restatement of its line (tests/temp_series_utils.py, which the GPU tests hold the kernel to) against
``numpy.polyfit``."""
import os
import re

import numpy as np
import pytest

from temp_series_utils import line_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lists_and_ranges():
    from main import parse_temperatures
    assert parse_temperatures("100,150,200") == [100.0, 150.0, 200.0]
    assert parse_temperatures(" 93.5 , 120,200.25 ") == [93.5, 120.0, 200.25]
    assert parse_temperatures("150") == [150.0]
    assert parse_temperatures("100:300:50") == [100.0, 150.0, 200.0, 250.0, 300.0]
    assert parse_temperatures("100:290:50") == [100.0, 150.0, 200.0, 250.0]
    assert parse_temperatures("100:300:100") == [100.0, 200.0, 300.0]
    assert parse_temperatures("100:100:10") == [100.0]
    assert parse_temperatures("90:91:0.1")[-1] == pytest.approx(91.0, abs=1e-9) and len(parse_temperatures("90:91:0.1")) == 11
    assert all(isinstance(v, float) for v in parse_temperatures("100:300:50"))


@pytest.mark.parametrize("spec,word", [
    ("", "empty"), ("  ", "empty"), (None, "empty"),
    ("100,abc", "no number"), ("100,,200", "no number"), ("a:300:50", "no number"), ("100:300", "A:B:STEP"),
    ("100:300:50:2", "A:B:STEP"),
    ("100,inf", "not finite"), ("nan", "not finite"), ("100:inf:50", "not finite"),
    ("0,100", "> 0"), ("-5", "> 0"), ("-100:100:50", "> 0"),
    ("200,100", "strictly increasing"), ("100,100", "strictly increasing"),
    ("100:300:0", "STEP"), ("100:300:-50", "STEP"),
    ("300:100:50", "empty"),
])
def test_rejections(spec, word):
    from main import parse_temperatures
    with pytest.raises(SystemExit) as e:
        parse_temperatures(spec)
    assert "--predict_temperatures" in str(e.value) and word in str(e.value)


def test_the_flag_is_refused_before_the_device_is_touched(monkeypatch):
    """Without ``--predict`` and with ``--disable_temp``: ``main`` exits on its arguments alone."""
    import main as entry
    from cartnet_amd.config import set_cfg

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry, "create_model", touched)
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    try:
        with pytest.raises(SystemExit, match="--predict only"):
            entry.main(["--predict_temperatures", "100,200"])
        common = ["--predict", "--predict_input", "x.cnshard", "--checkpoint_path", "x.ckpt"]
        with pytest.raises(SystemExit, match="--disable_temp"):
            entry.main(common + ["--predict_temperatures", "100,200", "--disable_temp"])
        with pytest.raises(SystemExit, match="strictly increasing"):
            entry.main(common + ["--predict_temperatures", "200,100"])
    finally:
        set_cfg()


def test_the_binding_mirrors_the_header():
    from cartnet_amd import lib
    from cartnet_amd.build import SOURCES
    from cartnet_amd.predict import SERIES_KEYS, SERIES_SPLIT, SPLIT
    with open(os.path.join(ROOT, "include", "cartnet_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_temp_series\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 13 == len(lib.PROTOTYPES["cartnet_adp_temp_series"][1])
    assert "series_ops.hip" in SOURCES
    assert lib.ABI_VERSION == 16
    assert [SERIES_SPLIT[k] for k in SERIES_KEYS] == ["row"] * 6 + ["crystal"] and tuple(SERIES_SPLIT) == SERIES_KEYS
    assert not set(SERIES_SPLIT) & set(SPLIT)


def test_the_entry_point_checks_its_sizes_without_a_launch():
    """No kernel is launched for any of these: sizes are refused, and nothing to do returns at once."""
    from cartnet_amd import lib
    l = lib.load()
    f, none = l.cartnet_adp_temp_series, (None,) * 5
    assert f(None, None, None, 2, None, 4, 0, *none, None) == 0              # M == 0
    assert f(None, None, None, 2, None, 0, 0, *none, None) == 0              # B == 0
    assert f(None, None, None, 1, None, 4, 0, *none, None) != 0              # T < 2
    assert b"bad sizes" in l.cartnet_last_error()
    assert f(None, None, None, 2, None, 4, -1, *none, None) != 0
    assert f(None, None, None, 2, None, 4, 5, *none, None) != 0              # before any launch
    assert b"null pointer" in l.cartnet_last_error()


def test_the_restatement_reproduces_polyfit():
    rng = np.random.default_rng(7)
    for T in (2, 3, 7):
        temps = np.sort(rng.uniform(80.0, 400.0, T)).astype(np.float32)
        u_cif = rng.normal(0.0, 0.05, (T, 40, 6)).astype(np.float32)
        u_eq = rng.uniform(0.01, 0.1, (T, 40)).astype(np.float32)
        slope, intercept, resid, drops = line_reference(u_cif, u_eq, temps)
        y = np.concatenate([u_cif, u_eq[..., None]], axis=2).astype(np.float64).reshape(T, -1)
        t64 = temps.astype(np.float64)
        p = np.polyfit(t64, y, 1)                                             # [2, M*7]: slope, intercept
        scale = np.abs(y).max()
        assert np.abs(slope.reshape(-1) - p[0]).max() <= 1e-10 * np.abs(p[0]).max()
        assert np.abs(intercept.reshape(-1) - p[1]).max() <= 1e-10 * max(np.abs(p[1]).max(), scale)
        fit = p[0][None] * t64[:, None] + p[1][None]
        want = np.abs(y - fit).reshape(T, 40, 7).max(axis=(0, 2))
        assert np.abs(resid - want).max() <= 1e-10 * scale
        assert (drops == (np.diff(u_eq, axis=0) < 0).sum(axis=0)).all()
        if T == 2:
            assert resid.max() <= 1e-12 * scale                               # two points lie on their line
