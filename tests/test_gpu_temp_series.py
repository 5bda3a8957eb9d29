"""``cartnet_adp_temp_series`` (csrc/series_ops.hip) against fp64 numpy on the same fp32 inputs: the least-squares line per
row and column over T temperatures, the largest residual, the steps on which U_eq falls, the per-crystal figures; the exact
cases (members on a line of dyadic coefficients, constant members, two runs), a NaN member and the argument checks."""
import numpy as np
import pytest
import torch

from temp_series_utils import line_bounds, line_reference

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 65, 130, 7)       # an empty crystal, a single row, past one and two strides of a wave, a ragged grid tail
M, B = sum(ROWS), len(ROWS)
TEMPS = {2: (93.5, 120.0), 3: (93.5, 120.0, 200.25), 7: (93.5, 120.0, 200.25, 210.0, 250.5, 293.0, 400.125)}
TILED = (1030, 0, 5)            # one crystal across the boundary of a workgroup's tile (1024 rows), an empty one, a tail


def _ptr(rows=ROWS):
    return torch.tensor((0,) + tuple(rows), dtype=torch.int64).cumsum(0).cuda()


def _per_crystal(rows=ROWS):
    at = 0
    for g, n in enumerate(rows):
        yield g, n, slice(at, at + n)
        at += n


def _members(T, m, seed):
    """``u_cif`` [T*m,6] (signed, scale 0.05) and ``u_eq`` [T*m] (positive, growing with t on average, not monotonically):
    plain random fp32."""
    g = torch.Generator().manual_seed(seed)
    u_cif = 0.05 * torch.randn(T * m, 6, generator=g)
    u_eq = 0.02 + 0.01 * torch.arange(T).repeat_interleave(m) + 0.02 * torch.rand(T * m, generator=g)
    return u_cif.float(), u_eq.float()


def _run(u_cif, u_eq, temps, rows=ROWS, **kw):
    from cartnet_amd import metrics as gm
    return gm.temp_series(u_cif.cuda(), u_eq.cuda(), temps, _ptr(rows), **kw)


def _np(res):
    """(slope [m,7], intercept [m,7], resid [m], drops [m]) of a ``TempSeries`` on the host, fp64."""
    s = torch.cat([res.slope, res.ueq_slope.unsqueeze(1)], dim=1).cpu().numpy().astype(np.float64)
    i = torch.cat([res.intercept, res.ueq_intercept.unsqueeze(1)], dim=1).cpu().numpy().astype(np.float64)
    return s, i, res.resid.cpu().numpy().astype(np.float64), res.drops.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """Per T: the fp32 inputs, the kernel's result and the fp64 reference, computed once and left unchanged."""
    out = {}
    for T, temps in TEMPS.items():
        u_cif, u_eq = _members(T, M, 50 + T)
        ref = line_reference(u_cif.numpy().reshape(T, M, 6), u_eq.numpy().reshape(T, M), temps)
        out[T] = (u_cif, u_eq, _run(u_cif, u_eq, temps), ref)
    return out


def _check_against_fp64(res, u_cif, u_eq, temps, rows, m, ref):
    T = len(temps)
    slope, intercept, resid, drops = ref
    got_s, got_i, got_r, got_d = _np(res)
    assert res.slope.dtype == torch.float32 and tuple(res.slope.shape) == (m, 6) == tuple(res.intercept.shape)
    assert tuple(res.ueq_slope.shape) == (m,) == tuple(res.ueq_intercept.shape) == tuple(res.resid.shape)
    assert res.drops.dtype == torch.int32 and tuple(res.drops.shape) == (m,)
    c3, e2 = u_cif.numpy().reshape(T, m, 6), u_eq.numpy().reshape(T, m)
    for g, n, sl in _per_crystal(rows):
        if n == 0:
            continue
        bs, bi, br = line_bounds(c3[:, sl], e2[:, sl], temps, slope[sl], intercept[sl], resid[sl])
        for what, err, bound in (("slope", np.abs(got_s[sl] - slope[sl]).max(), bs),
                                 ("intercept", np.abs(got_i[sl] - intercept[sl]).max(), bi),
                                 ("resid", np.abs(got_r[sl] - resid[sl]).max(), br)):
            print(f"T={T} crystal {g} {what}: max error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (T, g, what)
    assert (got_d == drops).all()


def _check_stats(res, rows):
    cs = res.crystal_stats.cpu()
    assert cs.dtype == torch.float64 and tuple(cs.shape) == (len(rows), 4)
    s, r, d = res.ueq_slope.cpu(), res.resid.cpu().double(), res.drops.cpu()
    for g, n, sl in _per_crystal(rows):
        if n == 0:
            assert cs[g].tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        assert np.allclose(cs[g, 0].item(), s[sl].double().sum().item(), rtol=1e-12, atol=0)    # only the order differs
        assert cs[g, 1].item() == float((~(s[sl] > 0)).sum())
        assert cs[g, 2].item() == float((d[sl] > 0).sum())
        assert cs[g, 3].item() == r[sl].max().item()


@pytest.mark.parametrize("T", sorted(TEMPS))
def test_line_against_fp64(cases, T):
    u_cif, u_eq, res, ref = cases[T]
    _check_against_fp64(res, u_cif, u_eq, TEMPS[T], ROWS, M, ref)
    if T == 2:
        assert float(res.resid.max()) <= 2.0 ** -23 * float(u_cif.abs().max())        # two points lie on their line
    else:
        assert (ref[3] > 0).any() and (ref[3] == 0).any()                              # both kinds of row are in the data


@pytest.mark.parametrize("T", sorted(TEMPS))
def test_crystal_stats_restate_the_stored_rows(cases, T):
    _check_stats(cases[T][2], ROWS)


@pytest.mark.parametrize("T", sorted(TEMPS))
def test_two_runs_give_the_same_bytes_and_stats_are_optional(cases, T):
    u_cif, u_eq, res, _ = cases[T]
    again = _run(u_cif, u_eq, TEMPS[T])
    for a, b in zip(res, again):
        assert a.contiguous().cpu().numpy().tobytes() == b.contiguous().cpu().numpy().tobytes()
    part = _run(u_cif, u_eq, TEMPS[T], stats=False)
    assert part.crystal_stats is None
    for a, b in zip(res[:6], part[:6]):
        assert a.contiguous().cpu().numpy().tobytes() == b.contiguous().cpu().numpy().tobytes()
    as_tensor = _run(u_cif, u_eq, torch.tensor(TEMPS[T], dtype=torch.float32).cuda())
    assert all(torch.equal(a, b) for a, b in zip(res, as_tensor))


def test_rows_across_a_tile_boundary():
    T, temps, m = 3, TEMPS[3], sum(TILED)
    u_cif, u_eq = _members(T, m, 61)
    res = _run(u_cif, u_eq, temps, TILED)
    _check_against_fp64(res, u_cif, u_eq, temps, TILED, m,
                        line_reference(u_cif.numpy().reshape(T, m, 6), u_eq.numpy().reshape(T, m), temps))
    _check_stats(res, TILED)


def _on_a_line(b6_sign=1):
    """Members ``a_c + b_c T_t`` at (100, 200, 300, 400) K with ``a = i 2^-12``, ``b = j 2^-20``, i and j small integers:
    every member is exact in fp32, every product and sum of the kernel exact in fp64."""
    temps = (100.0, 200.0, 300.0, 400.0)
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-40, 41, (M, 7), generator=g).double() * 2.0 ** -12
    b = torch.randint(-9, 10, (M, 7), generator=g).double() * 2.0 ** -20
    b[:, 6] = b[:, 6].abs() * b6_sign
    u = a.unsqueeze(0) + b.unsqueeze(0) * torch.tensor(temps, dtype=torch.float64).view(4, 1, 1)      # [4,M,7]
    assert torch.equal(u.float().double(), u)
    return temps, a, b, u[..., :6].reshape(4 * M, 6).float(), u[..., 6].reshape(4 * M).float()


def test_an_exact_line_comes_back_exactly():
    temps, a, b, u_cif, u_eq = _on_a_line()
    res = _run(u_cif, u_eq, temps)
    slope, intercept, resid, drops = _np(res)
    assert (slope == b.numpy()).all() and (intercept == a.numpy()).all()
    assert (resid == 0).all() and (drops == 0).all()                          # b_6 >= 0 in every row
    cs = res.crystal_stats.cpu()
    for g, n, sl in _per_crystal():
        assert cs[g, 0].item() == b[sl, 6].sum().item() and cs[g, 3].item() == 0.0 and cs[g, 2].item() == 0.0
        assert cs[g, 1].item() == float((b[sl, 6] == 0).sum())


def test_a_strictly_decreasing_u_eq_drops_on_every_step():
    temps, a, b, u_cif, u_eq = _on_a_line(b6_sign=-1)
    falling = (b[:, 6] < 0).numpy()
    assert falling.any() and not falling.all()
    res = _run(u_cif, u_eq, temps)
    drops = res.drops.cpu().numpy()
    assert (drops[falling] == 3).all() and (drops[~falling] == 0).all()
    cs = res.crystal_stats.cpu()
    for g, n, sl in _per_crystal():
        assert cs[g, 2].item() == float(falling[sl].sum()) and cs[g, 1].item() == float(n)       # no slope is > 0


def test_constant_members():
    """Unequally spaced temperatures whose mean (200) and deviations (-100, -50, 150) are small integers: every product
    ``(T_t - tbar) u`` is then exact in fp64 and their sum is exactly 0, whatever the fp32 value u."""
    T, temps = 3, (100.0, 150.0, 350.0)
    g = torch.Generator().manual_seed(4)
    u_cif, u_eq = 0.05 * torch.randn(M, 6, generator=g), 0.02 + 0.02 * torch.rand(M, generator=g)
    res = _run(u_cif.repeat(T, 1), u_eq.repeat(T), temps)
    slope, intercept, resid, drops = _np(res)
    assert (slope == 0).all() and (resid == 0).all() and (drops == 0).all()
    assert torch.equal(res.intercept.cpu(), u_cif) and torch.equal(res.ueq_intercept.cpu(), u_eq)
    assert res.crystal_stats[:, 1].cpu().tolist() == [float(n) for n in ROWS]  # a slope of 0 is not > 0
    assert res.crystal_stats[:, 0].cpu().tolist() == [0.0] * B


@pytest.mark.parametrize("column", [2, 6])
def test_a_nan_member_stays_in_its_row(cases, column):
    T = 3
    u_cif, u_eq, clean, _ = cases[T]
    row, t = 70, 1                                                            # a row of crystal 3, the middle temperature
    u_cif, u_eq = u_cif.clone(), u_eq.clone()
    if column < 6:
        u_cif[t * M + row, column] = float("nan")
    else:
        u_eq[t * M + row] = float("nan")
    res = _run(u_cif, u_eq, TEMPS[T])
    s = torch.cat([res.slope, res.ueq_slope.unsqueeze(1)], dim=1).cpu()
    i = torch.cat([res.intercept, res.ueq_intercept.unsqueeze(1)], dim=1).cpu()
    assert torch.isnan(s[row, column]) and torch.isnan(i[row, column]) and torch.isnan(res.resid[row])
    others = torch.arange(M) != row
    for a, b in zip(res[:6], clean[:6]):
        assert a.cpu()[others].numpy().tobytes() == b.cpu()[others].numpy().tobytes()
    cs, cs0 = res.crystal_stats.cpu(), clean.crystal_stats.cpu()
    assert torch.isnan(cs[3, 3]) and torch.equal(cs[[0, 1, 2, 4]], cs0[[0, 1, 2, 4]])
    if column == 6:                                                           # a NaN slope is not > 0: slot 1 counts it
        assert cs[3, 1].item() == cs0[3, 1].item() + (1.0 if clean.ueq_slope[row].item() > 0 else 0.0)


def test_argument_checks():
    from cartnet_amd import metrics as gm
    T, temps = 3, TEMPS[3]
    u_cif, u_eq = (t.cuda() for t in _members(T, M, 3))
    with pytest.raises(ValueError, match="temps"):
        gm.temp_series(u_cif[:M], u_eq[:M], (150.0,), _ptr())                                   # T = 1
    with pytest.raises(ValueError, match="temps.*increasing"):
        gm.temp_series(u_cif, u_eq, (93.5, 200.25, 120.0), _ptr())
    with pytest.raises(ValueError, match="temps.*increasing"):
        gm.temp_series(u_cif, u_eq, (93.5, 120.0, 120.0), _ptr())
    with pytest.raises(ValueError, match="temps.*> 0"):
        gm.temp_series(u_cif, u_eq, (0.0, 120.0, 200.25), _ptr())
    with pytest.raises(ValueError, match="temps.*finite"):
        gm.temp_series(u_cif, u_eq, (93.5, 120.0, float("inf")), _ptr())
    with pytest.raises(ValueError, match="u_cif must be"):
        gm.temp_series(u_cif.double(), u_eq, temps, _ptr())
    with pytest.raises(ValueError, match="u_eq must be"):
        gm.temp_series(u_cif, u_eq.double(), temps, _ptr())
    with pytest.raises(ValueError, match="u_eq must hold"):
        gm.temp_series(u_cif, u_eq[:-1], temps, _ptr())
    with pytest.raises(ValueError, match="no multiple"):
        gm.temp_series(u_cif[:-1], u_eq[:-1], temps, _ptr())
    with pytest.raises(ValueError, match="row_ptr"):
        gm.temp_series(u_cif, u_eq, temps, _ptr().to(torch.int32))
    empty = gm.temp_series(u_cif[:0], u_eq[:0], temps, torch.zeros(B + 1, dtype=torch.int64, device="cuda:0"))
    assert tuple(empty.slope.shape) == (0, 6) and tuple(empty.ueq_slope.shape) == (0,) and tuple(empty.drops.shape) == (0,)
    assert empty.crystal_stats.tolist() == [[0.0] * 4] * B
    assert gm.temp_series(u_cif[:0], u_eq[:0], temps, _ptr() * 0, stats=False).crystal_stats is None
