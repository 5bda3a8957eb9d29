"""``cartnet_adp_export`` (csrc/export_ops.hip) against fp64 numpy on the same fp32 inputs: the predictions on the unit
reciprocal axes, U_eq, principal values and axes, the per-crystal statistics, and the round trip through the transform the
reference applied to the dataset's targets (dataset/extract_csd_data.py:115-123, restated in tests/predict_utils.py)."""
import numpy as np
import pytest
import torch

import predict_utils as pu

pytestmark = pytest.mark.gpu

EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24
KINDS = ("cubic", "orthorhombic", "triclinic", "triclinic_rotated")


def _rows():
    """Empty crystals first, in the middle and last; one crystal crosses a tile boundary of the kernel."""
    from cartnet_amd.metrics import ADP_EXPORT_TILE as T
    return [0, 3, 1, 0, T + 44, 2, 0]


def _cells(B, shift):
    """[B,3,3] fp32: crystal g has kind (g + shift) % 4, each scaled a little differently."""
    c = pu.cells()
    return np.stack([c[KINDS[(g + shift) % 4]] * np.float32(1.0 + 0.03 * g) for g in range(B)])


def _tensors(M, seed):
    """[M,3,3] fp32: L L^T of scale 0.02, row 1 = 0.01 I (degenerate axes), rows 2 and M - 3 with principal values in ratio
    1 : 1e4 on generic axes; every fifth row carries a small antisymmetric part (the kernel symmetrises)."""
    g = torch.Generator().manual_seed(seed)
    L = torch.randn(M, 3, 3, generator=g, dtype=torch.float64)
    U = 0.02 * L @ L.transpose(1, 2)
    if M > 1:
        U[1] = 0.01 * torch.eye(3, dtype=torch.float64)
    R = torch.from_numpy(pu.fixed_rotation())
    flat = R @ torch.diag(torch.tensor([5e-6, 2e-2, 5e-2], dtype=torch.float64)) @ R.T
    for r in (2, M - 3):
        if 0 <= r < M:
            U[r] = flat
    A = 1e-4 * torch.randn(M, 3, 3, generator=g, dtype=torch.float64)
    U[::5] += (A - A.transpose(1, 2))[::5]
    return U.to(torch.float32)


def _ptr(rows):
    return torch.tensor([0] + list(rows), dtype=torch.int64).cumsum(0).cuda()


def _check_against_fp64(res, u, rows, cells, skip=()):
    """Every bound of the issue, per crystal; prints each figure before it asserts."""
    u_np = u.numpy()
    got = {k: getattr(res, k).cpu().numpy() for k in ("u_cif", "u_eq", "principal", "axes")}
    at = 0
    for g, n in enumerate(rows):
        sl = slice(at, at + n)
        at += n
        if n == 0 or g in skip:
            continue
        cif, ueq, prin, U = pu.export_reference(u_np[sl], cells[g])
        for name, ref in (("u_cif", cif), ("u_eq", ueq), ("principal", prin)):
            err, bound = np.abs(np.asarray(got[name][sl], dtype=np.float64) - ref).max(), EPS23 * np.abs(ref).max()
            print(f"crystal {g} {name}: max error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (g, name)
        V, lam = np.asarray(got["axes"][sl], dtype=np.float64), np.asarray(got["principal"][sl], dtype=np.float64)
        recon = np.einsum("nka,nk,nkb->nab", V, lam, V)
        err = np.abs(recon - U).max(axis=(1, 2)) / np.abs(lam).max(axis=1)
        orth = np.abs(np.einsum("nak,nbk->nab", V, V) - np.eye(3)).max()
        print(f"crystal {g} axes: reconstruction {err.max():.3e} (bound {2.0 ** -20:.3e}), orthonormality {orth:.3e} "
              f"(bound {2.0 ** -21:.3e})")
        assert err.max() <= 2.0 ** -20 and orth <= 2.0 ** -21
        big = np.take_along_axis(V, np.abs(V).argmax(axis=2)[..., None], axis=2)
        assert (big > 0).all()                                               # sign-normalised
        assert (np.diff(got["principal"][sl], axis=1) >= 0).all()            # ascending


def _check_stats(res, rows):
    st = res.crystal_stats.cpu()
    assert st.dtype == torch.float64 and tuple(st.shape) == (len(rows), 3)
    ueq, lo = torch.split(res.u_eq.double().cpu(), rows), torch.split(res.principal[:, 0].double().cpu(), rows)
    for g, n in enumerate(rows):
        if n == 0:
            assert st[g].tolist() == [0.0, float("inf"), 0.0]
            continue
        assert abs(st[g, 0].item() - ueq[g].sum().item()) <= 1e-12 * abs(ueq[g].sum().item())
        assert st[g, 1].item() == lo[g].min().item() and st[g, 2].item() == float((lo[g] <= 0).sum())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_export_against_fp64(shift):
    from cartnet_amd import metrics as gm
    rows = _rows()
    M, B = sum(rows), len(rows)
    u, cells = _tensors(M, 10 + shift), _cells(B, shift)
    ud, cd, rp = u.cuda(), torch.from_numpy(cells).cuda(), _ptr(rows)
    res = gm.adp_export(ud, rp, cd)
    assert res.status.tolist() == [0] * B
    _check_against_fp64(res, u, rows, cells)
    _check_stats(res, rows)
    again = gm.adp_export(ud, rp, cd)
    for a, b in zip(res, again):
        assert torch.equal(a, b)                                             # no atomics, fixed order
    assert res.crystal_stats.cpu().numpy().tobytes() == again.crystal_stats.cpu().numpy().tobytes()
    part = gm.adp_export(ud, rp, cd, axes=None, stats=None)
    assert part.axes is None and part.crystal_stats is None
    for k in ("u_cif", "u_eq", "principal", "status"):
        assert torch.equal(getattr(part, k), getattr(res, k)), k


def test_a_non_positive_principal_value_is_counted():
    from cartnet_amd import metrics as gm
    rows = [4, 0, 3]
    u = _tensors(7, 3)
    u[1] = torch.diag(torch.tensor([0.02, -0.001, 0.03]))
    u[5] = torch.zeros(3, 3)
    cells = _cells(3, 2)
    res = gm.adp_export(u.cuda(), _ptr(rows), torch.from_numpy(cells).cuda())
    _check_stats(res, rows)
    st = res.crystal_stats.cpu()
    assert st[:, 2].tolist() == [1.0, 0.0, 1.0] and st[0, 1].item() == float(np.float32(-0.001))


def test_one_crystal_and_no_rows():
    from cartnet_amd import lib as _l
    from cartnet_amd import metrics as gm
    M = 70
    u, cells = _tensors(M, 5), _cells(1, 3)
    res = gm.adp_export(u.cuda(), _ptr([M]), torch.from_numpy(cells).cuda())
    _check_against_fp64(res, u, [M], cells)
    _check_stats(res, [M])
    cells = _cells(3, 0)
    empty = gm.adp_export(u[:0].cuda(), _ptr([0, 0, 0]), torch.from_numpy(cells).cuda())
    assert tuple(empty.u_cif.shape) == (0, 6) and tuple(empty.axes.shape) == (0, 3, 3) and empty.status.tolist() == [0] * 3
    _check_stats(empty, [0, 0, 0])
    # the entry point itself: no rows or no crystals is not an error and launches nothing
    assert _l.load().cartnet_adp_export(None, None, None, 3, 0, None, None, None, None, None, None, None) == 0
    assert _l.load().cartnet_adp_export(None, None, None, 0, 0, None, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        gm.adp_export(u.cuda(), _ptr([M]), torch.from_numpy(_cells(2, 0)).cuda())      # two cells for one crystal
    with pytest.raises(ValueError):
        gm.adp_export(u.cuda().double(), _ptr([M]), torch.from_numpy(_cells(1, 0)).cuda())


def test_singular_cell_in_the_middle_of_a_batch():
    from cartnet_amd import metrics as gm
    rows = _rows()
    M, B = sum(rows), len(rows)
    u, cells = _tensors(M, 8), _cells(B, 1)
    good = gm.adp_export(u.cuda(), _ptr(rows), torch.from_numpy(cells).cuda())
    cells[2, 1] = 0.0                                                        # crystal 2 (row 3): a zero lattice vector
    with pytest.raises(ValueError, match="crystal 2"):
        gm.adp_export(u.cuda(), _ptr(rows), torch.from_numpy(cells).cuda())
    res = gm.adp_export(u.cuda(), _ptr(rows), torch.from_numpy(cells).cuda(), check=False)
    assert res.status.tolist() == [0, 0, 1, 0, 0, 0, 0]
    with pytest.raises(ValueError, match=r"crystal 2 \(c\)"):
        gm.check_export_status(res.status.cpu(), names=list("abcdefg"))
    keep = torch.ones(M, dtype=torch.bool)
    keep[3] = False
    for k in ("u_cif", "u_eq", "principal", "axes"):
        a, b = getattr(res, k).cpu(), getattr(good, k).cpu()
        assert torch.equal(a[keep], b[keep]), k                              # the other crystals' rows are untouched
        assert torch.isnan(a[3]).all(), k
    _check_against_fp64(res, u, rows, cells, skip=(2,))
    st, st_good = res.crystal_stats.cpu(), good.crystal_stats.cpu()
    others = [g for g in range(B) if g != 2]
    assert torch.equal(st[others], st_good[others])


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_through_the_reference_transform(kind):
    """Random symmetric U_cif -> Cartesian in fp64 by the reference's formula -> fp32 -> export.  Bound per crystal:
    8 * 2^-24 * max|U_cart| (input rounding: |delta|_F <= 3 * 2^-24 max|U_cart| seen through two unit vectors; the output's
    own rounding at most another 3 * 2^-24 max|U_cart|; the rest is slack)."""
    from cartnet_amd import metrics as gm
    rows = [37, 0, 5]
    cell = pu.cells()[kind]
    cells = np.stack([cell, cell * np.float32(1.7), cell * np.float32(0.6)])
    rng = np.random.default_rng(4)
    s = rng.normal(size=(sum(rows), 3, 3)) * 0.02
    u_cif = 0.5 * (s + s.transpose(0, 2, 1))
    per_row_cell = np.repeat(np.arange(3), rows)
    u_cart = np.stack([pu.cart_from_cif(u_cif[i:i + 1], cells[per_row_cell[i]])[0] for i in range(sum(rows))])
    res = gm.adp_export(torch.from_numpy(np.float32(u_cart)).cuda(), _ptr(rows), torch.from_numpy(cells).cuda())
    got = np.asarray(res.u_cif.cpu().numpy(), dtype=np.float64)
    want = np.stack([u_cif[:, i, j] for i, j in pu.CIF_ORDER], axis=1)
    for g in (0, 2):
        sel = per_row_cell == g
        err, bound = np.abs(got[sel] - want[sel]).max(), 8 * EPS24 * np.abs(u_cart[sel]).max()
        print(f"{kind} crystal {g}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
