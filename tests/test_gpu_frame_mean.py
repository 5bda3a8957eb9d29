"""``cartnet_adp_frame_mean`` (csrc/frame_ops.hip) against fp64 numpy on the same fp32 inputs: the mean over K frames of
``R P_k R^T``, the largest deviation of a member from it, the per-crystal sums; the exact cases (one identity frame, two
runs) and the direction of the convention (an equivariant model's members come back to one tensor, the transposed
convention's do not)."""
import numpy as np
import pytest
import torch

from test_gpu_adp_export import _tensors          # random SPD rows with 0.01 I and two 1 : 1e4 flat ones

pytestmark = pytest.mark.gpu

EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24
ROWS = (0, 1, 65, 130, 7)       # an empty crystal, a single row, past one and two strides of a wave, a ragged grid tail
M, B = sum(ROWS), len(ROWS)
KS = (1, 2, 7)


def _ptr():
    return torch.tensor((0,) + ROWS, dtype=torch.int64).cumsum(0).cuda()


def _crystal_of_row():
    return np.repeat(np.arange(B), ROWS)


def _reference(pred: np.ndarray, rot: np.ndarray):
    """fp64: members U [K,M,3,3] = R P R^T, their mean [M,3,3] and spread [M]; ``pred`` [K*M,3,3], ``rot`` [K,B,3,3]."""
    K = rot.shape[0]
    P = np.asarray(pred, dtype=np.float64).reshape(K, M, 3, 3)
    R = np.asarray(rot, dtype=np.float64)[:, _crystal_of_row()]               # [K,M,3,3]
    U = np.einsum("kmab,kmbd,kmcd->kmac", R, P, R)
    mean = U.mean(axis=0)
    return U, mean, np.abs(U - mean[None]).max(axis=(0, 2, 3))


@pytest.fixture(scope="module")
def cases():
    """Per K: the fp32 inputs on the device, the kernel's result and the fp64 reference, computed once and left unchanged."""
    from cartnet_amd import metrics as gm
    from cartnet_amd.shard import random_rotations
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    out = {}
    for K in KS:
        pred = _tensors(K * M, 20 + K).cuda()
        rot = random_rotations(K * B, gen, "cuda:0").view(K, B, 3, 3)
        res = gm.frame_mean(pred, rot, _ptr())
        out[K] = (pred, rot, res, _reference(pred.cpu().numpy(), rot.cpu().numpy()))
    return out


def _per_crystal():
    at = 0
    for g, n in enumerate(ROWS):
        yield g, n, slice(at, at + n)
        at += n


@pytest.mark.parametrize("K", KS)
def test_mean_and_spread_against_fp64(cases, K):
    _, _, res, (U, mean, spread) = cases[K]
    assert tuple(res.mean.shape) == (M, 3, 3) and tuple(res.spread.shape) == (M,) and res.mean.dtype == torch.float32
    got_m, got_s = res.mean.cpu().numpy().astype(np.float64), res.spread.cpu().numpy().astype(np.float64)
    for g, n, sl in _per_crystal():
        if n == 0:
            continue
        err, bound = np.abs(got_m[sl] - mean[sl]).max(), EPS23 * np.abs(mean[sl]).max()
        print(f"K={K} crystal {g} mean: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (K, g)
        err, bound = np.abs(got_s[sl] - spread[sl]).max(), EPS23 * spread[sl].max() + 1e-12 * np.abs(U[:, sl]).max()
        print(f"K={K} crystal {g} spread: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (K, g)
    assert (got_s >= 0).all()
    if K > 1:
        assert (got_s > 0).all()                                             # generic members do not coincide


@pytest.mark.parametrize("K", KS)
def test_crystal_spread_is_the_sum_and_maximum_of_the_stored_spread(cases, K):
    _, _, res, _ = cases[K]
    cs, s = res.crystal_spread.cpu(), res.spread.cpu().double()
    assert cs.dtype == torch.float64 and tuple(cs.shape) == (B, 2)
    for g, n, sl in _per_crystal():
        if n == 0:
            assert cs[g].tolist() == [0.0, 0.0]
            continue
        assert np.allclose(cs[g, 0].item(), s[sl].sum().item(), rtol=1e-12, atol=0)      # only the order differs
        assert cs[g, 1].item() == s[sl].max().item()


@pytest.mark.parametrize("K", KS)
def test_two_runs_give_the_same_bytes_and_stats_are_optional(cases, K):
    from cartnet_amd import metrics as gm
    pred, rot, res, _ = cases[K]
    again = gm.frame_mean(pred, rot, _ptr())
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    part = gm.frame_mean(pred, rot, _ptr(), stats=False)
    assert part.crystal_spread is None and torch.equal(part.mean, res.mean) and torch.equal(part.spread, res.spread)


def test_one_identity_frame_returns_the_input():
    from cartnet_amd import metrics as gm
    pred = _tensors(M, 31).cuda()
    eye = torch.eye(3, device="cuda:0").repeat(1, B, 1, 1)
    res = gm.frame_mean(pred, eye, _ptr())
    assert torch.equal(res.mean, pred)
    assert torch.equal(res.spread, torch.zeros(M, device="cuda:0"))
    assert torch.equal(res.crystal_spread, torch.zeros(B, 2, dtype=torch.float64, device="cuda:0"))


def _equivariant_inputs(K, transposed):
    """V [M,3,3] fp64 (the values of fp32 SPD rows) and the members an equivariant model returns for frames R:
    P_k = R^T V R (or, transposed, R V R^T), formed in fp64 and rounded to fp32."""
    from cartnet_amd.shard import random_rotations
    gen = torch.Generator(device="cuda:0").manual_seed(17)
    rot = random_rotations(K * B, gen, "cuda:0").view(K, B, 3, 3)
    V = _tensors(M, 41).numpy().astype(np.float64)
    R = rot.cpu().numpy().astype(np.float64)[:, _crystal_of_row()]
    P = np.einsum("kmab,mbd,kmcd->kmac", R, V, R) if transposed else np.einsum("kmba,mbd,kmdc->kmac", R, V, R)
    return V, R, P, torch.from_numpy(P.astype(np.float32)).reshape(K * M, 3, 3).cuda(), rot


@pytest.mark.parametrize("K", [2, 7])
def test_an_equivariant_models_members_come_back_to_one_tensor(K):
    """The issue's bounds are 4 * 2^-24 max|V| for the mean and 8 * 2^-24 max|V| for the spread: 3 for a member's input
    rounding (|dP| <= 2^-24 max|P| per element, seen through R . R^T: two row sums of |R|, each <= sqrt(3)) plus 1 for the
    mean's own rounding, and twice a member's error for the spread.  Two things that derivation leaves out are added here,
    both computed from the inputs alone:
      mu    = max|P_k| / max|V| (>= 1 in general: a rotated tensor's largest element can exceed the stored one's, up to its
              largest principal value), which scales the input rounding: 3 mu instead of 3;
      delta = max|R R^T - I| of the fp32 rotations as given (they are not re-orthonormalised): in exact arithmetic the
              member comes back as (R R^T) V (R R^T) = V + E V + V E + E V E, elementwise within (6 delta + 9 delta^2) max|V|.
    So per crystal a member is within e = (3 mu 2^-24 + 6 delta + 9 delta^2) max|V| of V, the mean within e + 2^-24 max|V|
    (its rounding to fp32), the spread within 2 e (1 + 2^-24)."""
    from cartnet_amd import metrics as gm
    V, R, P, pred, rot = _equivariant_inputs(K, transposed=False)
    res = gm.frame_mean(pred, rot, _ptr())
    mean, spread = res.mean.cpu().numpy().astype(np.float64), res.spread.cpu().numpy().astype(np.float64)
    delta = np.abs(np.einsum("kmab,kmcb->kmac", R, R) - np.eye(3)).max(axis=(0, 2, 3))          # per row
    for g, n, sl in _per_crystal():
        if n == 0:
            continue
        vmax = np.abs(V[sl]).max()
        mu, d = np.abs(P[:, sl]).max() / vmax, delta[sl].max()
        e = (3 * mu * EPS24 + 6 * d + 9 * d * d) * vmax
        err_m, err_s = np.abs(mean[sl] - V[sl]).max(), spread[sl].max()
        print(f"K={K} crystal {g}: mu {mu:.3f}, delta {d:.3e}; mean off V by {err_m:.3e} (bound {e + EPS24 * vmax:.3e}, "
              f"nominal {4 * EPS24 * vmax:.3e}); spread {err_s:.3e} (bound {2 * e * (1 + EPS24):.3e}, nominal "
              f"{8 * EPS24 * vmax:.3e})")
        assert err_m <= e + EPS24 * vmax, (K, g)
        assert err_s <= 2 * e * (1 + EPS24), (K, g)


def test_the_transposed_convention_does_not_come_back():
    """Members R V R^T belong to the other convention (input R @ cart_dir): brought back as R P R^T they land on
    R R V R^T R^T, which generic rotations (no half turns: R R != I) keep well away from V.  This pins the direction."""
    from cartnet_amd import metrics as gm
    V, R, _, pred, rot = _equivariant_inputs(3, transposed=True)
    # every row has a frame that is far from a half turn (and from the identity)
    assert np.abs(np.einsum("kmab,kmbc->kmac", R, R) - np.eye(3)).max(axis=(0, 2, 3)).min() > 0.5
    res = gm.frame_mean(pred, rot, _ptr())
    off = np.abs(res.mean.cpu().numpy().astype(np.float64) - V).max()
    print(f"transposed members: mean off V by {off:.3e}, max|V| {np.abs(V).max():.3e}")
    assert off > 1e-3 * np.abs(V).max()
    assert float(res.spread.max()) > 1e-3 * np.abs(V).max()


def test_argument_checks():
    from cartnet_amd import metrics as gm
    pred = _tensors(2 * M, 3).cuda()
    rot = torch.eye(3, device="cuda:0").repeat(2, B, 1, 1)
    with pytest.raises(ValueError, match="rot must be"):
        gm.frame_mean(pred, rot[:, :B - 1], _ptr())
    with pytest.raises(ValueError, match="rot must be"):
        gm.frame_mean(pred, rot.double(), _ptr())
    with pytest.raises(ValueError, match="no multiple"):
        gm.frame_mean(pred[:-1], rot, _ptr())
    with pytest.raises(ValueError, match="pred must be"):
        gm.frame_mean(pred.double(), rot, _ptr())
    with pytest.raises(ValueError, match="row_ptr"):
        gm.frame_mean(pred, rot, _ptr().to(torch.int32))
    empty = gm.frame_mean(pred[:0], rot, torch.zeros(B + 1, dtype=torch.int64, device="cuda:0"))
    assert tuple(empty.mean.shape) == (0, 3, 3) and empty.crystal_spread.tolist() == [[0.0, 0.0]] * B
