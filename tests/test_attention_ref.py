"""The shared torch reference of the flash and ring paths (xdot/parallel/_ref.py): its gradients
against autograd of a dense softmax attention, and the exactness of splitting the columns."""
import pytest
import torch

B, R, T, H, DH, DV, SCALE = 2, 5, 7, 2, 4, 6, 0.3
TOL = dict(rtol=1e-12, atol=1e-12)  # fp64 round-off on sums of at most 7 terms


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(11)
    k = torch.randn(B, R, H * DH, generator=g, dtype=torch.float64)
    q = torch.randn(B, T, H * DH, generator=g, dtype=torch.float64)
    v = torch.randn(B, T, H * DV, generator=g, dtype=torch.float64)
    do = torch.randn(B, R, H * DV, generator=g, dtype=torch.float64)
    mask = torch.rand(B, R, T, generator=g) < 0.4
    mask[..., 5] = False                        # every row alive, also within the segment [3, 7)
    return k, q, v, do, mask


def _dense(k, q, v, mask):
    """softmax(mask(k qᵀ·scale)) v per head -> (out (B, R, H*DV), lse (B, H, R))"""
    kh = k.view(B, R, H, DH).transpose(1, 2)
    qh = q.view(B, T, H, DH).transpose(1, 2)
    vh = v.view(B, T, H, DV).transpose(1, 2)
    s = (kh @ qh.transpose(-1, -2) * SCALE).masked_fill(mask.unsqueeze(1), -float("inf"))
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, R, H * DV), s.logsumexp(-1)


def test_block_fwd_bwd_match_autograd(case):
    from xdot.parallel import _ref

    k, q, v, do, mask = case
    ka, qa, va = (t.clone().requires_grad_(True) for t in (k, q, v))
    ref_o, ref_lse = _dense(ka, qa, va, mask)
    ref_o.backward(do)
    o, lse = _ref.block_fwd(k, q, v, mask, H, SCALE)
    torch.testing.assert_close(o, ref_o.detach(), **TOL)
    torch.testing.assert_close(lse, ref_lse.detach(), **TOL)
    dk, dq, dv = _ref.block_bwd(do, k, q, v, lse, _ref.delta(do, o, H, torch.float64), mask, H, SCALE)
    torch.testing.assert_close(dk, ka.grad, **TOL)
    torch.testing.assert_close(dq, qa.grad, **TOL)
    torch.testing.assert_close(dv, va.grad, **TOL)


def _partials(k, q, v, mask):
    from xdot.parallel import _ref

    return [_ref.block_fwd(k, q[:, a:b], v[:, a:b], mask[..., a:b], H, SCALE) for a, b in ((0, 3), (3, 7))]


def test_column_split_is_exact(case):
    from xdot.parallel import _ref

    k, q, v, _, mask = case
    mask = mask.clone()
    mask[0, 2, :3] = True                       # a row the first segment masks entirely
    parts = _partials(k, q, v, mask)
    o0, l0 = parts[0]
    assert (o0[0, 2] == 0).all() and (l0[0, :, 2] == -float("inf")).all()
    whole_o, whole_lse = _ref.block_fwd(k, q, v, mask, H, SCALE)
    o, lse = _ref.combine(parts, torch.float64)
    torch.testing.assert_close(o, whole_o, **TOL)
    torch.testing.assert_close(lse, whole_lse, **TOL)


def test_fully_masked_row_is_nan(case):
    from xdot.parallel import _ref

    k, q, v, _, mask = case
    mask = mask.clone()
    mask[1, 3, :] = True
    o, lse = _ref.combine(_partials(k, q, v, mask), torch.float64)
    dead = torch.zeros(B, R, dtype=torch.bool)
    dead[1, 3] = True
    assert torch.isnan(o[dead]).all() and torch.isfinite(o[~dead]).all()
    assert (lse[1, :, 3] == -float("inf")).all()
