"""The one-node module's argument list (``xdot.models.fused.AttnBlockFn``): the tuple of names its
backward indexes by is the forward's signature, and each parameter's gradient comes back in that
parameter's own slot -- freezing one parameter leaves its ``.grad`` None and every other gradient
as it was."""
import inspect

import pytest
import torch

B, T, DIM, H, HG = 1, 8, 16, 4, 2  # head dim 4: the smallest even one with two gathered groups
TOL = 1e-11  # the figure tests/test_gate.py holds the same fp64 module comparisons to


def test_names_are_the_forward_signature():
    from xdot.models import fused

    params = list(inspect.signature(fused.AttnBlockFn.forward).parameters)
    assert params[0] == "ctx"
    assert tuple(params[1:]) == fused.ARG_NAMES
    assert len(set(fused.ARG_NAMES)) == len(fused.ARG_NAMES)


def _module():
    import xdot

    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(DIM, num_heads=H, distributed=False, impl="flash", add_bias=True,
                                       num_gathered_heads=HG, rope=xdot.Rotary(), qk_norm=True, sinks=True,
                                       gate="headwise").double()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():  # off their initial values: ones / zeros hide a swapped pair
        m.keys_norm.weight.copy_(torch.rand(DIM // H, dtype=torch.float64, generator=gen) + 0.5)
        m.queries_norm.weight.copy_(torch.rand(DIM // H, dtype=torch.float64, generator=gen) + 0.5)
        m.sinks.copy_(torch.rand(H, dtype=torch.float64, generator=gen) * 2 - 1)
    return m


def _step(m, x, spec):
    for p in m.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    out = m(xr, xr, xr, spec)
    assert type(out.grad_fn).__name__ == "AttnBlockFnBackward"  # the one-node path ran
    out.pow(2).mean().backward()
    return xr.grad, {n: p.grad for n, p in m.named_parameters()}


def test_freezing_one_parameter_moves_no_other_gradient(monkeypatch):
    import xdot
    from xdot.utils.env import FLAGS

    monkeypatch.setattr(FLAGS, "fused_module", True)
    m = _module()
    names = [n for n, _ in m.named_parameters()]
    assert sorted(names) == sorted(["keys.weight", "keys.bias", "queries.weight", "queries.bias", "values.weight",
                                    "values.bias", "composition.weight", "composition.bias", "keys_norm.weight",
                                    "queries_norm.weight", "sinks", "gate.weight", "gate.bias"])
    x = torch.randn(B, T, DIM, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    spec = xdot.StructuredMask(causal=True)
    dx0, g0 = _step(m, x, spec)
    assert all(g is not None and float(g.abs().max()) > 0 for g in g0.values())
    for frozen in names:
        p = dict(m.named_parameters())[frozen]
        p.requires_grad_(False)
        dx, g = _step(m, x, spec)
        p.requires_grad_(True)
        assert g[frozen] is None, frozen
        torch.testing.assert_close(dx, dx0, rtol=TOL, atol=TOL, msg=lambda s: f"dx, {frozen} frozen: {s}")
        for n in names:
            if n != frozen:
                assert g[n] is not None, (n, frozen)
                torch.testing.assert_close(g[n], g0[n], rtol=TOL, atol=TOL, msg=lambda s: f"d{n}, {frozen} frozen: {s}")
