"""``MLP3Energy`` on the host: the wrapped stack, adoption of a hand-written one, and the routes a CPU energy takes."""

import pytest
import torch
from torch import nn

import torchebm_amd as ta
from torchebm_amd.core import MLP3Energy


def _stack(d=3, h=16, act=nn.SiLU, bias=True, h2=None, out=1):
    h2 = h if h2 is None else h2
    return nn.Sequential(nn.Linear(d, h), act(), nn.Linear(h, h2), act(), nn.Linear(h2, h2), act(), nn.Linear(h2, out, bias=bias))


def test_forward_is_the_sequential_it_wraps():
    torch.manual_seed(0)
    model = MLP3Energy(5, 32)
    x = torch.randn(9, 5)
    assert [type(m) for m in model.net] == [nn.Linear, nn.SiLU] * 3 + [nn.Linear]
    assert torch.equal(model(x), model.net(x).squeeze(-1))
    assert torch.equal(model.double()(x.double()), model.net(x.double()).squeeze(-1))
    assert ta.MLP3Energy is MLP3Energy


def test_from_sequential_shares_the_parameters():
    net = _stack()
    model = MLP3Energy.from_sequential(net)
    assert model.net is net and (model.in_dim, model.hidden) == (3, 16)
    assert {id(p) for p in model.parameters()} == {id(p) for p in net.parameters()}
    with pytest.raises(ValueError):  # the two-layer class keeps refusing seven modules
        ta.MLPEnergy.from_sequential(net)


@pytest.mark.parametrize("net", [
    nn.Sequential(nn.Linear(3, 16), nn.SiLU(), nn.Linear(16, 16), nn.SiLU(), nn.Linear(16, 1)),  # wrong length
    _stack(act=nn.ReLU), _stack(bias=False), _stack(h2=24), _stack(out=2),
], ids=["length", "activation", "bias", "widths", "last-width"])
def test_from_sequential_refuses_other_stacks(net):
    with pytest.raises(ValueError, match="expected nn.Sequential"):
        MLP3Energy.from_sequential(net)


@pytest.mark.parametrize("in_dim,hidden", [(2, 64), (129, 64), (33, 128), (8, 96)])
def test_fused_spec_is_none_on_cpu_and_outside_the_table(in_dim, hidden):
    model = MLP3Energy(in_dim, hidden)
    assert model.fused_spec() is None  # CPU parameters
    assert (in_dim <= MLP3Energy.FUSED_MAX_DIM.get(hidden, 0)) == ((in_dim, hidden) == (2, 64))


def test_langevin_on_cpu_is_the_per_step_route_of_the_reference_update():
    torch.manual_seed(1)
    model = MLP3Energy(3, 16)
    x0 = torch.randn(11, 3)
    eta, sigma, k = 0.05, 0.7, 5
    out = ta.LangevinDynamics(model, step_size=eta, noise_scale=sigma).sample(x=x0, n_steps=k, generator=torch.Generator().manual_seed(2))
    g, want = torch.Generator().manual_seed(2), x0
    for _ in range(k):
        z = torch.randn(want.shape, generator=g)
        want = (want - eta * model.gradient(want)) + (2.0 * sigma**2) ** 0.5 * (z * eta**0.5)
    torch.testing.assert_close(out, want, rtol=1e-6, atol=1e-6)
