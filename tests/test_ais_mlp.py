"""ebm_ais_mlp_chain_f32 and the ``fused_mlp`` opt-in of AnnealedImportanceSampling without a GPU: the export and its
declaration, the refusals the entry makes in front of any device access, and the opt-in's default and CPU behaviour."""

import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib

ENTRY = "ebm_ais_mlp_chain_f32"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ebm_hip.h")


def test_the_entry_is_exported_and_declared():
    assert ENTRY in _lib.EXPORTS and ENTRY in _lib._PROTOTYPES
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES["ebm_ais_chain_f32"]  # the same parameter list
    with open(HEADER) as fh:
        assert re.search(r"EBM_API\s+int\s+" + ENTRY + r"\s*\(", fh.read())
    assert _lib.ABI_VERSION == 9
    assert hasattr(_lib.lib(), ENTRY)


def _abi_call(desc, x=16, logw=16, dim=32, T=3, L=2, beta=16, eps=16, x0=None, p=None, u=None):
    _lib.call(ENTRY, desc, x, logw, 8, dim, T, L, beta, eps, 1.0, 1.0, None, None, x0, p, u, 0, 0, None)


def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any device access (the pointers below are never dereferenced)."""
    desc = _mlp_desc(64)
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None)
    with pytest.raises(ValueError, match="state pointer is NULL"):
        _abi_call(desc, x=None)
    with pytest.raises(ValueError, match="logw is NULL"):
        _abi_call(desc, logw=None)
    with pytest.raises(ValueError, match="beta / eps is NULL"):
        _abi_call(desc, beta=None)
    with pytest.raises(ValueError, match="beta / eps is NULL"):
        _abi_call(desc, eps=None)
    with pytest.raises(ValueError, match="n_temps=0"):
        _abi_call(desc, T=0)
    with pytest.raises(ValueError, match="n_leapfrog=0"):
        _abi_call(desc, L=0)
    for given in [dict(x0=16), dict(p=16), dict(u=16), dict(x0=16, p=16), dict(x0=16, u=16), dict(p=16, u=16)]:
        with pytest.raises(ValueError, match="must be given together"):  # EBM_EINVAL
            _abi_call(desc, **given)
    other = _lib.EnergyDesc()
    other.kind = _lib.ENERGY_DOUBLE_WELL
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):  # EBM_EKIND
        _abi_call(other)
    with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 32"):  # EBM_EDIM
        _abi_call(_mlp_desc(96))
    with pytest.raises(RuntimeError, match=r"code -3.*1 <= dim <= 128.*got 64, 129"):  # EBM_EDIM
        _abi_call(desc, dim=129)
    with pytest.raises(RuntimeError, match=r"code -3.*got 128, 0"):  # EBM_EDIM
        _abi_call(_mlp_desc(128), dim=0)
    # ebm_ais_chain_f32 is untouched: it still refuses the MLP
    with pytest.raises(RuntimeError, match=r"code -2.*no annealed-importance-sampling kernel"):
        _lib.call("ebm_ais_chain_f32", desc, 16, 16, 8, 32, 3, 2, 16, 16, 1.0, 1.0, None, None, None, None, None, 0, 0, None)


def test_the_opt_in_is_off_by_default_and_changes_nothing_on_the_cpu():
    assert ta.AnnealedImportanceSampling.fused_mlp is False
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    kw = dict(n_temperatures=5, schedule="sigmoid", step_size=0.2, n_leapfrog_steps=3, base_std=1.2)
    plain = ta.AnnealedImportanceSampling(model, **kw)
    opted = ta.AnnealedImportanceSampling(model, **kw)
    assert plain.fused_mlp is False
    opted.fused_mlp = True
    assert plain._route(4)[0] == "eager" and opted._route(4)[0] == "eager"  # CPU instances
    a = plain.run(48, 4, generator=torch.Generator().manual_seed(9))
    b = opted.run(48, 4, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a.log_weights, b.log_weights) and torch.equal(a.samples, b.samples)
    assert torch.equal(a.acceptance_rate, b.acceptance_rate) and a.log_z == b.log_z
    assert torch.isfinite(a.log_weights).all()
