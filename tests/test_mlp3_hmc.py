"""The HMC transition entry of ``MLP3Energy`` on the host: name lists, a refusal that needs no GPU, the route of a CPU energy."""

import pathlib
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.core import MLP3Energy


def test_the_companion_header_declares_exactly_the_listed_entry():
    header = pathlib.Path(__file__).resolve().parents[1] / "include" / "ebm_hip_mlp3_hmc.h"
    declared = tuple(re.findall(r"EBM_API\s+\w+\s+(\w+)\s*\(", header.read_text()))
    assert declared == _lib.EXPORTS_MLP3_HMC == ("ebm_hmc_chain_mlp3_f32",)
    others = _lib.EXPORTS + _lib.EXPORTS_ADAPT + _lib.EXPORTS_ADAPT_MASS + _lib.EXPORTS_MLP3 + _lib.EXPORTS_MLP3_STREAM
    assert declared[0] in _lib._PROTOTYPES and hasattr(_lib.lib(), declared[0]) and declared[0] not in others


def test_a_null_state_is_refused_without_a_gpu():
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP3, 64, 16  # (never dereferenced: the refusal comes first)
    with pytest.raises(ValueError, match="state pointer is NULL"):
        _lib.call("ebm_hmc_chain_mlp3_f32", desc, None, 4, 2, 1, 1, 0.1, None, _lib.MASS_NONE, 1.0, 1, None, None, None, None, None,
                  0, 0, None)


def test_class_attribute_and_the_cpu_route():
    assert isinstance(MLP3Energy.HMC_MAX_DIM, dict) and set(MLP3Energy.HMC_MAX_DIM) == {64}
    sampler = ta.HamiltonianMonteCarlo(MLP3Energy(3, 64), step_size=0.1, n_leapfrog_steps=2)
    assert sampler._route(torch.zeros(5, 3), {}) == ("eager", None)
