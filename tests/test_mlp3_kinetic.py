"""The underdamped-Langevin entry of ``MLP3Energy`` on the host: name lists, a refusal that needs no GPU, the route of a CPU energy."""

import pathlib
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib
from torchebm_amd.core import MLP3Energy

ENTRY = "ebm_kinetic_chain_mlp3_f32"


def test_the_companion_header_declares_exactly_the_listed_entry():
    header = pathlib.Path(__file__).resolve().parents[1] / "include" / "ebm_hip_mlp3_kinetic.h"
    declared = tuple(re.findall(r"EBM_API\s+\w+\s+(\w+)\s*\(", header.read_text()))
    assert declared == _lib.EXPORTS_MLP3_KINETIC == (ENTRY,)
    others = (_lib.EXPORTS + _lib.EXPORTS_ADAPT + _lib.EXPORTS_ADAPT_MASS + _lib.EXPORTS_MLP3 + _lib.EXPORTS_MLP3_STREAM
              + _lib.EXPORTS_MLP3_HMC)
    assert _lib._PROTOTYPES[ENTRY] == _lib._PROTOTYPES["ebm_kinetic_mlp_chain_f32"]
    assert hasattr(_lib.lib(), ENTRY) and ENTRY not in others


def test_a_null_state_is_refused_without_a_gpu():
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP3, 64, 16  # (never dereferenced: the refusal comes first)
    for x, v, what in ((None, 16, "state"), (16, None, "velocity")):
        with pytest.raises(ValueError, match=what + " pointer is NULL"):
            _lib.call(ENTRY, desc, x, v, 4, 2, 1, 0.1, 1.0, 1.0, 0, 1, None, None, 0, 0, None)


def test_class_attribute_and_the_cpu_route():
    assert isinstance(MLP3Energy.KINETIC_MAX_DIM, dict) and set(MLP3Energy.KINETIC_MAX_DIM) == {64}
    model, x = MLP3Energy(3, 64), torch.randn(5, 3)
    plain, opted = (ta.UnderdampedLangevin(model, step_size=0.1, friction=1.5, temperature=0.8) for _ in range(2))
    opted.fused_mlp = True
    assert opted._route(x) == ("eager", None)
    runs = [s.sample(x=x, n_steps=3, return_velocity=True, generator=torch.Generator().manual_seed(1)) for s in (plain, opted)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
