"""Samplers (reference package: torchebm/samplers)."""

from .descent import GradientDescentSampler, NesterovSampler
from .hamiltonian import HamiltonianMonteCarlo
from .langevin import LangevinDynamics
from .tempering import ReplicaExchangeLangevin

__all__ = ["LangevinDynamics", "HamiltonianMonteCarlo", "GradientDescentSampler", "NesterovSampler",
           "ReplicaExchangeLangevin"]
