"""Samplers (reference package: torchebm/samplers)."""

from .adapt import StepSizeAdaptation
from .ais import AISResult, AnnealedImportanceSampling
from .descent import GradientDescentSampler, NesterovSampler
from .ghmc import GeneralizedHMC
from .hamiltonian import HamiltonianMonteCarlo
from .kinetic import UnderdampedLangevin
from .langevin import LangevinDynamics
from .moments import ChainMoments, RunningMoments
from .tempering import ReplicaExchangeHMC, ReplicaExchangeLangevin
from .warmup import Warmup

__all__ = ["LangevinDynamics", "HamiltonianMonteCarlo", "GradientDescentSampler", "NesterovSampler",
           "ReplicaExchangeLangevin", "ReplicaExchangeHMC", "AnnealedImportanceSampling", "AISResult", "ChainMoments", "RunningMoments",
           "UnderdampedLangevin", "GeneralizedHMC", "StepSizeAdaptation", "Warmup"]
