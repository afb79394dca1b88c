"""Route pinning: every case of tests/chain_cases.py ROUTES launches the kernel family the map names (torch.profiler sees
the launches of libebm_hip.so).  A predicate that changes, or a branch put in front of another, moves cases to another
family -- this fails instead of the old family's tests quietly testing something else."""

import pytest
import torch

import chain_cases as cc
from helpers import launched_kernels

pytestmark = pytest.mark.gpu


def _families(names):
    return " ".join(cc.family_of(n) for n in names if "ebm::" in n)


@pytest.mark.parametrize("case", cc.ROUTES, ids=lambda c: c.id)
def test_route(cuda_device, case):
    _, spec, fp = cc.device_model(case, cuda_device)
    if case.sampler == "hmc":
        x0, p, mass = cc.hmc_inputs(case, fp)
        u = torch.zeros(case.n)
        with launched_kernels() as k:
            cc.run_hmc(case, spec, x0, p, u, mass, 0.01, cuda_device)
        assert _families(k.names) == case.family, k.names
        return
    x0 = cc.langevin_x0(case, fp)
    for noise_field, want in ((False, case.family), (True, case.family_noise or case.family)):
        with launched_kernels() as k:
            cc.run_langevin(case, spec, x0, 0.01, noise_field, cuda_device)
        assert _families(k.names) == want, (noise_field, k.names)
