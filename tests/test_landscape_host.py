"""Host side of the fused landscape energies (Rosenbrock, Ackley, Rastrigin): descriptors, ABI constants and the argument
checks of the C entries that need no launch.  CPU only."""

import ctypes
import math
import os
import re

import pytest
import torch

from torchebm_amd import _lib
from torchebm_amd.core import AckleyModel, RastriginModel, RosenbrockModel
from torchebm_amd.core.energies import fused_spec_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBM_EKIND, EBM_EDIM, EBM_EINVAL = -2, -3, -1


def test_fused_specs_carry_the_documented_kind_and_scalars():
    s = RosenbrockModel(a=1.5, b=80.0).fused_spec()
    assert s is not None and s.kind == _lib.ENERGY_ROSENBROCK == 5 and tuple(s.scalars)[:2] == (1.5, 80.0)
    s = AckleyModel(a=10.0, b=0.3, c=2.0).fused_spec()
    assert s is not None and s.kind == _lib.ENERGY_ACKLEY == 6 and tuple(s.scalars)[:3] == (10.0, 0.3, 2.0)
    assert tuple(AckleyModel().fused_spec().scalars)[:3] == (20.0, 0.2, 2 * math.pi)
    s = RastriginModel(a=7.0).fused_spec()
    assert s is not None and s.kind == _lib.ENERGY_RASTRIGIN == 7 and tuple(s.scalars)[0] == 7.0
    for spec in (RosenbrockModel().fused_spec(), AckleyModel().fused_spec(), RastriginModel().fused_spec()):
        assert not spec.elementwise and spec.dev0 is None and spec.dev1 is None and spec.aux is None and spec.hmc
        assert not spec.langevin_only


def test_gradient_stays_autograd():
    for cls in (RosenbrockModel, AckleyModel, RastriginModel):
        assert cls.HIP_GRADIENT is False


@pytest.mark.parametrize("cls", [RosenbrockModel, AckleyModel, RastriginModel])
def test_a_subclass_that_overrides_forward_or_gradient_is_not_fused(cls):
    class Fwd(cls):
        def forward(self, x):
            return super().forward(x) + 1.0

    class Grad(cls):
        def gradient(self, x, model_kwargs=None):
            return super().gradient(x, model_kwargs)

    class Same(cls):
        pass

    assert Fwd().fused_spec() is None and Grad().fused_spec() is None
    assert Same().fused_spec() is not None


def test_widths_the_fused_route_takes():
    ros, ack = RosenbrockModel(), AckleyModel()
    assert fused_spec_for(ros, torch.zeros(3, 1), None) is None  # the step route raises the reference's ValueError
    assert fused_spec_for(ros, torch.zeros(3, 2), None) is not None
    assert fused_spec_for(ack, torch.zeros(3, 1), None) is not None
    for m in (ros, ack, RastriginModel()):
        assert fused_spec_for(m, torch.zeros(2, 1024), None, cap_elementwise=False) is not None
        assert fused_spec_for(m, torch.zeros(2, 1025), None, cap_elementwise=False) is None  # FUSED_MAX_ROW applies
    with pytest.raises(ValueError):
        ros.forward(torch.zeros(3, 1))


def test_header_enum_matches_the_python_constants():
    text = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    enum = dict(re.findall(r"\b(EBM_ENERGY_[A-Z_]+)\s*=\s*(\d+)", text))
    want = {"EBM_ENERGY_DOUBLE_WELL": _lib.ENERGY_DOUBLE_WELL, "EBM_ENERGY_HARMONIC": _lib.ENERGY_HARMONIC,
            "EBM_ENERGY_GAUSSIAN": _lib.ENERGY_GAUSSIAN, "EBM_ENERGY_GMM": _lib.ENERGY_GMM, "EBM_ENERGY_MLP": _lib.ENERGY_MLP,
            "EBM_ENERGY_ROSENBROCK": _lib.ENERGY_ROSENBROCK, "EBM_ENERGY_ACKLEY": _lib.ENERGY_ACKLEY,
            "EBM_ENERGY_RASTRIGIN": _lib.ENERGY_RASTRIGIN}
    assert {k: int(v) for k, v in enum.items()} == want
    assert int(re.search(r"#define EBM_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 9


def _desc(kind, scalars=(1.0, 100.0, 0.0, 0.0)):
    d = _lib.EnergyDesc()
    d.kind = kind
    for i, v in enumerate(scalars):
        d.s[i] = v
    return d


def _langevin(desc, x_ptr, dim):
    fn = _lib.lib().ebm_langevin_chain_f32
    rc = fn(ctypes.byref(desc), x_ptr, 4, dim, 1, 0.01, 0.1, 1.0, None, 0, 0.0, 0.0, 1, None, None, None, 0, 0, None)
    return rc, _lib.lib().ebm_last_error_string().decode()


@pytest.mark.parametrize("kind", [5, 6, 7])
def test_chain_entry_knows_the_kinds_before_any_launch(kind):
    rc, msg = _langevin(_desc(kind), None, 8)
    assert rc == EBM_EINVAL and "state pointer is NULL" in msg, (rc, msg)


def test_unknown_kind_is_still_refused():
    rc, msg = _langevin(_desc(77), None, 8)
    assert rc == EBM_EKIND and "unknown energy kind" in msg, (rc, msg)
    rc, msg = _langevin(_desc(8), None, 8)
    assert rc == EBM_EKIND and "unknown energy kind" in msg, (rc, msg)


def test_rosenbrock_needs_two_dimensions_before_any_launch():
    rc, msg = _langevin(_desc(5), None, 1)
    assert rc == EBM_EDIM, (rc, msg)
    lib = _lib.lib()
    d = _desc(5)
    assert lib.ebm_energy_grad_f32(ctypes.byref(d), None, 4, 1, None, None, None) == EBM_EDIM
    assert lib.ebm_energy_grad_f32(ctypes.byref(d), None, 4, 2, None, None, None) == EBM_EINVAL  # NULL state, kind and dim accepted
    d = _desc(7)
    assert lib.ebm_energy_grad_f32(ctypes.byref(d), None, 4, 1, None, None, None) == EBM_EINVAL


def test_audit_entry_keeps_refusing_the_landscapes():
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15  # host memory: the entry refuses the kind before anything reads it
    for kind in (5, 6, 7):
        d = _desc(kind)
        rc = lib.ebm_hmc_chain_audit_f32(ctypes.byref(d), ctypes.c_void_p(addr), 2, 4, 1, 1, 0.1, None, 0, 1.0, None, 1, None, None,
                                         None, None, None, 0, 0, None)
        assert rc == EBM_EKIND, (kind, rc, lib.ebm_last_error_string())
