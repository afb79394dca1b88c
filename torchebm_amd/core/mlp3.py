"""``MLP3Energy``: the three-hidden-layer SiLU MLP energy of the reference's energy-matching examples
(examples/20-training/04-energy-matching/01-energy-matching-2d/main.py:31-34), with a fused Langevin chain kernel and a
one-launch input gradient of its own (include/ebm_hip_mlp3.h, docs/design/mlp3.md)."""

from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .energies import BaseModel, FusedSpec, fused_spec_for


def _is_stack(net) -> bool:
    """``net`` is exactly ``Linear(d, H) - SiLU - Linear(H, H) - SiLU - Linear(H, H) - SiLU - Linear(H, 1)`` with biases."""
    from torch import nn

    if not isinstance(net, nn.Sequential) or len(net) != 7:
        return False
    lin, act = [net[i] for i in (0, 2, 4, 6)], [net[i] for i in (1, 3, 5)]
    if not all(type(l) is nn.Linear and l.bias is not None for l in lin) or not all(type(a) is nn.SiLU for a in act):
        return False
    hidden = lin[0].out_features
    return all(l.in_features == hidden for l in lin[1:]) and lin[1].out_features == lin[2].out_features == hidden and lin[3].out_features == 1


class MLP3Energy(BaseModel):
    r"""``E(x) = w_4^\top \mathrm{silu}(W_3\,\mathrm{silu}(W_2\,\mathrm{silu}(W_1 x + b_1) + b_2) + b_3) + b_4``.

    ``forward`` is ``self.net`` under plain autograd on every device and dtype, and training stays autograd.  On a CUDA device
    in fp32, with ``hidden == 64`` and ``in_dim <= 128`` or ``hidden == 128`` and ``in_dim <= 32``:

    * ``gradient()`` is one launch of ``ebm_energy_grad_mlp3_f32`` (forward and backward through all three hidden layers on the
      matrix cores), so every sampler's per-step route takes it;
    * ``LangevinDynamics.sample()`` is one launch of ``ebm_langevin_chain_mlp3_f32`` for the plain call (Euler-Maruyama, constant
      step size and noise scale, no clamp, trajectory or diagnostics, ``thin == 1``, no ``model_kwargs``); any other
      configuration takes the per-step route;
    * at ``hidden == 64``, ``HamiltonianMonteCarlo.sample()`` is one launch of ``ebm_hmc_chain_mlp3_f32``
      (include/ebm_hip_mlp3_hmc.h, docs/design/mlp3_hmc.md) with no mass or a scalar one, ``exact`` off and no diagnostics;
      ``thin``, ``return_trajectory`` and a scheduled step size stay in that launch;
    * at ``hidden == 64``, ``UnderdampedLangevin.sample()`` with the sampler's opt-in ``fused_mlp = True`` is one launch of
      ``ebm_kinetic_chain_mlp3_f32`` (include/ebm_hip_mlp3_kinetic.h, docs/design/mlp3_kinetic.md): BAOAB with no mass and a
      constant step size; ``thin``, ``return_trajectory``, ``return_diagnostics``, ``velocity=`` and ``return_velocity`` stay in
      that launch.  Without the opt-in, with a mass or a scheduled step size, and in ``sample_moments``, the sampler keeps its
      eager route with the one-launch gradient.

    At ``hidden == 128`` and ``33 <= in_dim <= 128`` both go through the streamed bf16 kernel instead
    (``ebm_energy_grad_mlp3_stream_f32`` / ``ebm_langevin_chain_mlp3_stream_f32``, include/ebm_hip_mlp3_stream.h,
    docs/design/mlp3_stream.md), whose spec carries a pre-split weight image in ``aux``; ``streamed_bf16 = True`` opts
    ``in_dim <= 32`` into that kernel as well.

    The parameters are ordinary ``nn.Linear`` weights, re-read (packed) at every call.
    """

    HIP_GRADIENT = True
    #: ``fused_spec_for`` forms this energy's spec only for a caller that asks for its kind (``mlp3=True``)
    FUSED_SPEC_ON_REQUEST = True
    #: hidden width -> widest input with a kernel (csrc/mlp3.hip: what is resident in LDS at each width)
    FUSED_MAX_DIM = {64: 128, 128: 32}
    #: hidden width -> widest input of the streamed bf16 kernel (csrc/mlp3_stream.hip), the only kernel above FUSED_MAX_DIM
    STREAMED_MAX_DIM = {128: 128}
    #: hidden width -> widest input of the HMC transition kernel (csrc/mlp3_hmc.hip; docs/design/mlp3_hmc.md: every width measured)
    HMC_MAX_DIM = {64: 128}
    #: hidden width -> widest input of the underdamped-Langevin kernel (csrc/mlp3_kinetic.hip; docs/design/mlp3_kinetic.md: every
    #: width measured)
    KINETIC_MAX_DIM = {64: 128}
    #: take the streamed bf16 kernel also where the exact-f32 kernel of FUSED_MAX_DIM serves (hidden 128, in_dim <= 32)
    streamed_bf16 = False
    ROWS_INDEPENDENT = True

    def __init__(self, in_dim: int = 2, hidden: int = 128, *args, **kwargs):
        super().__init__(*args, **kwargs)
        from torch import nn

        self.in_dim, self.hidden = in_dim, hidden
        self.net = nn.Sequential(
            nn.Linear(in_dim, hidden), nn.SiLU(), nn.Linear(hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden), nn.SiLU(),
            nn.Linear(hidden, 1),
        ).to(device=self._torchebm_probe.device, dtype=self._torchebm_probe.dtype)

    @classmethod
    def from_sequential(cls, net: "torch.nn.Sequential") -> "MLP3Energy":
        """Adopt a hand-written stack of this shape WITHOUT copying it: the returned energy shares ``net``'s parameters."""
        from torch import nn

        layers = list(net)
        ok = (
            len(layers) == 7
            and all(isinstance(layers[i], nn.Linear) for i in (0, 2, 4, 6))
            and all(isinstance(layers[i], nn.SiLU) for i in (1, 3, 5))
            and layers[0].out_features == layers[2].in_features == layers[2].out_features == layers[4].in_features
            == layers[4].out_features == layers[6].in_features
            and layers[6].out_features == 1
            and all(layers[i].bias is not None for i in (0, 2, 4, 6))
        )
        if not ok:
            raise ValueError(
                "expected nn.Sequential(Linear(d, H), SiLU(), Linear(H, H), SiLU(), Linear(H, H), SiLU(), Linear(H, 1)) with biases"
            )
        w = layers[0].weight
        self = cls(in_dim=layers[0].in_features, hidden=layers[0].out_features, device=w.device, dtype=w.dtype)
        self.net = net
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.net(x).squeeze(-1)

    def _plain_net(self) -> bool:
        """``self.net`` is the stack ``fused_spec`` packs, at the widths the kernels index it by, with nothing hooked into it."""
        n = self.net
        if type(self) is not MLP3Energy or not _is_stack(n):
            return False
        if n[0].in_features != self.in_dim or n[0].out_features != self.hidden:
            return False
        mods = (self, n, *n)
        return not any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None)
                       for m in mods)

    def fused_spec(self) -> Optional[FusedSpec]:
        resident = 1 <= self.in_dim <= self.FUSED_MAX_DIM.get(self.hidden, 0)
        streamed = 1 <= self.in_dim <= self.STREAMED_MAX_DIM.get(self.hidden, 0) and (self.streamed_bf16 or not resident)
        if not self._is_exactly(MLP3Energy) or not (resident or streamed):
            return None
        if not self._plain_net():
            return None
        params = [p for i in (0, 2, 4, 6) for p in (self.net[i].weight, self.net[i].bias)]
        if not all(p.is_cuda and p.dtype == torch.float32 and p.device == params[0].device for p in params):
            return None
        with torch.no_grad():  # W1[H,d] b1[H] W2[H,H] b2[H] W3[H,H] b3[H] w4[H] b4[1], packed on every call: the weights train
            packed = torch.cat([p.detach().reshape(-1) for p in params])
            image = None
            if streamed:  # the pre-split image of W1 and W3 the streamed kernel walks: rebuilt with `packed`, i.e. on every call
                n_img = int(_lib.lib().ebm_mlp3_image_bytes(int(self.hidden), int(self.in_dim)))
                image = torch.empty(n_img // 4, dtype=torch.int32, device=packed.device)
                _lib.call("ebm_mlp3_image_f32", packed.data_ptr(), int(self.hidden), int(self.in_dim), image.data_ptr(),
                          _lib.stream_handle(packed.device))
        return FusedSpec(_lib.ENERGY_MLP3, n_comp=int(self.hidden), dev0=packed, aux=image, langevin_only=True, dim=int(self.in_dim),
                         hmc=image is None and self.in_dim <= self.HMC_MAX_DIM.get(self.hidden, 0),
                         kinetic=image is None and self.in_dim <= self.KINETIC_MAX_DIM.get(self.hidden, 0))

    def _hip_gradient(self, x: torch.Tensor, model_kwargs: Optional[dict]) -> Optional[torch.Tensor]:
        """``gradient()`` in one ``ebm_energy_grad_mlp3_f32`` launch (``ebm_energy_grad_mlp3_stream_f32`` when the spec carries an
        image) under the conditions ``MLPEnergy.gradient`` uses (fp32 ``[n, dim]`` CUDA state, no kwargs, no autocast); ``None``
        sends the caller to autograd."""
        if model_kwargs or not x.is_cuda or x.dtype != torch.float32 or x.ndim != 2:
            return None
        if torch.is_autocast_enabled() or getattr(self, "use_mixed_precision", False):
            return None
        spec = fused_spec_for(self, x, None, mlp3=True)
        if spec is None:
            return None
        state = x.detach().contiguous()
        if state.data_ptr() % 16 != 0 or state.shape[0] == 0:
            return None
        grad = torch.empty_like(state)
        entry = "ebm_energy_grad_mlp3_f32" if spec.aux is None else "ebm_energy_grad_mlp3_stream_f32"
        _lib.call(entry, spec.to_c(), state.data_ptr(), state.shape[0], state.shape[1], None, grad.data_ptr(),
                  _lib.stream_handle(state.device))
        return grad
