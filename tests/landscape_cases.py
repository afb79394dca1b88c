"""Inputs, float64 references, natural scales and bars for the three landscape energies (Rosenbrock, Ackley, Rastrigin)
of the fused kernels (csrc/landscape_energies.h).  Shared by tests/test_landscape_bars.py (CPU), tests/test_landscape_host.py
(CPU) and tests/test_landscape_gpu.py.

Float64 is the referee: the references below evaluate the model's formula in closed form with its Python-double parameters
on the fp32 inputs.  The yardstick is the package's own CPU path, ``model.forward`` / ``BaseModel.gradient`` in fp32 (the
reference's lines restated, autograd).  Errors are measured in units of ``U * N`` with ``U = 2^-24`` and ``N`` the natural
scale of the quantity: its formula with every term replaced by its absolute value and every rounding it goes through
counted once (per element for the gradient, per chain for the energy).
"""

import math
import zlib

import torch

import oracle
import torchebm_amd as ta  # noqa: F401
from torchebm_amd import core

U = 2.0 ** -24

ENERGIES = ("rosenbrock", "ackley", "rastrigin")

# Row widths that cover every lane geometry of rows.h pick_geometry: G = 1 ... 64 with one vector per lane, each with a
# masked width and the full one, then (64, 2) and (64, 4).
WIDTHS = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 100, 128, 129, 256, 257, 260, 512, 1000, 1024)
SCALES = (0.5, 5.0)  # x uniform in +-scale (Ackley's scale below has no term for |x| >> 5: kept inside)
N_ROWS = 300


def model(name, device=None):
    return {"rosenbrock": core.RosenbrockModel, "ackley": core.AckleyModel, "rastrigin": core.RastriginModel}[name](device=device)


def inputs(name, dim, scale, n=N_ROWS, salt=0):
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{dim}/{scale}/{salt}".encode()))
    return ((torch.rand(n, dim, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


# ----------------------------------------------------------------------------------------------------------------
# float64 references (closed forms) and natural scales
# ----------------------------------------------------------------------------------------------------------------
def energy64(name, m, x):
    x = x.double()
    n = x.shape[1]
    if name == "rastrigin":
        return m.a * n + (x * x - m.a * torch.cos(2 * math.pi * x)).sum(1)
    if name == "ackley":
        r = (x.square().sum(1) / n).sqrt()
        return -m.a * torch.exp(-m.b * r) - torch.exp(torch.cos(m.c * x).sum(1) / n) + m.a + math.e
    head, tail = x[:, :-1], x[:, 1:]
    return ((m.a - head) ** 2 + m.b * (tail - head ** 2) ** 2).sum(1)


def grad64(name, m, x):
    x = x.double()
    n = x.shape[1]
    if name == "rastrigin":
        return 2 * x + 2 * math.pi * m.a * torch.sin(2 * math.pi * x)
    if name == "ackley":
        r = (x.square().sum(1, keepdim=True) / n).sqrt()
        A = m.a * m.b * torch.exp(-m.b * r) / (n * r)
        B = m.c * torch.exp(torch.cos(m.c * x).sum(1, keepdim=True) / n) / n
        return A * x + B * torch.sin(m.c * x)
    g = torch.zeros_like(x)
    res = x[:, 1:] - x[:, :-1] ** 2
    g[:, :-1] += -2 * (m.a - x[:, :-1]) - 4 * m.b * x[:, :-1] * res
    g[:, 1:] += 2 * m.b * res
    return g


def natural(name, m, x):
    """(N_g [n, dim], N_E [n]) in float64."""
    x = x.double()
    n = x.shape[1]
    xa = x.abs()
    if name == "rastrigin":
        c = 2 * math.pi
        return 2 * xa + m.a * c * (1 + c * xa), m.a * n + (x * x + m.a).sum(1)
    if name == "ackley":
        r = (x.square().sum(1, keepdim=True) / n).sqrt()
        e1 = torch.exp(-m.b * r)
        e2 = torch.exp(torch.cos(m.c * x).sum(1, keepdim=True) / n)
        A = m.a * m.b * e1 / (n * r)
        B = m.c * e2 / n
        return A * xa * (2 + m.b * r) + B * (2 + m.c * xa), (m.a * e1 + e2 + m.a + math.e).squeeze(1)
    N = torch.zeros_like(x)
    ra = xa[:, 1:] + x[:, :-1] ** 2
    N[:, :-1] += 2 * (abs(m.a) + xa[:, :-1]) + 4 * m.b * xa[:, :-1] * ra
    N[:, 1:] += 2 * m.b * ra
    return N, ((abs(m.a) + xa[:, :-1]) ** 2 + m.b * ra ** 2).sum(1)


def errors(name, m, x, e_got, g_got):
    """Worst energy and gradient error of (e_got, g_got) against float64, in units of U * N."""
    ng, ne = natural(name, m, x)
    eg = ((g_got.double().cpu() - grad64(name, m, x)).abs() / (U * ng)).max().item()
    ee = ((e_got.double().cpu() - energy64(name, m, x)).abs() / (U * ne)).max().item()
    return ee, eg


def cpu32(m, x):
    """The yardstick: the package's CPU path in fp32."""
    return m.forward(x), m.gradient(x)


def degraded_grad(name, m, x):
    """A deliberately degraded evaluation: the float64 gradient of the inputs rounded to 16 significant bits."""
    mant, expo = torch.frexp(x.double())
    return grad64(name, m, torch.ldexp((mant * 65536).round() / 65536, expo).float())


# ----------------------------------------------------------------------------------------------------------------
# Bars.  CPU_WORST is the worst error the CPU fp32 path reaches over every (width, scale) of the inputs above, measured
# with tests/test_landscape_bars.py's own loop (torch 2 CPU kernels; that test allows another host's torch 1.5 x); the bar is twice that
# -- the kernel adds a row in another order than torch and may use another, equally valid, sine.  A bar loose enough to
# hide a 16-bit operand is caught by the degraded evaluation, whose worst element must fail it in every case.
# ----------------------------------------------------------------------------------------------------------------
CPU_WORST = {
    "rosenbrock": {"energy": 4.005, "grad": 3.898},  # degraded gradient, its best case: 319.7
    "ackley": {"energy": 1.106, "grad": 3.697},      # ... 64.1
    "rastrigin": {"energy": 6.359, "grad": 1.642},   # ... 96.6
}
BAR = {name: {q: 2.0 * w for q, w in d.items()} for name, d in CPU_WORST.items()}


# ----------------------------------------------------------------------------------------------------------------
# oracle adapter: oracle.hmc.leapfrog / oracle.langevin take any object with .energy(x) / .grad(x)
# ----------------------------------------------------------------------------------------------------------------
class Adapter:
    """fp32: the package model's forward / autograd gradient.  fp64: the closed forms above (on float64 states)."""

    def __init__(self, name, f64=False):
        self.name, self.m, self.f64 = name, model(name), f64

    def energy(self, x):
        if self.f64:
            return _energy64_raw(self.name, self.m, x)
        return self.m.forward(x)

    def grad(self, x):
        if self.f64:
            x = x.detach().double().requires_grad_(True)
            (g,) = torch.autograd.grad(_energy64_raw(self.name, self.m, x).sum(), x)
            return g
        return self.m.gradient(x)


def _energy64_raw(name, m, x):
    return m.forward(x.double())


# ----------------------------------------------------------------------------------------------------------------
# HMC accept decisions: a batch in which about half the chains have an acceptance probability below one
# ----------------------------------------------------------------------------------------------------------------
def accept_batch(name, dim, n_half=300):
    """Starts (x0, p) and their time reversals (x1, -p1), rounded to fp32, with eps halved from 0.1 until the median |dH|
    of the batch is below 2: one of each pair climbs in H, so about half the chains have a < 1 (arbitrary starts keep 0 - 38 %).
    Returns x [n, dim], p [n, dim] (fp32), eps and float64 (h0, h1, n0, n1)."""
    a64 = Adapter(name, f64=True)
    m = model(name)
    g = torch.Generator().manual_seed(1000 + dim)
    xs = inputs(name, dim, 0.5 if name != "rosenbrock" else 1.0, n=n_half, salt=9)
    ps = torch.randn(n_half, dim, generator=g)
    eps = 0.1
    for _ in range(30):
        x1, p1 = oracle.hmc.leapfrog(a64, xs.double(), ps.double(), eps, 1, None, safe=True)
        x = torch.cat([xs, x1.float()])
        p = torch.cat([ps, (-p1).float()])
        xe, pe = oracle.hmc.leapfrog(a64, x.double(), p.double(), eps, 1, None, safe=True)
        h0 = energy64(name, m, x) + 0.5 * p.double().square().sum(1)
        h1 = a64.energy(xe) + 0.5 * pe.square().sum(1)
        if (h1 - h0).abs().median().item() < 2.0:
            break
        eps = float(torch.tensor(eps * 0.5, dtype=torch.float32))
    n0 = natural(name, m, x)[1] + 0.5 * p.double().square().sum(1)
    n1 = natural(name, m, xe.float())[1] + 0.5 * pe.square().sum(1)
    return x, p, eps, (h0, h1, n0, n1)
