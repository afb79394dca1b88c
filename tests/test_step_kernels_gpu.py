"""The step-route entries called directly on the GPU, entry by entry, against the restatements of step_cases.py: every state
bit for bit (`same_bits`: torch.equal on the bit patterns), at the sizes where their launches change -- the ragged float4 tail,
the two kernels behind ebm_langevin_step_f32, the second trip of every grid-stride loop -- with the aliasing the header allows,
the accept rule's edges, the safe mode and mass forms of the kicks, and the RNG coordinates read from device memory.

Every call runs through `Call`: outputs start from FILL in front of GUARD floats of FILL, inputs are kept in a second copy; after
the call the guards must hold FILL and every input its bits."""

import numpy as np
import pytest
import torch

import oracle
from oracle.hmc import leapfrog
from torchebm_amd import _lib
from helpers import hip_calls
import step_cases as sc
from step_cases import same_bits

gpu = pytest.mark.gpu
FILL = 7.0
GUARD = 64  # elements behind every output that must keep FILL
SEED = 0x1234567887654321
ELEM_SIZES = sc.SMALL + (sc.BIG_ELEM,)
GROUP_SIZES = sc.SMALL + sc.BIG_GROUPS


def _guarded(dev, numel, src=None, dtype=torch.float32):
    """`numel` elements in front of GUARD elements of FILL (one allocation) -> (tensor, guard)."""
    buf = torch.full((numel + GUARD,), int(FILL) if dtype != torch.float32 else FILL, device=dev, dtype=dtype)
    t = buf[:numel]
    if src is not None:
        t.copy_(src.reshape(-1))
    return t, buf[numel:]


class Call:
    """The buffers of one call of an entry."""

    def __init__(self, dev):
        self.dev, self.inputs, self.guards = dev, [], []
        self.stream = _lib.stream_handle(dev)

    def inp(self, t):
        """A read-only input on the device (None stays None)."""
        if t is None:
            return None
        d = t.to(self.dev).contiguous()
        self.inputs.append((d, d.clone()))
        return d

    def out(self, numel, src=None, dtype=torch.float32):
        """An output (or, with `src`, an in/out buffer) in front of a guard."""
        t, g = _guarded(self.dev, numel, src, dtype)
        self.guards.append(g)
        return t

    def run(self, entry, *args, launches=1):
        before = hip_calls(entry)
        _lib.call(entry, *args, self.stream)
        torch.cuda.synchronize()
        assert hip_calls(entry) == before + launches
        for g in self.guards:
            assert bool((g == FILL).all()), f"{entry} wrote behind an output"
        for d, keep in self.inputs:
            bits = torch.int32 if d.dtype == torch.float32 else d.dtype
            assert torch.equal(d.view(bits), keep.view(bits)), f"{entry} changed an input"


def _written(*outs):
    for t in outs:
        assert not bool((t == FILL).any()), "an output slot was not written"


def rng_state(dev, seed, step):
    return torch.tensor([seed, step], dtype=torch.int64, device=dev)


def field(dev, n, kind, seed, step):
    """What ebm_noise_fill_f32 materialises (on the device)."""
    c = Call(dev)
    out = c.out(n)
    c.run("ebm_noise_fill_f32", out.data_ptr(), n, kind, seed, step)
    _written(out)
    return out


# ---------------------------------------------------------------------------------
# Langevin step
# ---------------------------------------------------------------------------------
def langevin(dev, x, grad, noise, coef=sc.NOISE_COEF, clamp=None, seed=0, offset=0, alias=False, state=None):
    """One call of ebm_langevin_step_f32 (or, with `state` = (seed, step) in device memory, of the _dev form) -> out on the CPU."""
    n, c = x.numel(), Call(dev)
    if alias:
        xd = out = c.out(n, x)
    else:
        xd, out = c.inp(x), c.out(n)
    gd, nd = c.inp(grad), c.inp(noise)
    cl = (0, 0.0, 0.0) if clamp is None else (1, clamp[0], clamp[1])
    if state is None:
        c.run("ebm_langevin_step_f32", xd.data_ptr(), _lib.ptr(gd), out.data_ptr(), _lib.ptr(nd), n, sc.ETA, sc.SQRT_ETA, coef, *cl,
              seed, offset)
    else:
        st = c.inp(rng_state(dev, *state))
        c.run("ebm_langevin_step_dev_f32", xd.data_ptr(), _lib.ptr(gd), out.data_ptr(), n, sc.ETA, sc.SQRT_ETA, coef, *cl,
              st.data_ptr())
    _written(out)
    return out.cpu()


@gpu
@pytest.mark.parametrize("n", GROUP_SIZES)
def test_langevin_step_is_the_restatement(cuda_device, n):
    c = sc.elem_case(n)
    for clamp in (None, sc.CLAMP):
        for grad in (c["grad"], None):
            for coef in (sc.NOISE_COEF, 0.0):
                got = langevin(cuda_device, c["x"], grad, c["noise"], coef, clamp)
                want = sc.langevin_step(c["x"], grad, c["noise"], sc.ETA, sc.SQRT_ETA, coef, clamp)
                assert same_bits(got, want), (clamp, grad is None, coef)


@gpu
@pytest.mark.parametrize("n", [1025, 1028])
def test_langevin_clamp_edges(cuda_device, n):
    c = sc.elem_case(n)
    x = c["x"].clone()
    x[0], x[1], x[2], x[n - 1], x[n - 2] = float("nan"), float("inf"), -float("inf"), float("nan"), float("inf")
    for clamp in (sc.CLAMP, (0.25, 0.25)):
        got = langevin(cuda_device, x, c["grad"], c["noise"], clamp=clamp)
        want = sc.langevin_step(x, c["grad"], c["noise"], sc.ETA, sc.SQRT_ETA, sc.NOISE_COEF, clamp)
        assert same_bits(got, want)
        assert torch.isnan(got[0]) and torch.isnan(got[n - 1]) and got[1] == clamp[1] and got[2] == clamp[0]
    assert bool((got[3:n - 2] == 0.25).all())


@gpu
@pytest.mark.parametrize("n", GROUP_SIZES)
def test_langevin_native_draw_is_the_field(cuda_device, n):
    c, (seed, offset) = sc.elem_case(n), (SEED, (3 << 32) + 5)
    eps = field(cuda_device, n, _lib.NOISE_NORMAL, seed, offset).cpu()
    for clamp in (None, sc.CLAMP):
        native = langevin(cuda_device, c["x"], c["grad"], None, clamp=clamp, seed=seed, offset=offset)
        assert same_bits(native, langevin(cuda_device, c["x"], c["grad"], eps, clamp=clamp))
        assert same_bits(native, sc.langevin_step(c["x"], c["grad"], eps, sc.ETA, sc.SQRT_ETA, sc.NOISE_COEF, clamp))
    native = langevin(cuda_device, c["x"], c["grad"], None, seed=seed, offset=offset)
    assert not same_bits(native, langevin(cuda_device, c["x"], c["grad"], None, seed=seed, offset=offset + 1))


@gpu
@pytest.mark.parametrize("n", [5, 1023, 1025, sc.BIG_GROUPS[1]])
def test_wide_and_plain_langevin_kernels_agree(cuda_device, n):
    """n is ragged (the plain kernel), n - n % 4 whole groups (the wide one): the same first n - n % 4 outputs."""
    c, n4 = sc.elem_case(n), n - n % 4
    for noise in (c["noise"], None):
        plain = langevin(cuda_device, c["x"], c["grad"], noise, seed=SEED, offset=9)
        wide = langevin(cuda_device, c["x"][:n4], c["grad"][:n4], None if noise is None else noise[:n4], seed=SEED, offset=9)
        assert plain.numel() == n and wide.numel() == n4 and same_bits(plain[:n4], wide)


@gpu
@pytest.mark.parametrize("n", [3, 5, 1024, 1025] + list(sc.BIG_GROUPS))
def test_langevin_out_may_alias_x(cuda_device, n):
    c = sc.elem_case(n)
    for noise, clamp in ((c["noise"], None), (None, sc.CLAMP)):
        apart = langevin(cuda_device, c["x"], c["grad"], noise, clamp=clamp, seed=SEED, offset=2)
        assert same_bits(langevin(cuda_device, c["x"], c["grad"], noise, clamp=clamp, seed=SEED, offset=2, alias=True), apart)


@gpu
@pytest.mark.parametrize("n", [3, 1024, 1025] + list(sc.BIG_GROUPS))
def test_langevin_step_dev_reads_seed_and_step_from_memory(cuda_device, n):
    c = sc.elem_case(n)
    seen = []
    for step in (11, (5 << 32) + 17):  # the second above 2^32: a counter cut to 32 bits would draw step 17
        dev_form = langevin(cuda_device, c["x"], c["grad"], None, state=(SEED, step))
        assert same_bits(dev_form, langevin(cuda_device, c["x"], c["grad"], None, seed=SEED, offset=step))
        seen.append(dev_form)
    assert not same_bits(seen[0], seen[1])
    assert not same_bits(seen[1], langevin(cuda_device, c["x"], c["grad"], None, seed=SEED, offset=17))
    clamped = langevin(cuda_device, c["x"], c["grad"], None, clamp=sc.CLAMP, state=(SEED, 11))
    assert same_bits(clamped, seen[0].clamp(*sc.CLAMP))


# ---------------------------------------------------------------------------------
# diffusion step
# ---------------------------------------------------------------------------------
def diffusion(dev, x, grad, noise, d, period, seed=0, offset=0, alias=False):
    n, c = x.numel(), Call(dev)
    if alias:
        xd = out = c.out(n, x)
    else:
        xd, out = c.inp(x), c.out(n)
    gd, nd, dd = c.inp(grad), c.inp(noise), c.inp(d)
    c.run("ebm_langevin_step_diffusion_f32", xd.data_ptr(), _lib.ptr(gd), out.data_ptr(), _lib.ptr(nd), dd.data_ptr(), period, n,
          sc.ETA, sc.SQRT_ETA, seed, offset)
    _written(out)
    return out.cpu()


@gpu
@pytest.mark.parametrize("dim", [1, 3, 5, 64])
def test_diffusion_step_is_the_restatement(cuda_device, dim):
    n = 7 * dim  # ragged for every dim but 64
    c, (seed, offset) = sc.elem_case(n), (SEED, 21)
    eps = field(cuda_device, n, _lib.NOISE_NORMAL, seed, offset).cpu()
    for period in sorted({1, dim, n}):
        d = sc.diffusion_field(period)
        for grad in (c["grad"], None):
            want = sc.diffusion_step(c["x"], grad, c["noise"], d, period, sc.ETA, sc.SQRT_ETA)
            assert same_bits(diffusion(cuda_device, c["x"], grad, c["noise"], d, period), want), (period, grad is None)
            assert same_bits(diffusion(cuda_device, c["x"], grad, c["noise"], d, period, alias=True), want), (period, "aliased")
        native = diffusion(cuda_device, c["x"], c["grad"], None, d, period, seed=seed, offset=offset)
        assert same_bits(native, sc.diffusion_step(c["x"], c["grad"], eps, d, period, sc.ETA, sc.SQRT_ETA)), (period, "native")
        assert same_bits(native, diffusion(cuda_device, c["x"], c["grad"], None, d, period, seed=seed, offset=offset, alias=True))
    # D = 0 switches the noise off: the drift alone
    zero = diffusion(cuda_device, c["x"], c["grad"], c["noise"], torch.zeros(1), 1)
    assert same_bits(zero, c["x"] - sc.s32(sc.ETA) * c["grad"] + 0.0 * c["noise"])


@gpu
@pytest.mark.parametrize("n,period", [(sc.BIG_GROUPS[1], 1), (sc.BIG_GROUPS[0], 245), (sc.BIG_GROUPS[1], sc.BIG_GROUPS[1])])
def test_diffusion_step_past_one_grid_pass(cuda_device, n, period):
    assert n % period == 0
    c, d = sc.elem_case(n), sc.diffusion_field(period)
    eps = field(cuda_device, n, _lib.NOISE_NORMAL, SEED, 4).cpu()
    assert same_bits(diffusion(cuda_device, c["x"], c["grad"], None, d, period, seed=SEED, offset=4),
                     sc.diffusion_step(c["x"], c["grad"], eps, d, period, sc.ETA, sc.SQRT_ETA))


# ---------------------------------------------------------------------------------
# leapfrog sub-steps
# ---------------------------------------------------------------------------------
def kick_drift(dev, x, p, force, eps, mass_kind=sc.MASS_NONE, mass_scalar=0.0, mass_diag=None, safe=False, alias=False):
    (n_chains, dim), c = x.shape, Call(dev)
    n = n_chains * dim
    if alias:
        xd = x_new = c.out(n, x)
        pd = p_half = c.out(n, p)
    else:
        xd, pd, x_new, p_half = c.inp(x), c.inp(p), c.out(n), c.out(n)
    fd = c.inp(force)
    md = c.inp(mass_diag) if mass_kind == sc.MASS_DIAG else None
    c.run("ebm_leapfrog_kick_drift_f32", xd.data_ptr(), pd.data_ptr(), fd.data_ptr(), x_new.data_ptr(), p_half.data_ptr(), n_chains, dim,
          eps, mass_kind, float(mass_scalar), _lib.ptr(md), int(safe))
    _written(x_new, p_half)
    return x_new.cpu().view(n_chains, dim), p_half.cpu().view(n_chains, dim)


def kick(dev, x_new, p_half, force, eps, safe=False, alias=False):
    n, c = x_new.numel(), Call(dev)
    xd = c.out(n, x_new)  # in/out: the scrub
    if alias:
        pd = p_new = c.out(n, p_half)
    else:
        pd, p_new = c.inp(p_half), c.out(n)
    fd = c.inp(force)
    c.run("ebm_leapfrog_kick_f32", xd.data_ptr(), pd.data_ptr(), fd.data_ptr(), p_new.data_ptr(), n, eps, int(safe))
    _written(p_new)
    return xd.cpu().view(x_new.shape), p_new.cpu().view(x_new.shape)


KICK_SHAPES = [(1, 1), (2, 1), (1, 3), (4, 1), (1, 5), (341, 3), (1024, 1), (205, 5), (103, 8)] + list(sc.BIG_KICK_DRIFT)


@gpu
@pytest.mark.parametrize("n_chains,dim", KICK_SHAPES)
def test_kick_drift_is_the_restatement(cuda_device, n_chains, dim):
    mass = sc.diag_mass(dim)
    for wild in (False, True):
        c = sc.kick_case(n_chains, dim, wild)
        for name, kind, scalar in sc.MASS_FORMS:
            for safe in (False, True):
                want = sc.kick_drift(c["x"], c["p"], c["force"], sc.EPS, kind, scalar, mass, safe)
                got = kick_drift(cuda_device, c["x"], c["p"], c["force"], sc.EPS, kind, scalar, mass, safe)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, safe, wild)
                if wild or n_chains * dim > 100000:  # (the aliased form once per mass form and safe flag is enough at the small sizes)
                    continue
                again = kick_drift(cuda_device, c["x"], c["p"], c["force"], sc.EPS, kind, scalar, mass, safe, alias=True)
                assert same_bits(again[0], want[0]) and same_bits(again[1], want[1]), (name, safe, "aliased")
    big = kick_drift(cuda_device, c["x"], c["p"], c["force"], sc.EPS, sc.MASS_DIAG, 0.0, mass, True, alias=True)
    assert same_bits(big[0], want[0]) and same_bits(big[1], want[1])


@gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_kick_is_the_restatement(cuda_device, n):
    for wild in (False, True):
        c = sc.kick_case(n, 1, wild)
        for safe in (False, True):
            want = sc.kick(c["x"], c["p"], c["force"], sc.EPS, safe)
            for alias in (False, True):
                got = kick(cuda_device, c["x"], c["p"], c["force"], sc.EPS, safe, alias)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (safe, wild, alias)
            if safe:  # what needs no scrub keeps its bits; NaN -> 0, +-inf -> +-FLT_MAX
                clean = torch.isfinite(c["x"])
                assert torch.equal(got[0][clean].view(torch.int32), c["x"][clean].view(torch.int32))
                assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
            else:
                assert torch.equal(torch.isnan(got[0]), torch.isnan(c["x"]))
    if n >= 5:
        fmax = torch.finfo(torch.float32).max
        assert sorted(got[0][~clean].flatten().tolist()) == [-fmax, 0.0, fmax]


@gpu
@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("name,kind,scalar", sc.MASS_FORMS)
def test_the_two_kernels_are_the_oracle_leapfrog(cuda_device, name, kind, scalar, safe):
    n, dim, dev = 37, 5, cuda_device
    g = torch.Generator().manual_seed(11)
    x, p = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    x[3, 1] = 300.0  # a force past the safe-mode clamp
    energy, mass = oracle.DoubleWell(2.0, 1.0), sc.diag_mass(dim)
    want_x, want_p = leapfrog(energy, x, p, 0.05, 1, sc.oracle_mass(kind, scalar, mass), safe=safe)
    got_x, got_p = sc.leapfrog_once(energy, x, p, 0.05, kind, scalar, mass, safe,
                                    kd=lambda *a: kick_drift(dev, *a), kk=lambda *a: kick(dev, *a))
    assert same_bits(got_x, want_x) and same_bits(got_p, want_p)


# ---------------------------------------------------------------------------------
# Metropolis accept
# ---------------------------------------------------------------------------------
COUNT0 = 1000  # what accept_count holds before the call: the entry adds to it


def accept(dev, x, x_prop, h0, h1, u, mask=True, count=True, seed=0, offset=0, state=None, delta=0):
    """-> (x, mask or None, count or None) on the CPU.  `state` = (seed, step): the _dev form at step + delta."""
    (n, dim), c = x.shape, Call(dev)
    xd = c.out(n * dim, x)
    pd, h0d, h1d, ud = c.inp(x_prop), c.inp(h0), c.inp(h1), c.inp(u)
    m = c.out(n, dtype=torch.uint8) if mask else None
    k = c.out(1, torch.tensor([COUNT0], dtype=torch.int32), dtype=torch.int32) if count else None
    if state is None:
        c.run("ebm_hmc_accept_f32", xd.data_ptr(), pd.data_ptr(), h0d.data_ptr(), h1d.data_ptr(), _lib.ptr(ud), _lib.ptr(m), _lib.ptr(k),
              n, dim, seed, offset)
    else:
        st = c.inp(rng_state(dev, *state))
        c.run("ebm_hmc_accept_dev_f32", xd.data_ptr(), pd.data_ptr(), h0d.data_ptr(), h1d.data_ptr(), _lib.ptr(m), _lib.ptr(k), n, dim,
              st.data_ptr(), delta)
    if mask:
        assert bool((m <= 1).all()), "a mask slot was not written"
    return xd.cpu().view(n, dim), None if m is None else m.cpu().bool(), None if k is None else int(k.item())


@gpu
@pytest.mark.parametrize("n,dim", sc.accept_shapes())
def test_accept_is_the_restatement(cuda_device, n, dim):
    c = sc.accept_case(n, dim)
    args = (c["x"], c["x_prop"], c["h0"], c["h1"], c["u"])
    x, mask, count = accept(cuda_device, *args)
    assert torch.equal(mask, c["acc"]), f"{int((mask != c['acc']).sum())} decisions differ"
    assert same_bits(x, c["x_out"])
    assert count == COUNT0 + int(c["acc"].sum()), "accept_count is added to"
    for pos, j in sc.edge_positions(n).items():
        assert bool(mask[pos]) == sc.EDGE_ROWS[j][3], (pos, sc.EDGE_ROWS[j])
    # rejected rows keep their bits (a NaN coordinate among them), accepted rows are the proposal's
    keep = ~c["acc"]
    assert torch.equal(x[keep].view(torch.int32), c["x"][keep].view(torch.int32))
    assert torch.equal(x[c["acc"]].view(torch.int32), c["x_prop"][c["acc"]].view(torch.int32))
    for with_mask, with_count in ((False, True), (True, False), (False, False)):
        x2, mask2, count2 = accept(cuda_device, *args, mask=with_mask, count=with_count)
        assert same_bits(x2, x)
        assert mask2 is None or torch.equal(mask2, mask)
        assert count2 is None or count2 == count


def _native_accept_inputs(dev, n, dim, seed, step):
    """Hamiltonians built from the kernel's own uniforms at (seed, step), so that no decision is close."""
    u = field(dev, n, _lib.NOISE_UNIFORM, seed, step).cpu()
    assert torch.equal(u, torch.from_numpy(oracle.uniform_field(seed, step, n)))
    h0, h1 = sc.hamiltonians_from_u(u)
    sc.apply_edges(h0, h1, u, fixed_u=True)
    acc, a64 = sc.accept_ref(h0, h1, u)
    assert bool((sc.accept_margin_ok(u, a64) | torch.isnan(a64)).all())
    g = torch.Generator().manual_seed(9500 + n + dim)
    x, x_prop = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    return x, x_prop, h0, h1, acc


@gpu
@pytest.mark.parametrize("n,dim", [(1, 3), (63, 1), (65, 8), (257, 3), (1000, 1030)] + list(sc.ACCEPT_BIG))
def test_accept_native_uniforms_are_the_field(cuda_device, n, dim):
    seed, step = SEED, (2 << 32) + 7
    x, x_prop, h0, h1, acc = _native_accept_inputs(cuda_device, n, dim, seed, step)
    got_x, mask, count = accept(cuda_device, x, x_prop, h0, h1, None, seed=seed, offset=step)
    assert torch.equal(mask, acc) and count == COUNT0 + int(acc.sum())
    assert same_bits(got_x, torch.where(acc.view(-1, 1), x_prop, x))
    if n >= 63:
        assert acc.any() and (~acc).any()
    # the _dev form: the stored step plus the launch's delta
    for stored, delta in ((step, 0), (step - 5, 5), ((2 << 32) - 1, 8)):
        dx, dmask, dcount = accept(cuda_device, x, x_prop, h0, h1, None, state=(seed, stored), delta=delta)
        assert torch.equal(dmask, mask) and dcount == count and same_bits(dx, got_x), (stored, delta)
    if n >= 63:  # another step decides otherwise
        assert not torch.equal(accept(cuda_device, x, x_prop, h0, h1, None, state=(seed, step), delta=1)[1], mask)


# ---------------------------------------------------------------------------------
# descent step and lookahead
# ---------------------------------------------------------------------------------
def descent(dev, x, grad, v, alias=False):
    n, c = x.numel(), Call(dev)
    if alias:
        xd = out = c.out(n, x)
    else:
        xd, out = c.inp(x), c.out(n)
    gd = c.inp(grad)
    vd = None if v is None else c.out(n, v)  # updated in place
    c.run("ebm_descent_step_f32", xd.data_ptr(), gd.data_ptr(), _lib.ptr(vd), out.data_ptr(), n, sc.DESCENT_ETA,
          sc.MOMENTUM if v is not None else 0.0)
    _written(out)
    return out.cpu(), None if vd is None else vd.cpu()


def lookahead(dev, x, v, alias=False):
    n, c = x.numel(), Call(dev)
    if alias:
        xd = out = c.out(n, x)
    else:
        xd, out = c.inp(x), c.out(n)
    vd = c.inp(v)
    c.run("ebm_lookahead_f32", xd.data_ptr(), vd.data_ptr(), out.data_ptr(), n, sc.MOMENTUM)
    _written(out)
    return out.cpu()


@gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_descent_step_and_lookahead_are_the_fma_restatement(cuda_device, n):
    c = sc.elem_case(n)
    for alias in (False, True):
        out, _ = descent(cuda_device, c["x"], c["grad"], None, alias)
        assert same_bits(out, sc.descent_step(c["x"], c["grad"], None, sc.DESCENT_ETA, 0.0)[0]), ("plain", alias)
        out, v = descent(cuda_device, c["x"], c["grad"], c["v"], alias)  # (Call.run checks that x kept its bits when it is apart)
        want = sc.descent_step(c["x"], c["grad"], c["v"], sc.DESCENT_ETA, sc.MOMENTUM)
        assert same_bits(out, want[0]) and same_bits(v, want[1]), ("momentum", alias)
        assert same_bits(lookahead(cuda_device, c["x"], c["v"], alias), sc.lookahead(c["x"], c["v"], sc.MOMENTUM)), ("lookahead", alias)
    assert not same_bits(v, c["v"])


# ---------------------------------------------------------------------------------
# noise fill
# ---------------------------------------------------------------------------------
KINDS = (_lib.NOISE_NORMAL, _lib.NOISE_UNIFORM, _lib.NOISE_RAW_U32)


def _bits(t):
    return t.view(torch.int32)


@gpu
@pytest.mark.parametrize("n", GROUP_SIZES)
def test_noise_fill_dev_is_noise_fill_at_the_stored_step_plus_delta(cuda_device, n):
    dev = cuda_device
    for kind in KINDS:
        for stored, delta in ((40, 2), ((1 << 32) - 1, 3)):
            want = field(dev, n, kind, SEED, stored + delta)
            c = Call(dev)
            out, st = c.out(n), c.inp(rng_state(dev, SEED, stored))
            c.run("ebm_noise_fill_dev_f32", out.data_ptr(), n, kind, st.data_ptr(), delta)
            assert torch.equal(_bits(out), _bits(want)), (kind, stored, delta)
        assert not torch.equal(_bits(want), _bits(field(dev, n, kind, SEED, stored)))
    # a shorter fill is the front of a longer one: the field does not depend on the launch
    if n > 4:
        assert torch.equal(_bits(field(dev, n - 3, _lib.NOISE_NORMAL, SEED, 6)), _bits(field(dev, n, _lib.NOISE_NORMAL, SEED, 6)[:n - 3]))


@gpu
@pytest.mark.parametrize("n", sc.BIG_GROUPS)
def test_noise_fill_past_one_grid_pass_is_the_oracle_field(cuda_device, n):
    seed, step = SEED, (7 << 32) + 11
    n_groups = (n + 3) // 4
    groups = np.unique(np.concatenate([np.arange(0, n_groups, 997), np.arange(sc.GRID_LANES - 2, n_groups)])).astype(np.uint64)
    assert (groups >= sc.GRID_LANES).sum() >= 257
    o = oracle.philox4x32_10(groups & np.uint64(0xFFFFFFFF), groups >> np.uint64(32), np.full(len(groups), step & 0xFFFFFFFF),
                             np.full(len(groups), step >> 32), seed & 0xFFFFFFFF, seed >> 32)
    elems = (groups.astype(np.int64)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    want = np.stack(o, axis=1).reshape(-1)[elems < n]
    elems = torch.from_numpy(elems[elems < n])
    raw = field(cuda_device, n, _lib.NOISE_RAW_U32, seed, step).cpu().view(torch.int32)[elems].numpy().view(np.uint32)
    assert np.array_equal(raw, want)
    uni = field(cuda_device, n, _lib.NOISE_UNIFORM, seed, step).cpu()[elems].numpy()
    assert np.array_equal(uni, ((want >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)).astype(np.float32))
    # the normals of the same counters: hardware log / sqrt / sin / cos, the bar of test_rng.py (not a state comparison)
    tail = 4 * (sc.GRID_LANES - 2)
    nor = field(cuda_device, n, _lib.NOISE_NORMAL, seed, step).cpu()[tail:].numpy()
    ref = oracle.normal_field(seed, step, n)[tail:]
    assert nor.shape == ref.shape and bool((np.abs(nor - ref) <= 5e-6 + 2e-5 * np.abs(ref)).all())


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
@gpu
def test_empty_and_negative_sizes_launch_nothing(cuda_device):
    dev = cuda_device
    bufs = [torch.full((256,), FILL, device=dev) for _ in range(6)]
    a, b, c, d, e, f = (t.data_ptr() for t in bufs)
    st = rng_state(dev, SEED, 3)
    keep = st.clone()
    s = _lib.stream_handle(dev)

    def calls(n):
        return [
            ("ebm_langevin_step_f32", (a, b, c, d, n, 0.1, 0.3, 1.0, 0, 0.0, 0.0, 1, 2, s)),
            ("ebm_langevin_step_dev_f32", (a, b, c, n, 0.1, 0.3, 1.0, 0, 0.0, 0.0, st.data_ptr(), s)),
            ("ebm_langevin_step_diffusion_f32", (a, b, c, d, e, 1, n, 0.1, 0.3, 1, 2, s)),
            ("ebm_leapfrog_kick_drift_f32", (a, b, c, d, e, n, 4, 0.1, 0, 0.0, None, 0, s)),
            ("ebm_leapfrog_kick_f32", (a, b, c, d, n, 0.1, 1, s)),
            ("ebm_hmc_accept_f32", (a, b, c, d, e, f, None, n, 4, 1, 2, s)),
            ("ebm_hmc_accept_dev_f32", (a, b, c, d, f, None, n, 4, st.data_ptr(), 1, s)),
            ("ebm_descent_step_f32", (a, b, c, d, n, 0.1, 0.9, s)),
            ("ebm_lookahead_f32", (a, b, c, n, 0.9, s)),
            ("ebm_noise_fill_f32", (a, n, 0, 1, 2, s)),
            ("ebm_noise_fill_dev_f32", (a, n, 0, st.data_ptr(), 1, s)),
        ]

    for name, args in calls(0):
        _lib.call(name, *args)  # an empty call is no error
    for name, args in calls(-1):
        with pytest.raises(ValueError, match=name):
            _lib.call(name, *args)
    # the diffusion entry's own refusals, the accept entries' row width, the fill's kind
    for name, args in [
        ("ebm_langevin_step_diffusion_f32", (a, b, c, d, e, 3, 64, 0.1, 0.3, 1, 2, s)),      # 3 does not divide 64
        ("ebm_langevin_step_diffusion_f32", (a, b, c, d, e, 0, 64, 0.1, 0.3, 1, 2, s)),
        ("ebm_langevin_step_diffusion_f32", (a, b, c, d, None, 1, 64, 0.1, 0.3, 1, 2, s)),   # no diffusion tensor
        ("ebm_hmc_accept_f32", (a, b, c, d, e, f, None, 16, 0, 1, 2, s)),
        ("ebm_hmc_accept_dev_f32", (a, b, c, d, f, None, 16, 0, st.data_ptr(), 1, s)),
        ("ebm_hmc_accept_dev_f32", (a, b, c, d, f, None, 16, 4, None, 1, s)),
        ("ebm_leapfrog_kick_drift_f32", (a, b, c, d, e, 16, 4, 0.1, 2, 0.0, None, 0, s)),      # diagonal mass without its tensor
        ("ebm_langevin_step_f32", (a + 4, b, c, d, 64, 0.1, 0.3, 1.0, 0, 0.0, 0.0, 1, 2, s)),  # a misaligned pointer
        ("ebm_noise_fill_f32", (a, 64, 3, 1, 2, s)),
        ("ebm_noise_fill_dev_f32", (a, 64, 0, None, 1, s)),
    ]:
        with pytest.raises(ValueError, match=name):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    for t in bufs:
        assert bool((t == FILL).all())
    assert torch.equal(st, keep)
