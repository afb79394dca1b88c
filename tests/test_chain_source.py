"""ebm_langevin_chain_from_f32 without a GPU: the entry's argument checks (they come before any launch), and the call
pattern of LangevinDynamics on the fused route, recorded through a stand-in for the library handle -- the real
``_lib.call`` runs, so the booking of the out-of-place entry under ``ebm_langevin_chain_f32`` is what is checked."""

import ctypes

import pytest
import torch

from helpers import fused_cpu  # noqa: F401  (the fixture)
from torchebm_amd import _lib

EINVAL = -1
X = 0x10000  # never dereferenced: every call below returns before a launch


def _from(x_src, x, n=8, dim=4, k=3, flags=0):
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    desc.s[0], desc.s[1] = 2.0, 1.0
    rc = _lib.lib().ebm_langevin_chain_from_f32(ctypes.byref(desc), x_src, x, n, dim, k, 0.01, 0.1, 1.0, None, flags, 0.0, 0.0, 1,
                                                None, None, None, 0, 0, None)
    return rc, _lib.lib().ebm_last_error_string().decode()


def test_the_entry_is_exported_at_the_same_abi_version():
    assert "ebm_langevin_chain_from_f32" in _lib.EXPORTS and _lib.ABI_VERSION == 9
    assert _lib.BOOKED_AS["ebm_langevin_chain_from_f32"] == "ebm_langevin_chain_f32"


@pytest.mark.parametrize("delta", [16, 8 * 4 * 4 - 16, -16, -(8 * 4 * 4 - 16)])  # the state is 128 bytes
def test_partial_overlap_is_refused(delta):
    rc, msg = _from(X + delta, X)
    assert rc == EINVAL and "overlaps" in msg, (rc, msg)
    rc, msg = _from(X + delta, X, k=0)  # also where no step would run
    assert rc == EINVAL and "overlaps" in msg, (rc, msg)


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_misaligned_source_is_refused(offset):
    rc, msg = _from(X + 4096 + offset, X)
    assert rc == EINVAL and "16-byte aligned" in msg, (rc, msg)


def test_the_same_pointer_and_null_are_accepted():
    """x_src == x and x_src == NULL are the in-place call.  With no step or no chain there is nothing to launch, so the
    call returns 0 from behind the argument checks (the launches themselves: tests/test_chain_source_gpu.py)."""
    for src in (X, None):
        assert _from(src, X, k=0)[0] == 0
        assert _from(src, X, n=0)[0] == 0


def test_the_other_checks_are_those_of_the_in_place_entry():
    rc, msg = _from(X + 4096, None)
    assert rc == EINVAL and "state pointer is NULL" in msg
    rc, msg = _from(X + 4096, X, flags=4)
    assert rc == EINVAL and "unknown bits" in msg
    rc, msg = _from(X + 4096, X + 4)
    assert rc == EINVAL and "16-byte aligned" in msg


# ---------------------------------------------------------------------------------------------------------------
# the sampler's call pattern
# ---------------------------------------------------------------------------------------------------------------
def _chain_calls(rec):
    return [(name, args) for name, args in rec.calls if name.startswith("ebm_langevin")]


def test_plain_sample_is_one_out_of_place_launch(fused_cpu):
    make, rec, clones = fused_cpu
    x = torch.randn(16, 4)
    out = make().sample(x=x, n_steps=3)
    calls = _chain_calls(rec)
    assert [name for name, _ in calls] == ["ebm_langevin_chain_from_f32"]
    args = calls[0][1]
    assert args[1] == x.data_ptr() and args[2] == out.data_ptr() and out.data_ptr() != x.data_ptr()
    assert args[3:6] == (16, 4, 3) and args[-3:-1] == (7, 11)
    assert x.data_ptr() not in clones
    assert _lib.call_counts["ebm_langevin_chain_f32"] == 1 and "ebm_langevin_chain_from_f32" not in _lib.call_counts


def test_timing_events_are_booked_under_the_in_place_name(fused_cpu, monkeypatch):
    make, rec, _ = fused_cpu

    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setitem(_lib.timed_events, "ebm_langevin_chain_f32", [])
    make().sample(x=torch.randn(16, 4), n_steps=3)
    assert len(_lib.timed_events["ebm_langevin_chain_f32"]) == 1


def test_donated_input_is_the_in_place_entry(fused_cpu):
    make, rec, clones = fused_cpu
    s = make()
    s.donate_input = True
    x = torch.randn(16, 4)
    out = s.sample(x=x, n_steps=3)
    calls = _chain_calls(rec)
    assert [name for name, _ in calls] == ["ebm_langevin_chain_f32"]
    assert calls[0][1][1] == x.data_ptr() and out.data_ptr() == x.data_ptr() and not clones


def test_a_call_without_a_launch_keeps_the_copy(fused_cpu):
    make, rec, clones = fused_cpu
    x = torch.randn(16, 4)
    out = make().sample(x=x, n_steps=0)
    assert not _chain_calls(rec) and torch.equal(out, x) and out.data_ptr() != x.data_ptr()
    empty = torch.empty(0, 4)
    assert make().sample(x=empty, n_steps=3).shape == (0, 4) and not _chain_calls(rec)


def test_an_input_that_is_converted_has_no_source(fused_cpu):
    """a state that dense_f32 had to copy (here: not contiguous) is already the sampler's own: in place, as before"""
    make, rec, _ = fused_cpu
    x = torch.randn(4, 16).t()
    make().sample(x=x, n_steps=3)
    assert [name for name, _ in _chain_calls(rec)] == ["ebm_langevin_chain_f32"]


def test_heun_keeps_its_copy(fused_cpu):
    make, rec, clones = fused_cpu
    x = torch.randn(16, 4)
    out = make(integrator="heun").sample(x=x, n_steps=3)
    calls = _chain_calls(rec)
    assert [name for name, _ in calls] == ["ebm_langevin_heun_chain_f32"]
    assert calls[0][1][1] == out.data_ptr() != x.data_ptr() and x.data_ptr() in clones


def test_only_the_first_launch_of_a_cut_call_reads_the_source(fused_cpu, monkeypatch):
    make, rec, _ = fused_cpu
    monkeypatch.setattr(_lib, "diag_layout", lambda *a, **kw: (1, 4, 1024))  # (n_blocks, slots, block_elems)
    s = make()
    s.DIAG_RECORD_BYTES = 2 * 4 * (2 * 4 + 8)  # the records of two kept steps
    x = torch.randn(16, 4)
    out, _ = s.sample(x=x, n_steps=5, return_diagnostics=True)
    calls = _chain_calls(rec)
    assert [name for name, _ in calls] == ["ebm_langevin_chain_from_f32", "ebm_langevin_chain_f32", "ebm_langevin_chain_f32"]
    assert calls[0][1][1] == x.data_ptr() and calls[0][1][2] == out.data_ptr()
    assert all(args[1] == out.data_ptr() for _, args in calls[1:])
    assert [args[4] for _, args in calls[1:]] == [2, 1] and calls[0][1][5] == 2  # steps per launch: 2, 2, 1

    rec.calls.clear()
    monkeypatch.setattr(_lib, "diag_layout", lambda *a, **kw: None)  # no in-kernel records: one launch per kept step
    out, _ = make().sample(x=x, n_steps=5, thin=2, return_diagnostics=True)
    calls = _chain_calls(rec)
    assert [name for name, _ in calls] == ["ebm_langevin_chain_from_f32", "ebm_langevin_chain_f32", "ebm_langevin_chain_f32"]
    assert calls[0][1][1] == x.data_ptr() and all(args[1] == out.data_ptr() for _, args in calls[1:])
