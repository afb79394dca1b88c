"""The route map (tests/chain_cases.py ROUTES) against what it claims to cover, on the CPU: every chain launcher chain_launch.h
declares and every chain kernel the built library holds has a pinned case, and every pinned family sits on one side of a
predicate edge whose other side is pinned too.  A launcher or kernel instantiation added later without a case breaks this."""

import os
import re
import subprocess

import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "torchebm_amd", "csrc", "chain_launch.h")


def declared_launchers():
    text = open(HEADER).read()
    return set(re.findall(r"^int\s+(launch_\w+)\s*\(", text, flags=re.M))


def library_kernel_families():
    """family_of of every kernel in libebm_hip.so: the host-side handles of the __global__ functions (one data symbol per
    instantiation, named as the kernel is)."""
    from torchebm_amd import _lib

    out = subprocess.run(["nm", "-C", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    fams = set()
    for line in out.splitlines():
        parts = line.split(" ", 2)
        if len(parts) < 3 or parts[1] not in "dDVvWu":
            continue
        name = parts[2]
        head = name.replace("(anonymous namespace)::", "").split("(")[0]
        if "(" not in name or "ebm::" not in head or "stub" in head or "_kernel" not in head.split("<")[0]:
            continue
        fams.add(cc.family_of(name))
    return fams


def pinned_families():
    out = set()
    for c in cc.ROUTES:
        out |= set(c.family.split()) | set(c.family_noise.split())
    return out


def test_every_chain_launcher_has_a_pinned_route_case():
    declared = declared_launchers()
    assert len(declared) >= 25, declared
    pinned = {c.launcher for c in cc.ROUTES}
    missing = declared - pinned - set(cc.ROUTE_EXEMPT)
    assert not missing, f"chain launchers without a case in tests/chain_cases.py ROUTES: {sorted(missing)}"
    assert not (pinned | set(cc.ROUTE_EXEMPT)) - declared, "ROUTES names a launcher chain_launch.h does not declare"


def test_every_chain_kernel_in_the_library_has_a_pinned_route_case():
    fams = library_kernel_families()
    assert len(fams) >= 60, sorted(fams)
    missing = fams - pinned_families() - set(cc.KERNELS_OFF_ROUTE)
    assert not missing, f"kernel families of libebm_hip.so without a case in tests/chain_cases.py ROUTES: {sorted(missing)}"
    stale = (pinned_families() | set(cc.KERNELS_OFF_ROUTE)) - fams
    assert not stale, f"families named in tests/chain_cases.py that the library does not hold: {sorted(stale)}"


def test_route_cases_are_distinct_and_complete():
    ids = [c.id for c in cc.ROUTES]
    assert len(ids) == len(set(ids))
    for c in cc.ROUTES:
        assert c.launcher and c.family, c.id
        assert c.sampler in ("langevin", "heun", "hmc") and c.energy in ("gauss", "gmm", "ring"), c.id
        assert (c.K > 0) == (c.energy != "gauss"), c.id


def test_every_pinned_family_sits_on_a_predicate_edge():
    by_id = {c.id: c for c in cc.ROUTES}
    on_edge = set()
    for a, b in cc.EDGES:
        assert a in by_id and b in by_id, (a, b)
        ca, cb = by_id[a], by_id[b]
        assert (ca.launcher, ca.family) != (cb.launcher, cb.family), (a, b)
        for c in (ca, cb):
            on_edge |= set(c.family.split())
    # (a case's noise-field family comes with its plain one)
    missing = {f for c in cc.ROUTES for f in c.family.split()} - on_edge
    assert not missing, f"pinned families with no case at a predicate edge: {sorted(missing)}"


def test_every_records_family_is_pinned_by_a_records_case():
    """the kernels that write diagnostics records themselves -- a *_diag_kernel, a DIAG=true instantiation of the matrix-core
    HMC template, a <true, ...> instantiation of the streamed-Ps Langevin kernels -- each have a records=True case, which
    is what tests/test_records_fp64_gpu.py reads the records of"""
    def emits(f):
        return f.endswith("_diag_kernel") or "DIAG=true" in f or re.match(r"gauss_(res|big)_langevin_kernel<(true,|\d+,true,)", f)

    fams = {f for f in library_kernel_families() if emits(f) and f not in cc.KERNELS_OFF_ROUTE}
    assert len(fams) >= 10, sorted(fams)
    with_records = {f for c in cc.ROUTES if c.records for f in (c.family + " " + c.family_noise).split()}
    assert not fams - with_records, f"records-emitting families without a records=True case: {sorted(fams - with_records)}"
