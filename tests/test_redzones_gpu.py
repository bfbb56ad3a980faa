"""Red zones around every tensor handed to a kernel: the parity tests that the suite already has, run again family by family
(tests/redzone_cases.py) in a child process (tests/redzone_worker.py) whose torch allocator is bsmi_debug_torch_malloc / _free
(csrc/dev_guard.hip): every tensor at its exact size -- no rounding to 512 bytes, no neighbour packed against it -- between two 4 MiB
zones of 0xFF, checked when it is released and after every family; the engines' own workspaces lie between the same zones
(BSMI_GUARD_MB, csrc/dev_guard.h).

What this proves: a WRITE outside a torch tensor or a guarded workspace (up to 4 MiB away) is counted and fails the family, with the
size of the tensor and the offsets on stderr.  A READ outside one returns 0xFF bytes (a NaN, the id 2^64 - 1, 255), and the parity
assertion of the test that ran the kernel fails if that value reaches a result.  A stray read whose value is then discarded stays
invisible.  And every device entry point of libbsmi.so was called at least once this way, or is listed with a reason."""
import json
import os
import subprocess
import sys

import pytest

import redzone_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def guard_run(tmp_path_factory):
    """the worker over every family, once for the whole module: (completed process, {family: report})"""
    report = os.path.join(str(tmp_path_factory.mktemp("redzones")), "report.json")
    env = dict(os.environ, BSMI_GUARD_MB="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "redzone_worker.py"), "all", report], env=env,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    return r, (json.load(open(report)) if os.path.exists(report) else {})


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_family_between_red_zones(guard_run, family):
    """the worker stops at the first family that fails or has a damaged zone: that one shows the log, the ones behind it did not run"""
    r, reports = guard_run
    assert "self-test ok" in r.stdout and "read control ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    assert family in reports or r.returncode != 0
    if family not in reports:
        ran = [f for f in RC.FAMILIES if f in reports]
        first = list(RC.FAMILIES)[len(ran)]
        assert family != first, r.stdout[-3000:] + r.stderr[-4000:]
        pytest.fail(f"not run: the worker stopped at family {first}")
    assert f"{family}: " in r.stdout


def test_the_guard_run_ended_with_every_zone_intact(guard_run):
    r, reports = guard_run
    assert r.returncode == 0 and "guards intact" in r.stdout.splitlines()[-1:] and set(reports) == set(RC.FAMILIES), \
        r.stdout[-3000:] + r.stderr[-4000:]


def test_every_device_entry_point_was_between_red_zones(guard_run):
    from bootstrapper_amd import _lib
    r, reports = guard_run
    assert set(reports) == set(RC.FAMILIES), "the guard run did not finish: " + r.stdout[-1000:] + r.stderr[-2000:]
    called = set().union(*(set(rep["called"]) for rep in reports.values()))
    missing = sorted(set(_lib.SYMBOLS) - called - set(RC.EXCLUDED))
    assert not missing, f"called by no family of tests/redzone_cases.py and not in its EXCLUDED: {missing}"
