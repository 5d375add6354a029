"""The HOST side of libwtk_hip.so under AddressSanitizer + UndefinedBehaviorSanitizer, in the build container (no GPU).

tests/hostsan/build.py compiles every translation unit with `hipcc --cuda-host-only -fsanitize=address,undefined` (no device code; kernels become launch
stubs) and links it against tests/hostsan/hip_stub.cpp — a no-op launch layer that models device memory, streams, events and stream capture, and checks
every launch's argument struct against the live allocations — and tests/hostsan/driver.cpp, which drives the C ABI over the GPU suite's shape matrix
(scales n / s / m, 32 x 32 ... 640 x 640 here, 1280 x 1280 and B = 256 in `full` mode; every dtype, both plans, every entry point, handles created and
destroyed out of phase, two host threads).  What it pins: planning, weight packing, launcher geometry, allocation sizes against kernel extents, and the
stream / event lifetime protocol of csrc/wtk_plan.hip / wtk_run.hip (the call of yolo_controller.py:64-90, 96-98 that must never die).
Launches are eager: the library captures nothing, so the stub's capture model is exercised by the selftest (a caller may still capture its own stream)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsan"))
import build as hostsan  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(hostsan.HIPCC), reason="hipcc not installed")


def _ok(r):
    tail = "\n".join(r.stdout.splitlines()[-60:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stdout and "runtime error:" not in r.stdout and "VIOLATION" not in r.stdout, tail


def test_launch_layer_flags_deliberate_violations():
    """The checker checks: eleven protocol / memory violations committed on purpose through the stub's HIP API, and a window launch whose symbol
    names another instantiation than its arguments ask for, are all reported."""
    r = hostsan.run("selftest")
    assert r.returncode == 0 and "12 of 12 deliberate violations flagged" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("env", list(hostsan.ENVS.values()), ids=list(hostsan.ENVS))  # default, suite-env, ungrouped: see tests/hostsan/build.py
def test_host_side_is_clean_over_the_shape_matrix(env):
    r = hostsan.run("quick", env)
    _ok(r)
    assert "violations 0; driver failures 0" in r.stdout, r.stdout[-3000:]


def _trace_matches(matrix):
    envs, fixture, _ = hostsan.TRACES[matrix]
    with open(fixture) as f:
        want = json.load(f)
    assert sorted(want) == sorted(envs)
    bad = []
    for name, env in envs.items():
        got = hostsan.trace(env, matrix)
        names = sorted(set(got["kernels"]) | set(want[name]["kernels"]))
        diff = {k: (want[name]["kernels"].get(k, 0), got["kernels"].get(k, 0)) for k in names if want[name]["kernels"].get(k, 0) != got["kernels"].get(k, 0)}
        print(f"{name}: {got['launches']} launches (recorded {want[name]['launches']}), sha256 {got['sha256']}")
        for k, (w, g) in diff.items():
            print(f"  {k}: recorded {w}, now {g}")
        if got["sha256"] != want[name]["sha256"] or diff:
            bad.append(name)
    assert not bad, f"launch trace differs from {os.path.relpath(fixture, hostsan.ROOT)} in {bad} (per-kernel count differences are printed above)"


def test_launch_trace_matches_the_recorded_one():
    """Planning and launching are pinned launch by launch: in every environment of the quick matrix the stub's ordered launch lines (kernel instantiation,
    grid, block, dynamic LDS, stream ordinal, hash of the argument struct with device pointers as (allocation, offset); the two-thread section left out)
    hash to the sha256 recorded in tests/golden/launch_trace.json, which was recorded on the commit BEFORE wtk_run.hip was split into resolve / issue steps.
    A change that leaves behaviour alone reproduces it.  A pull request that changes planning on purpose re-records it on its own tree with
    `python tests/hostsan/build.py trace --record` and says so."""
    _trace_matches("quick")


def test_failed_creates_leave_nothing_behind():
    """Mode `failures`: three handles (fp16 128 x 128, latency f16x3 384 x 384 with scratch and tickets, f16x3 640 x 640 B = 64 with the sparse region), each created
    once per allocation it makes with that allocation failing: the call returns non-zero, leaves *out null and an error text, and the device bytes and events
    that are live afterwards are those from before; then the create succeeds again.  The same for the fp16 range guards of pack_stem and pack_conv."""
    r = hostsan.run("failures", timeout=1500)
    _ok(r)
    assert "[hostsan] creation failures" in r.stdout and "violations 0; driver failures 0" in r.stdout, r.stdout[-3000:]


def test_host_side_is_clean_over_the_full_matrix():
    """`full` mode: 120 handles up to 1280 x 1280 and B = 256 (large device regions are address-space reservations: nothing is touched), ~50 s."""
    r = hostsan.run("full", {"WTK_SK_AUTOTUNE": "0"}, timeout=1500)
    _ok(r)
    assert "violations 0; driver failures 0" in r.stdout, r.stdout[-3000:]


def test_full_matrix_launch_trace_matches_the_recorded_one():
    """The same pin over the `full` matrix (tests/golden/launch_trace_full.json, recorded on the commit BEFORE wtk_yolo_create_planned was split into passes): the
    handles above 16 frames, which the quick matrix never creates — the sparse region and the list grids, ws64, the persistent window form, the 1280 geometry; and in a second environment the two-slab window kernels.
    Re-recorded with `python tests/hostsan/build.py trace full --record`."""
    _trace_matches("full")
