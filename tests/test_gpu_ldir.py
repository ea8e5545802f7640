"""GPU: the light direction's shared-reciprocal quotients (rt_device.h
div3_shared, formed by every lane of shade_hit's light loop with no guard
around it) against three IEEE divisions, bit for bit, wherever div3_ok holds --
the guard the loop carries in its wave-uniform predicate (light_common).
tests/native/ldir_check.hip, compiled here with the product's floating-point
flags: div_check.hip's four operand kinds, 2^20 triples each, two seeds."""
import os
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

N = 1 << 20


@pytest.fixture(scope="module")
def ldir_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ldir") / "ldir_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(REPO, "include"), "-o", str(exe),
                    os.path.join(REPO, "tests", "native", "ldir_check.hip")], check=True)
    return str(exe)


@pytest.mark.parametrize("seed", [3, 20261020])
def test_div3_shared_bit_identical_under_div3_ok(seed, ldir_check):
    out = subprocess.run([ldir_check, str(seed), str(N)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("kind")]
    assert len(rows) == 4, out.stdout
    tested = [int(r[3]) for r in rows]
    ok = [int(r[5]) for r in rows]
    bad = [int(r[7]) for r in rows]
    assert tested == [N] * 4
    # the same bits wherever the guard holds
    assert bad == [0] * 4, out.stdout
    # the renderer-shaped operands (a scene vector, a near-unit vector, over their own lengths) all pass the guard
    assert ok[0] == N and ok[1] == N
    # the whole double range and the edge values meet the guard's boundary from both sides
    assert 0 < ok[2] < N and 0 < ok[3] < N
