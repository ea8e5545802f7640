"""The predicated exact ray-sphere tests of the list loops against the chain
form, on the CPU (tests/native/exact_forms_check.cpp).

rt_device.h's exact_num / shadow_exact / closest_test decide a candidate with
lane predicates and wave-uniform branches (any_lane: the device's ballot, on
the host the lane's own value); the per-lane arithmetic is intersect_num's.
On num_check.cpp's generators at 1,000,000 accepted iterations -- 8 M shadow
pairs and 16 M closest pairs, plus a generator for the band class and the
lanes that are not `fast` -- the shadow decision equals the chain's and the
reference's, and the closest update leaves the same (bt, bi, bn) as the chain
after every candidate.  The class counts are asserted so that no class passes
by being absent."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predicated_forms_equal_the_chain(tmp_path):
    exe = tmp_path / "exact_forms_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I",
                    os.path.join(REPO, "cs420-ray-tracer_amd", "csrc"), "-I", os.path.join(REPO, "include"), "-o",
                    str(exe), os.path.join(REPO, "tests", "native", "exact_forms_check.cpp")], check=True)
    out = subprocess.run([str(exe), "1000000"], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    sh, cl = out.stdout.strip().splitlines()[-2:]
    w = sh.split()
    assert w[0] == "shadow", sh
    s = {w[k]: int(w[k + 1]) for k in range(2, len(w), 2)}
    assert int(w[1]) >= 8000000 and s["diff"] == 0 and s["wrong"] == 0, sh
    assert s["tangent"] >= 100000 and s["early"] >= 500000 and s["band"] >= 5000 and s["tiny"] >= 20, sh
    assert s["sqfree"] >= s["early"] and s["notfast"] >= 100000, sh
    c = cl.split()
    assert c[0] == "closest", cl
    q = {c[k]: int(c[k + 1]) for k in range(2, len(c), 2)}
    assert int(c[1]) >= 16000000 and q["diff"] == 0, cl
    assert q["hits"] >= 5000000 and q["cold"] >= 20 and q["notfast"] >= 100000, cl
