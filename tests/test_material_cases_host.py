"""CPU-only: the out-of-range material cases of tests/material_cases.py, before the GPU sees them.

* The conditions the GPU tests rely on hold on the oracle's fp64 framebuffer for every (case, form, size,
  depth) they render: no NaN, no channel at or below INT_MIN / 255.99 (where int() is undefined in the
  reference), +inf only in the `has_inf` cases and there at least once, a negative-channel count above 0
  in every `expects_negative` case and 0 in every other.
* The oracle equals the REFERENCE on them.  Each was rendered by oracle/_ref/ref_render (the reference's own
  trace_ray and write_ppm); write_ppm prints `r = int(...)` as a double, so a channel quantised below 0
  appears as a negative token such as -12.  tests/golden/material_cases.json records the SHA-256 of the
  scene text, the SHA-256 of the reference's P3 with every negative token replaced by 0, and the number of
  negative tokens; the oracle's P3 must hash to the one and its `negative` count equal the other.  Where the
  reference build is present the bytes are compared directly as well.
* rt_scene_parse reads every number of the texts (-0, 1e-300, -1e-300, 1e300, 1e9, 65535.5 among them) to
  the bits the oracle's parser reads.
* ray_hybrid's CPU tile worker (csrc/rt_cpu.cpp) renders the dense cases as the oracle does: byte-equal for
  the `exact` cases, within 1 per channel for the others (its pow is the host's, as the oracle's is, so no
  difference is expected there either).

  python tests/test_material_cases_host.py     # re-record the hashes (needs oracle/_ref/ref_render)
"""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import material_cases as mc
from test_hybrid import checker  # noqa: F401  (the fixture that builds tests/native/cpu_tiles_check.cpp)
from test_oracle_vs_reference import p3

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "oracle", "_ref", "ref_render")
RECORD = os.path.join(REPO, "tests", "golden", "material_cases.json")
INT_MIN = -2147483647.0


def key(case, form, W, H, D):
    return "%s/%s/%dx%d/d%d" % (case, form, W, H, D)


def case_forms():
    """(case, form) pairs with their (W, H, depth) lists, in material_cases.used()'s order."""
    out = {}
    for case, form, W, H, D in mc.used():
        out.setdefault((case, form), []).append((W, H, D))
    return out


CASE_FORMS = case_forms()
IDS = ["%s-%s" % cf for cf in CASE_FORMS]


def check_conditions(case, fb, negative, where, expects_negative=None):
    if expects_negative is None:
        expects_negative = mc.expects_negative(case)
    assert not np.isnan(fb).any(), where
    with np.errstate(invalid="ignore"):
        assert not (255.99 * np.minimum(1.0, fb) <= INT_MIN).any(), where
    assert not np.isneginf(fb).any(), where
    ninf = int(np.isposinf(fb).sum())
    if mc.has_inf(case):
        assert ninf > 0, where
    else:
        assert ninf == 0, where
    if expects_negative:
        assert negative > 0, where
    else:
        assert negative == 0, where


@pytest.mark.parametrize("case,form", list(CASE_FORMS), ids=IDS)
def test_conditions_hold_on_the_oracle(case, form):
    for W, H, D in CASE_FORMS[(case, form)]:
        rgb, counts, fb = mc.oracle(case, form, W, H, D)
        where = key(case, form, W, H, D)
        check_conditions(case, fb, counts["negative"], where)
        # the count is the framebuffer's: channels whose int(255.99 * min(1, c)) is below 0
        q = np.trunc(255.99 * np.minimum(1.0, fb))
        assert counts["negative"] == int((q < 0).sum()), where
        assert (np.frombuffer(rgb, np.uint8).reshape(H, W, 3)[q < 0] == 0).all(), where


@pytest.mark.parametrize("case", mc.AA_CASES)
def test_conditions_hold_on_the_antialias_oracle(case):
    for W, H, D in mc.AA_SHAPES:
        _, counts, fb = mc.oracle_aa(case, W, H, D)
        neg = mc.expects_negative(case) and (case, (W, H, D)) not in mc.AA_NO_NEGATIVE
        check_conditions(case, fb, counts["negative"], key(case, "aa", W, H, D), expects_negative=neg)


def test_classification():
    exact = {c for c in mc.ALL_CASES if mc.is_exact(c)}
    assert exact == {"refl_above_one", "refl_negative", "colour_negative", "colour_large", "light_negative",
                     "light_large", "ambient_negative", "refl_zeros"} | set(mc.F64_EXPECTS_NEGATIVE)
    assert len(mc.NAMES) == 12 and set(mc.EXPECTS_NEGATIVE) <= set(mc.NAMES)
    assert mc.text("refl_above_one", "sparse").count("sphere") == 40
    assert "sphere 0 -1001" not in mc.text("refl_above_one", "sparse")
    assert mc.text("refl_above_one", "dense").count("sphere") == 5


# ---- the oracle against the reference ------------------------------------------------------
def zero_negative_tokens(data: bytes):
    """(the P3 with every negative pixel token replaced by 0, the number replaced).  The three header
    lines hold no negative number."""
    lines = data.split(b"\n")
    n = 0
    for i in range(3, len(lines)):
        toks = lines[i].split()
        for k, t in enumerate(toks):
            if t.startswith(b"-"):
                toks[k] = b"0"
                n += 1
        lines[i] = b" ".join(toks)
    return b"\n".join(lines), n


def reference_p3(tmp, text, W, H, D) -> bytes:
    path, out = os.path.join(tmp, "scene.txt"), os.path.join(tmp, "out.ppm")
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([REF, path, str(W), str(H), str(D), "--out", out], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out, "rb") as f:
        return f.read()


@pytest.mark.parametrize("case,form", list(CASE_FORMS), ids=IDS)
def test_oracle_equals_reference(case, form, tmp_path):
    with open(RECORD) as f:
        record = json.load(f)
    live = os.access(REF, os.X_OK)
    text = mc.text(case, form)
    for W, H, D in CASE_FORMS[(case, form)]:
        where = key(case, form, W, H, D)
        want = record[where]
        rgb, counts, _ = mc.oracle(case, form, W, H, D)
        assert hashlib.sha256(text.encode()).hexdigest() == want["sha256_scene"], "generator changed: " + where
        assert hashlib.sha256(p3(rgb, W, H)).hexdigest() == want["sha256_p3"], where
        assert counts["negative"] == want["negative_tokens"], where
        if live:
            ref, n = zero_negative_tokens(reference_p3(str(tmp_path), text, W, H, D))
            assert p3(rgb, W, H) == ref, where
            assert counts["negative"] == n, where


def test_record_holds_nothing_else():
    with open(RECORD) as f:
        record = json.load(f)
    assert set(record) == {key(*u) for u in mc.used()}


# ---- parser parity -----------------------------------------------------------------------
def bits(*values):
    return [struct.pack("<d", v) for v in values]


@pytest.mark.parametrize("case,form", list(CASE_FORMS), ids=IDS)
def test_parser_reads_the_oracles_bits(case, form):
    import orc
    import rt_hip

    text = mc.text(case, form)
    sc = rt_hip.Scene.parse(text)
    keep = orc.OracleScene(text=text)  # owns the arrays `o` points into
    o = keep.s
    assert (sc.num_spheres, sc.num_lights, sc.raw.has_camera) == (o.num_spheres, o.num_lights, o.has_camera)
    v3 = lambda v: (v.x, v.y, v.z)  # noqa: E731
    for i in range(sc.num_spheres):
        a, b = sc.sphere(i), o.spheres[i]
        got = bits(*a["center"], a["radius"], *a["color"], a["reflectivity"], a["shininess"])
        want = bits(*v3(b.center), b.radius, *v3(b.color), b.reflectivity, b.shininess)
        assert got == want, (i, a)
    for i in range(sc.num_lights):
        a, b = sc.light(i), o.lights[i]
        assert bits(*a["position"], *a["color"], a["intensity"]) == bits(*v3(b.position), *v3(b.color),
                                                                         b.intensity), (i, a)
    raw = sc.raw
    assert bits(*raw.ambient, *raw.cam_position, *raw.cam_look_at, raw.cam_fov) == bits(
        *v3(o.ambient), *v3(o.cam_position), *v3(o.cam_look_at), o.cam_fov)


def test_parser_texts_hold_the_edge_tokens():
    """The numbers whose reading is least certain are in the texts, and read to the expected bits."""
    import rt_hip

    shin = lambda case: [rt_hip.Scene.parse(mc.text(case)).sphere(i)["shininess"] for i in (1, 2, 3)]  # noqa: E731
    refl = lambda case: [rt_hip.Scene.parse(mc.text(case)).sphere(i)["reflectivity"] for i in (1, 2, 3)]  # noqa: E731
    assert bits(*shin("shin_zero_tiny")) == bits(0.0, 1e-300, -0.0)
    assert bits(*shin("shin_huge")) == bits(65537.0, 1e9, 1e300)
    assert bits(*shin("shin_frac_edges")) == bits(1023.5, 0.999999999, 65535.5)
    assert bits(*refl("refl_negative")) == bits(-0.5, -2.0, -1e-300)
    assert bits(*refl("refl_zeros")) == bits(-0.0, 0.0, 1e-300)


# ---- ray_hybrid's CPU tile worker ---------------------------------------------------------------
@pytest.mark.parametrize("case", mc.NAMES)
def test_cpu_tile_worker_equals_oracle(checker, tmp_path, case):  # noqa: F811
    W, H, D = 64, 48, 4
    path = tmp_path / "scene.txt"
    path.write_text(mc.text(case, "dense"))
    out = tmp_path / "rgb.bin"
    # cpu_tiles_check SCENE W H DEPTH TILE OUT_RGB OUT_COSTS
    subprocess.run([checker, str(path), str(W), str(H), str(D), "16", str(out), str(tmp_path / "costs.txt")],
                   check=True, timeout=600)
    got = out.read_bytes()
    want, _, _ = mc.oracle(case, "dense", W, H, D)
    d = np.abs(np.frombuffer(got, np.uint8).astype(np.int16) - np.frombuffer(want, np.uint8).astype(np.int16))
    print("%s: %d of %d channels differ" % (case, int((d > 0).sum()), d.size))
    if mc.is_exact(case):
        assert got == want, int((d > 0).sum())
    else:
        assert len(got) == len(want) and int(d.max()) <= 1, int((d > 1).sum())


if __name__ == "__main__":
    import tempfile

    for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "cs420-ray-tracer_amd")):
        sys.path.insert(0, p)
    record = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, form, W, H, D in mc.used():
            text = mc.text(case, form)
            data, n = zero_negative_tokens(reference_p3(tmp, text, W, H, D))
            record[key(case, form, W, H, D)] = {"sha256_scene": hashlib.sha256(text.encode()).hexdigest(),
                                                "sha256_p3": hashlib.sha256(data).hexdigest(),
                                                "negative_tokens": n}
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
