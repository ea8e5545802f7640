"""CPU-only: the oracle (oracle/liborc.so, the C restatement the GPU parity
tests check against) pinned to the REFERENCE itself on random scenes, not
only on the committed fixtures.  Each scene of tests/fuzz_gen.py's general,
near-light and EPSILON-margin generators (the ones the GPU fuzz uses) was
rendered by oracle/_ref/ref_render -- the reference's own trace_ray /
load_scene / Camera / write_ppm (src/main.cpp:16-91, scene.h, sphere.h,
scene_loader.h) compiled from the reference sources by oracle/Makefile,
unmodified -- and the SHA-256 of its P3 bytes is recorded in
tests/golden/oracle_vs_reference.json; the oracle's P3 bytes of the same
scene must hash to it.  Where the reference build is present the scene is also
rendered by it again and the bytes compared directly.  The GPU fuzz then
compares the device against the oracle on the same generators, so the chain
device == oracle == reference holds on random inputs.

  python tests/test_oracle_vs_reference.py     # re-record the hashes (needs oracle/_ref/ref_render)
"""
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(REPO, "oracle", "_ref", "ref_render")
RECORD = os.path.join(REPO, "tests", "golden", "oracle_vs_reference.json")


def p3(rgb: bytes, w: int, h: int) -> bytes:
    out = [b"P3\n%d %d\n255\n" % (w, h)]
    for i in range(0, len(rgb), 3):
        out.append(b"%d %d %d\n" % (rgb[i], rgb[i + 1], rgb[i + 2]))
    return b"".join(out)


# (generator, seed, scenes)
CASES = [("scene", 501, 120), ("near", 502, 80), ("margin", 503, 160)]


def scenes(case):
    """The case's (k, scene text, W, H, D) sequence."""
    import fuzz_gen

    gen, seed, count = case
    rng = random.Random(seed)
    for k in range(count):
        text = fuzz_gen.margin_scene(rng) if gen == "margin" else fuzz_gen.scene(rng, near=(gen == "near"))
        W, H = rng.choice(fuzz_gen.ODD_SIZES if gen == "margin" else fuzz_gen.SIZES)
        W, H = min(W, 64), min(H, 48)  # the reference's serial brute force: keep each render well under a second
        D = rng.choice([1, 2, 4, 8])
        yield k, text, W, H, D


def reference_p3(tmp, k, text, W, H, D) -> bytes:
    path = os.path.join(tmp, "s%d.txt" % k)
    with open(path, "w") as f:
        f.write(text)
    out = os.path.join(tmp, "s%d.ppm" % k)
    r = subprocess.run([REF, path, str(W), str(H), str(D), "--out", out], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out, "rb") as f:
        return f.read()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_equals_reference_on_random_scenes(case, tmp_path):
    import orc

    gen, seed, count = case
    with open(RECORD) as f:
        want = json.load(f)[gen]
    assert want["seed"] == seed and len(want["sha256_p3"]) == count
    live = os.access(REF, os.X_OK)
    done = 0
    for k, text, W, H, D in scenes(case):
        got, _, _ = orc.OracleScene(text=text).render(W, H, D, threads=4)
        where = "%s seed %d scene %d (%dx%d d%d)\n%s" % (gen, seed, k, W, H, D, text)
        assert hashlib.sha256(text.encode()).hexdigest() == want["sha256_scene"][k], "generator changed: " + where
        assert hashlib.sha256(p3(got, W, H)).hexdigest() == want["sha256_p3"][k], where
        if live:
            assert p3(got, W, H) == reference_p3(str(tmp_path), k, text, W, H, D), where
        done += 1
    assert done == count


if __name__ == "__main__":
    import tempfile

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    record = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            rows = [(hashlib.sha256(text.encode()).hexdigest(),
                     hashlib.sha256(reference_p3(tmp, k, text, W, H, D)).hexdigest())
                    for k, text, W, H, D in scenes(case)]
            record[case[0]] = {"seed": case[1], "source": "oracle/_ref/ref_render (the reference's trace_ray)",
                               "sha256_scene": [a for a, _ in rows], "sha256_p3": [b for _, b in rows]}
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
