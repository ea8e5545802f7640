"""CPU-only: the generated cases of the query tests (tests/query_cases.py).
On every scene of its list the numpy checkers equal the oracle -- path_ref's
shading of the scene's own camera rays is the oracle's image and ray counts,
ray_ref.intersect is orc_intersect -- so the GPU tests compare with references
that are pinned on exactly the scenes where they are used.  Then the
conditions under which those GPU tests mean something, asserted on the
references alone: what the scene list contains, that its batches are not
degenerate, that the limb rays straddle their tangents, that the
lights-over-lanes lattice has mixed shadow masks, and that the edge classes of
tmax all occur with both outcomes."""
import numpy as np
import pytest

import orc
import path_ref
import query_cases as qc
import ray_ref

IDS = [qc.scene_id(c) for c in qc.SCENES]


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---- the checkers against the oracle, on the list's scenes ---------------------------------
@pytest.mark.parametrize("case", qc.SCENES, ids=IDS)
def test_checker_reproduces_oracle(case, tmp_path):
    sc, sa = qc.scene(*case)
    path = tmp_path / "scene.txt"
    path.write_text(qc.scene_text(*case))
    want_rgb, want_counts, _ = orc.OracleScene(str(path)).render(qc.W, qc.H, qc.DEPTH, threads=4)
    levels = qc.paths(*case, "cam")
    n, segments, hits, shadow = path_ref.counts(levels, sa)
    assert n == qc.W * qc.H
    assert {"primary": n, "reflect": segments - n, "shadow": shadow} == {k: want_counts[k] for k in
                                                                          ("primary", "reflect", "shadow")}
    assert path_ref.quantize(path_ref.shade(levels, sa)).tobytes() == want_rgb


@pytest.mark.parametrize("case", qc.SCENES, ids=IDS)
def test_ray_ref_equals_oracle_intersect(case):
    """The first 150 rays of the scene's batch, each against the sphere the scan chose (where one exists)
    and two random others: the hit flag and the bits of t."""
    sc, sa = qc.scene(*case)
    n = 150
    o, d = (a[:n] for a in qc.rays(*case, "gen"))
    dn = ray_ref.normalize(d)  # the oracle takes the Ray's stored (normalised) direction
    b = qc.batch(*case, "gen")
    pick = np.random.default_rng(2).integers(0, sc.num_spheres, (n, 3))
    pick[:, 0] = np.where(b.sphere[:n] >= 0, b.sphere[:n], pick[:, 0])
    hits = 0
    for i in range(n):
        hit, t = ray_ref.intersect(o[i], dn[i], sa.centers[pick[i]], sa.radii[pick[i]])
        for k, s in enumerate(pick[i]):
            want_hit, want_t = orc.intersect(tuple(sa.centers[s]), float(sa.radii[s]), tuple(o[i]), tuple(dn[i]))
            assert bool(hit[0, k]) == want_hit, (i, s)
            if want_hit:
                assert _bits(t[0, k]) == _bits(want_t), (i, s, t[0, k], want_t)
                hits += 1
        if b.sphere[i] >= 0:
            assert hit[0, 0] and _bits(t[0, 0]) == _bits(b.t[i])
    assert 0 < hits < 3 * n  # both outcomes sampled


# ---- what the list contains ----------------------------------------------------------------
def test_scene_list_contents():
    assert 16 <= len(qc.SCENES) == len(set(qc.SCENES)) <= 24
    assert {g for g, _ in qc.SCENES} == set(qc.GENERATORS)
    counts, lights, moved, negative, clouds = [], [], 0, 0, 0
    for case in qc.SCENES:
        sc, sa = qc.scene(*case)
        assert sc.num_lights <= path_ref.MAX_LIGHTS
        counts.append(sc.num_spheres)
        lights.append(sc.num_lights)
        moved += bool(np.abs(sa.centers).min(axis=0).max() >= 1e5)  # every sphere at least 1e5 from the origin
        negative += bool((sa.radii < 0).any())
        clouds += bool(sc.num_spheres >= 30 and (sa.refl >= 0.7).mean() >= 0.9)
    for lo, hi in ((1, 1), (2, 2), (25, 50), (190, 215), (700, 700), (1100, 1115), (1500, 1500)):
        assert any(lo <= c <= hi for c in counts), (lo, hi, counts)
    assert min(lights) == 0 and max(lights) == 6
    assert moved >= 1 and negative >= 1 and clouds >= 2
    # the other builds' subset: one scene on either side of kBvhAlwaysAbove = 1024
    below, above = (qc.scene(*c)[0].num_spheres for c in qc.SUBSET)
    assert below < 1024 < above
    assert all(c in qc.SCENES for c in qc.SUBSET + qc.LARGE)
    assert sorted(qc.LARGE) == sorted(c for c in qc.SCENES if qc.scene(*c)[0].num_spheres >= 1100)


def test_batches_are_not_degenerate():
    mid = level3 = mixed = slow_deep = 0
    for case in qc.SCENES:
        sc, sa = qc.scene(*case)
        levels = qc.paths(*case, "gen")
        share = float((levels[0]["sphere"] >= 0).mean())
        mid += 0.05 <= share <= 0.95
        level3 += bool(levels[3]["traced"].any())
        full = np.uint64((1 << sc.num_lights) - 1)
        for lv in levels:
            m = lv["shadowed"][lv["sphere"] >= 0]
            if ((m != 0) & (m != full)).any():
                mixed += 1
                break
        # the far batch: rays of both sweeps at level 0, and deeper levels that leave the query region
        o, d = qc.rays(*case, "far")
        slow0 = qc.slow_rays(sc, o, d)
        assert slow0[1::2].all() and not slow0[0::2].any(), case
        slow_deep += qc.paths_unaccelerated(*case, "far", first_level=1)
        assert len(qc.rays(*case, "gen")[0]) == qc.N_GEN and len(qc.rays(*case, "cam")[0]) == qc.W * qc.H
    assert 2 * mid >= len(qc.SCENES), mid
    assert level3 >= 6 and mixed >= 4, (level3, mixed)
    assert slow_deep >= 1


def test_limb_rays_straddle_the_tangent():
    """Aimed 1e-4 inside the limb the ray hits its sphere, 1e-4 outside it misses (the discriminant's
    rounding error, relative to r^2, is about (D / r)^2 2^-52, and D / r stays below 2e5 here); nearer the
    tangent rounding decides.  Every origin lies in the query region, half of them outside the scene's bounds."""
    inside, outside, decided = [0, 0], [0, 0], 0  # [as aimed, of]
    for case in qc.SCENES:
        sc, sa = qc.scene(*case)
        o, d, s, e = qc.limb_rays(*case)
        assert len(o) == qc.N_LIMB and not qc.slow_rays(sc, o, d).any()
        lo, hi, _ = qc.bounds(sc)
        out = ~((o >= lo) & (o <= hi)).all(axis=1)
        assert out[0::2].all() and not out[1::2].any()
        dn = ray_ref.normalize(d)
        hit = np.array([ray_ref.intersect(o[i], dn[i], sa.centers[s[i]], sa.radii[s[i]])[0][0, 0]
                        for i in range(len(o))])
        far_enough = np.sqrt(((sa.centers[s] - o) ** 2).sum(axis=1)) > 1.01 * np.abs(sa.radii[s])
        within, beyond = far_enough & (e <= -1e-4), far_enough & (e >= 1e-4)
        inside = [inside[0] + int(hit[within].sum()), inside[1] + int(within.sum())]
        outside = [outside[0] + int((~hit)[beyond].sum()), outside[1] + int(beyond.sum())]
        near = far_enough & (np.abs(e) <= 1e-10)
        decided += int(hit[near].any() and not hit[near].all())
    n = len(qc.SCENES) * qc.N_LIMB
    assert inside[1] >= n // 16 and outside[1] >= n // 16  # one of the eleven classes each, origins outside the sphere
    assert inside[0] >= 0.99 * inside[1] and outside[0] >= 0.99 * outside[1], (inside, outside)
    assert decided >= len(qc.SCENES) // 2, decided


# ---- the lights-over-lanes lattice ---------------------------------------------------------
@pytest.mark.parametrize("nl", qc.LATTICE_NL)
def test_lattice_conditions(nl):
    mixed = np.zeros(nl, bool)
    first = last = False
    for h in qc.LATTICE_H:
        sc, sa, o, d, lanes, levels = qc.lattice_ref(nl, h)
        assert sc.num_lights == nl and len(lanes) == h and len(o) == 64
        # the hit lanes are exactly the chosen ones, scattered over the wave, and all hit the mirror
        assert np.array_equal(np.flatnonzero(levels[0]["sphere"] >= 0), lanes)
        assert (levels[0]["sphere"][lanes] == 0).all() and levels[1]["traced"][lanes].all()
        if 2 <= h <= 32:
            assert not np.array_equal(lanes, np.arange(h))
        masks = levels[0]["shadowed"][lanes]
        if h >= 2 and nl >= 7:
            assert len(set(masks.tolist())) >= 2, (nl, h)
        for lv in levels:
            m = lv["shadowed"][lv["sphere"] >= 0]
            if m.size:
                bits = ((m[:, None] >> np.arange(nl, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
                mixed |= bits.any(axis=0) & (~bits).any(axis=0)
                first, last = first or bool(bits[:, 0].any()), last or bool(bits[:, nl - 1].any())
    assert 3 * int(mixed.sum()) >= nl, int(mixed.sum())
    assert first and last


def test_lattice_pass_shapes():
    """The (hits, lights) pairs reach what they are for: passes of lpp = min(64 / hits, lights) lights."""
    def passes(h, nl):
        lpp = min(64 // h, nl)
        return [min(lpp, nl - l0) for l0 in range(0, nl, lpp)] if nl >= 2 and lpp >= 2 else None

    assert passes(5, 13) == [12, 1] and passes(3, 64) == [21, 21, 21, 1] and 3 * 21 == 63
    assert passes(32, 64) == [2] * 32 and passes(1, 64) == [64] and passes(2, 32) == [32]
    assert passes(33, 64) is None and passes(64, 2) is None  # the one-light loop
    assert {3, 5, 32, 33, 64} <= set(qc.LATTICE_H) and {13, 64} <= set(qc.LATTICE_NL)


# ---- tmax at the occlusion test's thresholds -----------------------------------------------
def test_tmax_edge_values():
    names = qc.TMAX_EDGE_CLASSES
    assert names[:len(ray_ref.TMAX_CLASSES)] == ray_ref.TMAX_CLASSES and len(set(names)) == len(names) == 32
    t = np.linspace(1.0, 2.0, 64, endpoint=False)  # one binade: an ulp is 2^-52
    tmax, cls = qc.gen_tmax_edges(3, t)
    assert sorted(set(cls.tolist())) == list(range(len(names)))
    at = lambda name: cls == names.index(name)  # noqa: E731
    ulp = 2.0 ** -52
    assert np.array_equal(tmax[at("t+4ulp")], t[at("t+4ulp")] + 4 * ulp)
    assert np.array_equal(tmax[at("t-2ulp")], t[at("t-2ulp")] - 2 * ulp)
    assert (tmax[at("t(1+2^-48)")] > t[at("t(1+2^-48)")]).all() and (tmax[at("t(1-2^-52)")] < t[at("t(1-2^-52)")]).all()
    assert (tmax[at("below1e20")] < 1e20).all() and (tmax[at("dblmax")] == np.finfo(np.float64).max).all()
    assert (tmax[at("2^-901")] == 2.0 ** -901).all() and (tmax[at("denorm_min")] == 5e-324).all()
    # the first seven classes are gen_tmax's own
    old, _ = ray_ref.gen_tmax(3, t)
    assert np.isnan(old).sum() > 0 and np.isnan(tmax[at("nan")]).all() and (tmax[at("minus")] == -1.0).all()


@pytest.mark.parametrize("which", ["complex", ("margin", 7)], ids=["complex", "margin7"])
def test_tmax_edge_batches(which):
    b = qc.edge_batch(which)
    names = qc.TMAX_EDGE_CLASSES
    assert len(b.o) == qc.N_EDGE and 0.25 <= b.hit_share <= 0.85, b.hit_share
    if which != "complex":
        assert b.scene.num_spheres > 1024
    assert sorted(set(b.cls.tolist())) == list(range(len(names)))  # every class occurs
    front = (b.sphere >= 0) & (b.t > 0)
    for k in qc.REL_EXPONENTS:
        up, down = (front & (b.cls == names.index("t(1%s2^-%d)" % (s, k))) for s in "+-")
        assert up.sum() >= 8 and down.sum() >= 8, k
        assert (b.occ[up] == 1).all() and (b.occ[down] == 0).all(), k
    for k in qc.ULP_STEPS:
        up, down = (front & (b.cls == names.index("t%s%dulp" % (s, k))) for s in "+-")
        assert up.any() and down.any() and (b.occ[up] == 1).all() and (b.occ[down] == 0).all(), k
    big = front & np.isin(b.cls, [names.index(c) for c in ("1e20", "below1e20", "1e21", "dblmax")])
    tiny = front & np.isin(b.cls, [names.index(c) for c in ("2^-900", "2^-901", "denorm_min")])
    assert big.any() and (b.occ[big] == 1).all() and tiny.any() and (b.occ[tiny] == 0).all()
