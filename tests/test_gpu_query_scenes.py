"""GPU: ray and path queries on generated scenes (tests/query_cases.py: a fixed
list of fuzz_gen scenes with 1 to 1,500 spheres, margin geometry, scenes moved
up to 1e6 from the origin, negative radii, mirror clouds, 0 to 6 lights; and
one of tiny spheres in a large box) against ray_ref / path_ref, which
test_query_cases_host.py pins to the oracle on these same scenes.  The query
kernels run the render's sweeps and walks with a configuration of their own
(margins sized for the query region, no behind grid, the non-kFast closest-hit
body); these scenes are where a bound, a margin or a walk of that
configuration would drop or add a sphere.

Per scene four batches: 1,061 ray_ref.gen_rays rays; the scene's own camera
rays at 33x17 (the margin generator's tangent and surface cameras); 101 rays
of which every other starts far outside the query region (lanes of the
every-sphere sweep beside lanes of the culled one, and hit points whose
rounding error carries the deeper levels out of the region); and 229 rays
aimed at sphere limbs, within 1e-12 .. 1e-4 of the tangent, half of them from
the region's shell outside the scene's bounds, where the margins sized for
the region are needed.  tmax takes the classes of query_cases.gen_tmax_edges:
the limits at which the occlusion test changes its method.  Every comparison
covers all rays and records, as bit patterns."""
import pytest

import query_cases as qc
from test_gpu_paths import check_records, check_stats
from test_gpu_rays import KNOB_SETS, check_parity

pytestmark = pytest.mark.gpu

IDS = [qc.scene_id(c) for c in qc.SCENES]


def check_rays(r, case, kind):
    """Both modes of rt_trace_rays on one batch of the uploaded scene."""
    b = qc.batch(*case, kind)
    n = len(b.o)
    st, st2 = check_parity(r, b, n)
    assert st.rays_unaccelerated == int(qc.slow_rays(b.scene, b.o, b.d).sum())
    return st


def check_paths(r, case, kind):
    """rt_trace_paths at depth 4 on one batch of the uploaded scene, with and without surfaces."""
    sa = qc.scene(*case)[1]
    o, d = qc.rays(*case, kind)
    levels = qc.paths(*case, kind)
    unaccel = qc.paths_unaccelerated(*case, kind)
    verts, surf, st = r.trace_paths(o, d, qc.DEPTH, surfaces=True)
    check_records(levels, verts, surf)
    check_stats(st, levels, sa, unaccel)
    verts2, none, st2 = r.trace_paths(o, d, qc.DEPTH)
    assert none is None and verts2.tobytes() == verts.tobytes()
    check_stats(st2, levels, sa, unaccel)
    assert (st2.tests_exact, st2.tests_cull) == (st.tests_exact, st.tests_cull)
    return st


def check_scene(r, case):
    sc, sa = qc.scene(*case)
    r.upload(sc)
    large = case in qc.LARGE
    for kind in qc.KINDS:
        st = check_rays(r, case, kind)
        pst = check_paths(r, case, kind)
        if large and kind != "far":
            # the walks ran: far fewer exact tests than a sweep over every sphere would make
            m = sc.num_spheres
            queries = pst.segments + pst.shadow_rays
            print(f"{qc.scene_id(case)} {kind}: tests_exact / (rays * spheres) = {st.tests_exact / (st.rays * m):.4f}"
                  f" (rays), {pst.tests_exact / (queries * m):.4f} (paths)")
            assert st.rays_unaccelerated == 0 and pst.unaccelerated == 0
            assert st.tests_exact < st.rays * m // 4
            assert pst.tests_exact < queries * m // 4


# ---- 1. every scene of the list, the product build -----------------------------------------
@pytest.mark.parametrize("case", qc.SCENES, ids=IDS)
def test_generated_scene(gpu_renderer, case):
    check_scene(gpu_renderer, case)


# ---- 2. the bounds-checked build and the other BVH layouts, on a subset -----------------------
def test_checked_build():
    import rt_hip

    r = rt_hip.Renderer(0, variant="check")
    try:
        for case in qc.SUBSET:
            check_scene(r, case)
        r.stats()  # raises on RT_ERR_CHECK
    finally:
        r.close()


@pytest.fixture(params=list(KNOB_SETS))
def layout_renderer(request, monkeypatch):
    import rt_hip

    for k, v in KNOB_SETS[request.param].items():
        monkeypatch.setenv(k, v)
    r = rt_hip.Renderer(0, variant="tuning")  # reads the knobs at rt_create
    yield r
    r.close()


def test_layouts(layout_renderer):
    for case in qc.SUBSET:
        sc, _ = qc.scene(*case)
        layout_renderer.upload(sc)
        for kind in qc.KINDS:
            check_rays(layout_renderer, case, kind)
            check_paths(layout_renderer, case, kind)


# ---- 3. tmax at the occlusion test's thresholds, 4,133 rays ------------------------------------
@pytest.mark.parametrize("which", ["complex", ("margin", 7)], ids=["complex", "margin7"])
def test_tmax_edges(gpu_renderer, which):
    b = qc.edge_batch(which)
    gpu_renderer.upload(b.scene)
    check_parity(gpu_renderer, b, qc.N_EDGE)  # RT_QUERY_CLOSEST and RT_QUERY_OCCLUDED
