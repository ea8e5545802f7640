"""GPU: the lights-over-lanes pass of path_kernel (rt_paths.h).  A wave with
nh <= 32 hit lanes and nl >= 2 lights asks its shadow queries in passes of
lpp = min(64 / nh, nl) lights: lane j asks light l0 + j % cnt for the
(j / cnt)-th hit lane, and each hit lane collects its bits from the ballot.
One wave of 64 rays from the origin, h of them hitting the reflective sphere
at lanes scattered over the wave, in a scene of nl lights (tests/query_cases.py
lattice_*), over a lattice of (nl, h): one and several passes, a short last
pass (h = 5, nl = 13: 12 and 1), nh * cnt = 63 (h = 3, nl = 64: 21, 21, 21,
1), all 64 lanes helping (h = 32, nl = 64), and the one-light loop from h = 33
on.  Level 1 repeats it with the reflections.  test_query_cases_host.py
asserts on the references that the hit lanes are the chosen ones and that the
shadow masks are mixed; every record is compared with path_ref as bits."""
import pytest

import path_ref
import query_cases as qc
from test_gpu_paths import check_records, check_stats

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h", qc.LATTICE_H)
@pytest.mark.parametrize("nl", qc.LATTICE_NL)
def test_lattice(gpu_renderer, nl, h):
    sc, sa, o, d, lanes, levels = qc.lattice_ref(nl, h)
    gpu_renderer.upload(sc)
    verts, surf, st = gpu_renderer.trace_paths(o, d, 2, surfaces=True)
    check_records(levels, verts, surf)
    rlo, rhi = qc.query_region(sc)
    check_stats(st, levels, sa, unaccel=path_ref.unaccelerated(levels, o, sa, rlo, rhi))
    assert st.shadow_rays == nl * st.hits and st.hits >= h
