"""GPU: more rays than one pass of the query kernels' grid.  query_kernel and
path_kernel launch min(waves, CUs * 64) one-wave workgroups and stride over the
batch, so the loop's second trip -- its counters, the re-read of the last ray
by the lanes past the end, the level-major records k * n + i with a large n --
needs more than 64 * 64 * CUs rays.  The rays are simple.txt's 4,133-ray batch
repeated; 4,133 is no multiple of 64, so every repetition lands on other lanes,
and the answers are the batch's answers repeated."""
import functools

import numpy as np
import pytest

import path_ref
import query_cases as qc
import ray_ref
from conftest import scene_path
from test_gpu_paths import check_records
from test_gpu_rays import _bits

pytestmark = pytest.mark.gpu

N_BASE = 4133
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def _base():
    """simple.txt, its 4,133 rays and their answers: (scene, arrays, o, d, a RayBatch, the depth-2 levels)."""
    import rt_hip

    sc = rt_hip.Scene.load(scene_path("simple"))
    sa = path_ref.SceneArrays(sc)
    assert (sc.num_spheres, sc.num_lights) == (5, 2)
    o, d = ray_ref.gen_rays(1, N_BASE, sa.centers, sa.radii, tuple(sc.camera().position))
    levels = path_ref.trace_paths(o, d, 2, sa)
    b = qc.RayBatch(sc, o, d, levels[0]["t"], levels[0]["sphere"], 101)
    assert 0.25 <= b.hit_share <= 0.85 and 0 < b.occ.sum() < (b.sphere >= 0).sum()
    assert levels[1]["traced"].any() and (levels[1]["sphere"] >= 0).any()
    return sc, sa, o, d, b, levels


def _count():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 64 * cus + 64 + 37
    assert n > 64 * 64 * cus  # a second trip of the grid-stride loop, with a full wave and a ragged one in it
    return n


def test_trace_rays_second_trip(gpu_renderer):
    import rt_hip

    sc, sa, o, d, b, _ = _base()
    n = _count()
    gpu_renderer.upload(sc)
    ro, rd, rtmax = np.resize(o, (n, 3)), np.resize(d, (n, 3)), np.resize(b.tmax, n)
    want_t, want_s, want_occ = np.resize(b.t, n), np.resize(b.sphere, n), np.resize(b.occ, n)
    slow = int(np.resize(qc.slow_rays(sc, o, d), n).sum())
    t, s, occ, st = gpu_renderer.trace_rays(ro, rd, rtmax, rt_hip.RT_QUERY_CLOSEST)
    assert np.array_equal(s, want_s) and np.array_equal(_bits(t), _bits(want_t)) and np.array_equal(occ, want_occ)
    assert (st.rays, st.hits, st.rays_unaccelerated) == (n, int((want_s >= 0).sum()), slow)
    t2, s2, occ2, st2 = gpu_renderer.trace_rays(ro, rd, rtmax, rt_hip.RT_QUERY_OCCLUDED)
    assert np.array_equal(occ2, want_occ) and (s2 == -1).all() and np.array_equal(_bits(t2), _bits(np.full(n, 1e20)))
    assert (st2.rays, st2.hits, st2.rays_unaccelerated) == (n, int(want_occ.sum()), slow)


def test_trace_paths_second_trip(gpu_renderer):
    import rt_hip
    import torch

    sc, sa, o, d, _, base_levels = _base()
    n, depth = _count(), 2
    gpu_renderer.upload(sc)
    levels = [{k: np.resize(v, (n,) + v.shape[1:]) for k, v in lv.items() if k in ("traced", "reflects", "sphere",
                                                                                   "t", "shadowed")}
              for lv in base_levels]
    host = np.zeros((n, 8))
    host[:, 0:3], host[:, 3:6] = np.resize(o, (n, 3)), np.resize(d, (n, 3))
    rays = torch.from_numpy(host).to("cuda:0")
    vbytes, guard = depth * n * 32, 4096
    vbuf = torch.full((vbytes + guard,), FILL, dtype=torch.uint8, device="cuda:0")
    gpu_renderer.trace_paths_device(rays.data_ptr(), n, depth, vbuf.data_ptr(), 0)
    st = gpu_renderer.path_stats()
    vh = vbuf.cpu().numpy()
    verts = vh[:vbytes].view(rt_hip.VERTEX_DTYPE).reshape(depth, n)
    check_records(levels, verts, None)  # every vertex of both levels
    assert (vh[vbytes:] == FILL).all()  # the guard after the buffer is untouched
    segments = int(sum(int(lv["traced"].sum()) for lv in levels))
    hits = int(sum(int((lv["traced"] & (lv["sphere"] >= 0)).sum()) for lv in levels))
    assert (st.rays, st.segments, st.hits, st.shadow_rays) == (n, segments, hits, hits * sc.num_lights)
