"""GPU: the status the ray, path and radiance query entry points return when more
than one thing is wrong with a call -- which check comes first -- and what a
rejected or a foreign launch leaves of the families' own state (include/rt_hip.h:
rt_trace_rays, rt_trace_paths, rt_trace_radiance, rt_trace_radiance_resolve).

One context for the whole file.  The tests before `test_upload_*` run on it
before any scene is uploaded (file order); the others upload their scene
themselves.  65 rays throughout: two waves, the second with one lane.  The calls
go through the library handle where Renderer's wrappers would reject the
arguments first."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_paths import CAM, FILL, TRACED, TWO, _fan, _light_lines

pytestmark = pytest.mark.gpu

OK, INVALID, NO_SCENE, DEPTH = 0, 1, 5, 7  # RT_OK, RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE, RT_ERR_DEPTH
N = 65
D = 3
MAX_DEPTH, MAX_SAMPLES = 64, 64  # RT_MAX_DEPTH, RT_MAX_SAMPLES
F64 = 2  # RT_FB_F64X3
LIT = TWO + "light 3 4 0 1 1 1 1\n" + CAM
FAMILIES = ("rays", "paths", "radiance", "resolve")
DEEP = ("paths", "radiance", "resolve")  # the families that take a depth


class Ctx:
    """The context, its device buffers, and every entry point behind one signature."""

    def __init__(self):
        import rt_hip
        import torch

        self.rt = rt_hip
        self.r = rt_hip.Renderer(0)
        self.L, self.h = self.r._L, self.r.handle
        self.uploaded = False
        o, d = _fan()
        self.host_rays = np.zeros((N, 8), np.float64)
        self.host_rays[:, 0:3], self.host_rays[:, 3:6], self.host_rays[:, 6] = o, d, np.inf
        self.o, self.d = o, d
        self.rays = torch.from_numpy(self.host_rays).to("cuda:0")
        # every family's largest output here: D levels of 96-byte surface records, and 8 bytes to misalign into
        self.out = torch.zeros((D * N * 96 + 16,), dtype=torch.uint8, device="cuda:0")
        self.surf = torch.zeros((D * N * 96 + 16,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.p_rays, self.p_out, self.p_surf = self.rays.data_ptr(), self.out.data_ptr(), self.surf.data_ptr()
        assert (self.p_rays | self.p_out | self.p_surf) % 16 == 0

    def upload(self, text=LIT):
        self.r.upload(self.rt.Scene.parse(text))
        self.uploaded = True

    def stats_type(self, fam):
        return {"rays": self.rt.rt_query_stats, "paths": self.rt.rt_path_stats}.get(fam, self.rt.rt_radiance_stats)

    def call(self, fam, sync, rays, n, out, depth=D, mode=0, fmt=F64, samples=1, surf=None, on_device=1, st=None):
        """rt_trace_<fam>[_async]; `st` (a stats struct or None) only reaches the synchronous form."""
        L, h, P = self.L, self.h, C.c_void_p
        tail = (on_device, C.byref(st) if st is not None else None) if sync else ()
        if fam == "rays":
            return (L.rt_trace_rays if sync else L.rt_trace_rays_async)(h, mode, P(rays), n, P(out), *tail)
        if fam == "paths":
            return (L.rt_trace_paths if sync else L.rt_trace_paths_async)(h, P(rays), n, depth, P(out), P(surf), *tail)
        if fam == "radiance":
            return (L.rt_trace_radiance if sync else L.rt_trace_radiance_async)(h, P(rays), n, depth, fmt, P(out),
                                                                               *tail)
        assert fam == "resolve"
        fn = L.rt_trace_radiance_resolve if sync else L.rt_trace_radiance_resolve_async
        return fn(h, P(rays), n, samples, None, depth, fmt, P(out), *tail)

    def getter(self, fam):
        return {"rays": self.L.rt_trace_stats, "paths": self.L.rt_path_stats_get}.get(fam,
                                                                                      self.L.rt_radiance_stats_get)

    def stats(self, fam):
        st = self.stats_type(fam)()
        assert self.getter(fam)(self.h, C.byref(st)) == OK
        return st


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.r.close()


@pytest.fixture
def bare(ctx):
    assert not ctx.uploaded, "the no-scene tests run before the first upload (file order)"
    return ctx


@pytest.fixture
def lit(ctx):
    ctx.upload(LIT)
    return ctx


def _zero(st):
    return bytes(st) == bytes(C.sizeof(st))


def _filled(ctx, fam):
    st = ctx.stats_type(fam)()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert not _zero(st)
    return st


# ---- before any upload --------------------------------------------------------------
def test_bare_rays_alignment_comes_before_the_scene(bare):
    c = bare
    assert c.call("rays", False, c.p_rays + 8, N, c.p_out) == INVALID
    assert c.call("rays", False, c.p_rays, N, c.p_out + 8) == INVALID
    # the synchronous form reports the missing scene before it delegates
    assert c.call("rays", True, c.p_rays + 8, N, c.p_out) == NO_SCENE
    assert c.call("rays", True, c.p_rays, N, c.p_out + 8) == NO_SCENE
    assert c.call("rays", False, c.p_rays, N, c.p_out) == NO_SCENE


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("fam", DEEP)
def test_bare_scene_comes_before_alignment(bare, fam, sync):
    c = bare
    assert c.call(fam, sync, c.p_rays + 8, N, c.p_out + 8, surf=c.p_surf + 8) == NO_SCENE
    assert c.call(fam, sync, c.p_rays, N, c.p_out) == NO_SCENE


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("fam", DEEP)
def test_bare_depth_comes_before_the_scene(bare, fam, sync):
    c = bare
    assert c.call(fam, sync, c.p_rays, N, c.p_out, depth=MAX_DEPTH + 1) == DEPTH
    assert c.call(fam, sync, c.p_rays, N, c.p_out, depth=0) == INVALID
    assert c.call(fam, sync, c.p_rays + 8, N, c.p_out + 8, depth=MAX_DEPTH + 1) == DEPTH


@pytest.mark.parametrize("sync", [False, True])
def test_bare_no_rays(bare, sync):
    c = bare
    for mode, want in ((0, OK), (1, OK), (2, INVALID)):
        assert c.call("rays", sync, None, 0, None, mode=mode) == want
    for fam in DEEP:
        assert c.call(fam, sync, None, 0, None, depth=D) == OK
    assert c.call("paths", sync, None, 0, None, depth=0) == INVALID
    assert c.call("paths", sync, None, 0, None, depth=MAX_DEPTH + 1) == DEPTH
    assert c.call("radiance", sync, None, 0, None, fmt=3) == INVALID
    assert c.call("resolve", sync, None, 0, None, samples=0) == INVALID
    assert c.call("resolve", sync, None, 0, None, samples=MAX_SAMPLES + 1) == INVALID
    assert c.call("resolve", sync, None, 0, None, samples=MAX_SAMPLES) == OK


@pytest.mark.parametrize("fam", FAMILIES)
def test_bare_no_rays_zeroes_the_stats(bare, fam):
    st = _filled(bare, fam)
    assert bare.call(fam, True, None, 0, None, st=st) == OK
    assert _zero(st)
    st = _filled(bare, fam)
    assert bare.call(fam, True, None, 0, None, on_device=0, st=st) == OK
    assert _zero(st)


@pytest.mark.parametrize("fam", ("rays", "paths", "radiance"))
def test_bare_getters(bare, fam):
    st = _filled(bare, fam)
    assert bare.getter(fam)(bare.h, C.byref(st)) == OK
    assert _zero(st)  # nothing launched: the rejected calls above are not launches
    assert bare.getter(fam)(bare.h, None) == INVALID
    assert bare.getter(fam)(None, C.byref(st)) == INVALID


# ---- after the upload ------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_upload_misaligned_and_null(lit, fam):
    c = lit
    assert c.call(fam, False, c.p_rays + 8, N, c.p_out, surf=c.p_surf) == INVALID
    assert c.call(fam, False, c.p_rays, N, c.p_out + 8, surf=c.p_surf) == INVALID
    if fam == "paths":
        assert c.call(fam, False, c.p_rays, N, c.p_out, surf=c.p_surf + 8) == INVALID
    for sync in (False, True):
        assert c.call(fam, sync, c.p_rays, N, None, surf=c.p_surf) == INVALID
        assert c.call(fam, sync, None, N, c.p_out, surf=c.p_surf) == INVALID
    assert c.call(fam, False, c.p_rays, N, c.p_out, surf=c.p_surf) == OK  # the pointers themselves are fine
    assert c.stats(fam).rays == N


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("fam", FAMILIES)
def test_upload_too_many_rays(lit, fam, sync):
    c = lit
    # nothing is read: the count is refused first
    assert c.call(fam, sync, c.p_rays, 2 ** 31, c.p_out) == INVALID
    if fam == "resolve":
        assert c.call(fam, sync, c.p_rays, (2 ** 31 - 1) // 4 + 1, c.p_out, samples=4) == INVALID


def test_upload_65_lights(ctx):
    c = ctx
    pos = np.random.default_rng(6).uniform(-6, 6, (65, 3))
    c.upload(TWO + _light_lines(pos) + CAM)
    for sync in (False, True):
        assert c.call("paths", sync, c.p_rays, N, c.p_out) == INVALID
        assert c.call("paths", sync, c.p_rays, N, c.p_out, depth=MAX_DEPTH + 1) == DEPTH
        assert c.call("radiance", sync, c.p_rays, N, c.p_out) == OK
    assert c.stats("radiance").rays == N


def _rejected(c, fam):
    """One call of each kind of refusal for the family; none of them launches."""
    assert c.call(fam, False, c.p_rays + 8, N, c.p_out) == INVALID
    assert c.call(fam, False, c.p_rays, N, None) == INVALID
    assert c.call(fam, True, c.p_rays, 2 ** 31, c.p_out) == INVALID
    if fam == "rays":
        assert c.call(fam, False, c.p_rays, N, c.p_out, mode=2) == INVALID
    else:
        assert c.call(fam, False, c.p_rays, N, c.p_out, depth=MAX_DEPTH + 1) == DEPTH
        assert c.call(fam, True, c.p_rays, N, c.p_out, depth=0) == INVALID


def test_upload_independence(lit):
    c = lit
    counts = {"rays": 65, "paths": 64, "radiance": 63}
    for fam, n in counts.items():
        assert c.call(fam, False, c.p_rays, n, c.p_out) == OK
    for fam in counts:
        _rejected(c, fam)
    _rejected(c, "resolve")
    assert c.call("resolve", True, c.p_rays, 0, c.p_out) == OK  # no rays: not a launch either
    before = {fam: c.stats(fam) for fam in counts}
    assert {fam: st.rays for fam, st in before.items()} == counts
    # a launch of one family leaves the other two getters' answers as they were, kernel_ms included
    again = {"rays": ("rays", 3), "paths": ("paths", 5), "radiance": ("resolve", 7)}
    for fam, (entry, n) in again.items():
        assert c.call(entry, False, c.p_rays, n, c.p_out) == OK
        assert c.stats(fam).rays == n
        for other in counts:
            if other != fam:
                assert bytes(c.stats(other)) == bytes(before[other]), (fam, other)
        before[fam] = c.stats(fam)


def test_upload_host_radiance_reuses_its_staging(lit):
    c = lit
    a, st_a = c.r.trace_radiance(c.o, c.d, D)
    b, st_b = c.r.trace_radiance(c.o[:3], c.d[:3], D)
    a2, st_a2 = c.r.trace_radiance(c.o, c.d, D)
    assert a.tobytes() == a2.tobytes() and (st_a.rays, st_b.rays, st_a2.rays) == (N, 3, N)
    assert b.tobytes() == a[:3].tobytes()
    assert (a != 0).any()


def _host_paths(c, n):
    verts = np.zeros((D, n), c.rt.VERTEX_DTYPE)
    surf = np.full((D, n), FILL, np.uint8).repeat(96, axis=1).view(c.rt.SURFACE_DTYPE)
    assert surf.shape == (D, n) and surf.flags["C_CONTIGUOUS"]
    st = c.rt.rt_path_stats()
    rays = np.ascontiguousarray(c.host_rays[:n])
    assert c.call("paths", True, rays.ctypes.data, n, verts.ctypes.data, surf=surf.ctypes.data, on_device=0,
                  st=st) == OK
    assert st.rays == n
    return verts, surf


def test_upload_host_paths_reuse_their_staging(lit):
    c = lit
    va, sa = _host_paths(c, N)
    vb, sb = _host_paths(c, 3)
    va2, sa2 = _host_paths(c, N)
    assert va.tobytes() == va2.tobytes() and sa.tobytes() == sa2.tobytes()
    assert vb.tobytes() == va[:, :3].tobytes() and sb.tobytes() == sa[:, :3].tobytes()
    for verts, surf in ((va, sa), (vb, sb)):
        traced = (verts["flags"] & TRACED) != 0
        assert traced[0].all() and not traced[D - 1].all()  # sphere 1 does not reflect: its paths end at level 0
        raw = np.ascontiguousarray(surf).view(np.uint8).reshape(D, -1, 96)
        assert (raw[~traced] == FILL).all()  # untraced levels: the caller's bytes, there and back
        assert (raw[traced] != FILL).any(axis=1).all()
