"""ctypes binding of include/rt_hip.h (librt_hip.so) -- the Python host mirror.

This is the binding a reference-side maintainer would add to drive the HIP
render loop from Python; the C++ host (csrc/ray_hip.cpp) uses the same ABI.
Nothing here falls back to a CPU path: if librt_hip.so is missing or no GPU is
visible the calls raise.

Reference interfaces mirrored (file:line in shininglegend/cs420-ray-tracer):
  load_scene            include/scene_loader.h:27-135   -> Scene.load / Scene.parse
  Camera(pos, look, fov) include/camera.h:10-15          -> Camera.from_scene
  trace_ray pixel loop   src/main.cpp:146-157            -> Renderer.render
  launch_gpu_kernel      src/kernel.cu:185-200           -> Renderer.render_async
  write_ppm              src/main.cpp:69-91              -> write_ppm
  find_intersection      include/scene.h:41-61           -> Renderer.trace_rays (RT_QUERY_CLOSEST)
  in_shadow (any hit)    include/scene.h:65-86           -> Renderer.trace_rays (RT_QUERY_OCCLUDED)
  Camera::get_ray        include/camera.h:17-25          -> Renderer.camera_rays
  trace_ray's skeleton   src/main.cpp:16-58              -> Renderer.trace_paths (hits, shadow masks, reflections)
  trace_ray              src/main.cpp:16-58              -> Renderer.trace_radiance (colours of the caller's rays)
  the `-a` sample loop   src/main_gpu.cu:249-333         -> Renderer.render_samples, camera_sample_rays,
                                                            trace_radiance_resolve (a caller's pattern and weights),
                                                            Renderer.render_samples_async (one fused launch),
                                                            Group.render_samples (row-sharded over a group)
  a pinhole only         include/camera.h:17-25          -> Renderer.camera_lens_rays, render_lens_samples[_async],
                                                            Group.render_lens_samples, lens_pattern (a thin lens:
                                                            depth of field for the multi-sample renders)
  point lights only      include/scene.h:94-120          -> Renderer.set_light_samples, Group.set_light_samples,
                                                            light_pattern (per-sample light positions: area
                                                            lights, soft shadows, for the multi-sample renders)
  a perfect mirror       src/main.cpp:45-48              -> Renderer.set_gloss_samples, Group.set_gloss_samples,
                                                            gloss_pattern, scene_roughness (the scene files'
                                                            roughness column, which scene_loader.h:66-70 drops:
                                                            glossy reflections for the multi-sample renders)
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# RT_HIP_LIB selects an alternative build of the same ABI (tuning experiments).
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(HERE, "librt_hip.so")
# Test builds of the same sources (csrc/Makefile), selected per context with
# Renderer(variant=...): "tuning" reads every layout / grid knob (RT_TUNING),
# "check" range-checks every indirect device index (RT_CHECK).  The product
# build reads only RT_HIP_LDS_SCENE and RT_HIP_CAM_GRID.
VARIANTS = {"tuning": os.path.join(HERE, "variants", "librt_hip_tuning.so"),
            "check": os.path.join(HERE, "variants", "librt_hip_check.so")}

RT_MAX_DEPTH = 64
RT_MAX_GLOSS_BOUNCES = RT_MAX_DEPTH - 1
ABI_VERSION = 12  # RT_HIP_ABI_VERSION in include/rt_hip.h
MAX_FRAMES = 32  # RT_MAX_FRAMES


class RtError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        super().__init__(f"{what}: {status_string(status)}" + (f" ({detail})" if detail else ""))


class rt_sphere(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("color", C.c_double * 3),
                ("reflectivity", C.c_double), ("shininess", C.c_double)]


class rt_light(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("color", C.c_double * 3), ("intensity", C.c_double)]


class rt_scene(C.Structure):
    _fields_ = [("num_spheres", C.c_int32), ("num_lights", C.c_int32),
                ("spheres", C.POINTER(rt_sphere)), ("lights", C.POINTER(rt_light)),
                ("ambient", C.c_double * 3), ("cam_position", C.c_double * 3),
                ("cam_look_at", C.c_double * 3), ("cam_fov", C.c_double),
                ("has_camera", C.c_int32), ("warnings", C.c_int32)]


class rt_camera(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("forward", C.c_double * 3), ("right", C.c_double * 3),
                ("up", C.c_double * 3), ("scale", C.c_double)]


class rt_info(C.Structure):
    _fields_ = [("cam_grid_last", C.c_int32), ("cam_grid_n", C.c_int32), ("cam_grid_builds", C.c_uint64),
                ("cam_grid_build_ms", C.c_double), ("tile_order_builds", C.c_uint64),
                ("tile_order_build_ms", C.c_double), ("upload_ms", C.c_double), ("launches", C.c_uint64),
                ("sphere_grids", C.c_int32), ("sphere_grid_n", C.c_int32), ("sphere_grid_entries", C.c_uint64),
                ("sphere_grid_build_ms", C.c_double), ("behind_grid", C.c_int32), ("behind_grid_last", C.c_int32),
                ("behind_grid_cells", C.c_uint64), ("behind_grid_entries", C.c_uint64),
                ("behind_grid_build_ms", C.c_double), ("bvh_build_ms", C.c_double),
                ("light_grid_build_ms", C.c_double), ("scratch_bytes", C.c_uint64),
                ("shadow_line_bounded", C.c_int32), ("reserved0", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class rt_ray_table_info(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("used_last", C.c_int32), ("reserved0", C.c_int32), ("bytes", C.c_uint64),
                ("build_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class rt_tile(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class rt_rows(C.Structure):
    _fields_ = [("band", C.c_int32), ("first", C.c_int32), ("stride", C.c_int32), ("count", C.c_int32)]


class rt_stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_shadow", C.c_uint64), ("rays_reflect", C.c_uint64),
                ("negative_clamped", C.c_uint64), ("kernel_ms", C.c_double), ("tests_exact", C.c_uint64),
                ("tests_cull", C.c_uint64)]

    def as_dict(self):
        return {"primary": self.rays_primary, "shadow": self.rays_shadow, "reflect": self.rays_reflect,
                "negative": self.negative_clamped, "kernel_ms": self.kernel_ms, "tests_exact": self.tests_exact,
                "tests_cull": self.tests_cull}

    @property
    def rays(self) -> int:
        return self.rays_primary + self.rays_shadow + self.rays_reflect


# Ray queries (rt_trace_rays): a caller's ray, its answer, the launch's counts.
class rt_ray(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3), ("tmax", C.c_double),
                ("reserved", C.c_double)]


class rt_hit(C.Structure):
    _fields_ = [("t", C.c_double), ("sphere", C.c_int32), ("occluded", C.c_int32)]


class rt_query_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("tests_exact", C.c_uint64), ("tests_cull", C.c_uint64),
                ("rays_unaccelerated", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_QUERY_CLOSEST, RT_QUERY_OCCLUDED = 0, 1


# Path queries (rt_trace_paths): a level's vertex, its optional surface record, the launch's counts.
class rt_vertex(C.Structure):
    _fields_ = [("t", C.c_double), ("sphere", C.c_int32), ("flags", C.c_int32), ("shadowed", C.c_uint64),
                ("reserved", C.c_uint64)]


class rt_surface(C.Structure):
    _fields_ = [("dir", C.c_double * 3), ("hit", C.c_double * 3), ("normal", C.c_double * 3),
                ("view", C.c_double * 3)]


class rt_path_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("segments", C.c_uint64), ("hits", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("tests_exact", C.c_uint64), ("tests_cull", C.c_uint64), ("unaccelerated", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# Radiance queries (rt_trace_radiance): the launch's counts.
class rt_radiance_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("segments", C.c_uint64), ("hits", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("tests_exact", C.c_uint64), ("tests_cull", C.c_uint64), ("unaccelerated", C.c_uint64),
                ("negative_clamped", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_PATH_MAX_LIGHTS = 64
RT_VERTEX_TRACED, RT_VERTEX_REFLECTS = 1, 2
# numpy views of rt_vertex / rt_surface records (Renderer.trace_paths); built on first use
_PATH_DTYPES = {}


def _path_dtype(name: str):
    if not _PATH_DTYPES:
        import numpy as np

        _PATH_DTYPES["VERTEX_DTYPE"] = np.dtype([("t", np.float64), ("sphere", np.int32), ("flags", np.int32),
                                                 ("shadowed", np.uint64), ("reserved", np.uint64)])
        _PATH_DTYPES["SURFACE_DTYPE"] = np.dtype([("dir", np.float64, 3), ("hit", np.float64, 3),
                                                  ("normal", np.float64, 3), ("view", np.float64, 3)])
    return _PATH_DTYPES[name]


def __getattr__(name):  # VERTEX_DTYPE / SURFACE_DTYPE without importing numpy at module import
    if name in ("VERTEX_DTYPE", "SURFACE_DTYPE"):
        return _path_dtype(name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

# Every symbol include/rt_hip.h declares, with its ctypes signature.
_P = C.c_void_p
SIGNATURES = {
    "rt_scene_load": (C.c_int, [C.c_char_p, C.POINTER(rt_scene), C.c_int]),
    "rt_scene_parse": (C.c_int, [C.c_char_p, C.POINTER(rt_scene), C.c_int]),
    "rt_scene_free": (None, [C.POINTER(rt_scene)]),
    "rt_camera_from_scene": (C.c_int, [C.POINTER(rt_scene), C.POINTER(rt_camera)]),
    "rt_write_ppm": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int, C.c_int]),
    "rt_error_string": (C.c_char_p, [C.c_int]),
    "rt_abi_version": (C.c_int, []),
    "rt_rows_for_shard": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows)]),
    "rt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rt_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rt_destroy": (None, [_P]),
    "rt_last_error": (C.c_char_p, [_P]),
    "rt_set_stream": (C.c_int, [_P, _P]),
    "rt_upload_scene": (C.c_int, [_P, C.POINTER(rt_scene)]),
    "rt_set_culling": (C.c_int, [_P, C.c_int]),
    "rt_render": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows), _P,
                            C.c_int, C.POINTER(rt_stats)]),
    "rt_render_async": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows), _P]),
    "rt_render_stats": (C.c_int, [_P, C.POINTER(rt_stats)]),
    "rt_render_frames_async": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(rt_rows), _P, C.c_size_t]),
    "rt_kernel_times": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "rt_unpermute_rows": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rt_render_tile": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, _P]),
    "rt_render_tiles": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_tile), C.c_int,
                                  C.c_int, _P]),
    "rt_set_antialias": (C.c_int, [_P, C.c_int]),
    "rt_get_info": (C.c_int, [_P, C.POINTER(rt_info)]),
    "rt_get_ray_table_info": (C.c_int, [_P, C.POINTER(rt_ray_table_info)]),
    "rt_set_ray_table": (C.c_int, [_P, C.c_int, C.c_int64]),
    "rt_trace_rays_async": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P]),
    "rt_trace_rays": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P, C.c_int, C.POINTER(rt_query_stats)]),
    "rt_trace_stats": (C.c_int, [_P, C.POINTER(rt_query_stats)]),
    "rt_camera_rays": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.POINTER(rt_rows), _P]),
    "rt_trace_paths_async": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "rt_trace_paths": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, C.c_int, C.POINTER(rt_path_stats)]),
    "rt_path_stats_get": (C.c_int, [_P, C.POINTER(rt_path_stats)]),
    "rt_trace_radiance_async": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, _P]),
    "rt_trace_radiance": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, _P, C.c_int,
                                    C.POINTER(rt_radiance_stats)]),
    "rt_radiance_stats_get": (C.c_int, [_P, C.POINTER(rt_radiance_stats)]),
    "rt_camera_sample_rays": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.POINTER(rt_rows),
                                        C.POINTER(C.c_double), C.c_int, _P]),
    "rt_trace_radiance_resolve_async": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.c_int,
                                                  C.c_int, _P]),
    "rt_trace_radiance_resolve": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                                            _P, C.c_int, C.POINTER(rt_radiance_stats)]),
    "rt_render_samples": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows),
                                    C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, _P, C.c_int,
                                    C.c_size_t, C.POINTER(rt_radiance_stats)]),
    "rt_render_samples_async": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows),
                                          C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, _P]),
    "rt_group_render_samples": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.c_int, C.POINTER(C.c_double), C.c_int, _P, C.c_int,
                                          C.POINTER(rt_radiance_stats)]),
    "rt_camera_lens_rays": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.POINTER(rt_rows),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int, _P]),
    "rt_render_lens_samples_async": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int,
                                               C.POINTER(rt_rows), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, _P]),
    "rt_render_lens_samples": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.POINTER(rt_rows),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                         C.POINTER(C.c_double), C.c_int, _P, C.c_int,
                                         C.POINTER(rt_radiance_stats)]),
    "rt_group_render_lens_samples": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                               C.POINTER(C.c_double), C.c_int, _P, C.c_int,
                                               C.POINTER(rt_radiance_stats)]),
    "rt_set_light_samples": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
    "rt_group_set_light_samples": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
    "rt_set_gloss_samples": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int]),
    "rt_group_set_gloss_samples": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int]),
    "rt_scene_parse_roughness": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "rt_scene_load_roughness": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "rt_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(_P)]),
    "rt_group_destroy": (None, [_P]),
    "rt_group_size": (C.c_int, [_P]),
    "rt_group_member": (_P, [_P, C.c_int]),
    "rt_group_last_error": (C.c_char_p, [_P]),
    "rt_group_upload_scene": (C.c_int, [_P, C.POINTER(rt_scene)]),
    "rt_group_set_antialias": (C.c_int, [_P, C.c_int]),
    "rt_group_render": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, _P, C.c_int,
                                  C.POINTER(rt_stats)]),
    "rt_group_render_frames": (C.c_int, [_P, C.POINTER(rt_camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                         C.c_int, C.c_size_t, C.POINTER(rt_stats)]),
}

# include/rt_hip_compat.h: the reference's hybrid interface (src/kernel.cu:185-207),
# struct layouts of include/gpu_shared.h:84-171
class rt_float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class rt_gpu_material(C.Structure):
    _fields_ = [("albedo", rt_float3), ("metallic", C.c_float), ("shininess", C.c_float)]


class rt_gpu_sphere(C.Structure):
    _fields_ = [("center", rt_float3), ("radius", C.c_float), ("material", rt_gpu_material)]


class rt_gpu_light(C.Structure):
    _fields_ = [("position", rt_float3), ("color", rt_float3), ("intensity", C.c_float)]


class rt_gpu_camera(C.Structure):
    _fields_ = [("origin", rt_float3), ("lower_left", rt_float3), ("horizontal", rt_float3),
                ("vertical", rt_float3), ("forward", rt_float3), ("right", rt_float3), ("up", rt_float3),
                ("fov", C.c_float)]


COMPAT_SIGNATURES = {
    "launch_gpu_kernel": (None, [C.POINTER(rt_float3), C.POINTER(rt_gpu_sphere), C.c_int, C.c_int,
                                 C.POINTER(rt_gpu_camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, _P]),
    "upload_lights_and_ambience": (None, [C.POINTER(rt_gpu_light), C.c_int, rt_float3]),
    "rt_compat_status": (C.c_int, []),
}

# framebuffer formats of rt_render_tile and record formats of rt_trace_radiance (rt_hip.h)
RT_FB_RGB8, RT_FB_F32X3, RT_FB_F64X3 = 0, 1, 2

_libs = {}


def lib(path: str = LIB_PATH):
    """Load librt_hip.so (or a test variant of it; raises if it has not been built)."""
    _lib = _libs.get(path)
    if _lib is None:
        # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  If it
        # is importable, load it first so the dynamic linker binds librt_hip.so
        # to that same HIP runtime: two runtimes in one process cannot share
        # the device (torch then reports "No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(path)
        for name, (res, args) in list(SIGNATURES.items()) + list(COMPAT_SIGNATURES.items()):
            if os.environ.get("RT_HIP_LIB") and not hasattr(L, name):
                continue  # an older diagnostic build (RT_HIP_LIB) may predate an entry point
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _libs[path] = _lib = L
    return _lib


def variant_lib(variant: str | None):
    """The library of a test variant ("tuning", "check") or the product's (None)."""
    if variant is None:
        return lib()
    if variant not in VARIANTS:
        raise ValueError(f"unknown librt_hip variant {variant!r} (one of {sorted(VARIANTS)})")
    return lib(VARIANTS[variant])


def status_string(status: int) -> str:
    try:
        return lib().rt_error_string(status).decode()
    except Exception:  # pragma: no cover - only when the library itself is missing
        return f"status {status}"


def _check(rc: int, what: str, ctx=None, L=None):
    if rc != 0:
        detail = (L or lib()).rt_last_error(ctx).decode() if ctx else ""
        raise RtError(rc, what, detail)


class Scene:
    """A parsed scene (owns the C arrays).  Mirrors load_scene(), scene_loader.h:27."""

    def __init__(self):
        self._s = rt_scene()
        self._owned = False

    @classmethod
    def load(cls, path: str, verbose: bool = False) -> "Scene":
        s = cls()
        _check(lib().rt_scene_load(os.fsencode(path), C.byref(s._s), int(verbose)), f"rt_scene_load({path})")
        s._owned = True
        return s

    @classmethod
    def parse(cls, text: str, verbose: bool = False) -> "Scene":
        s = cls()
        _check(lib().rt_scene_parse(text.encode(), C.byref(s._s), int(verbose)), "rt_scene_parse")
        s._owned = True
        return s

    @property
    def raw(self) -> rt_scene:
        return self._s

    @property
    def num_spheres(self) -> int:
        return self._s.num_spheres

    @property
    def num_lights(self) -> int:
        return self._s.num_lights

    @property
    def warnings(self) -> int:
        return self._s.warnings

    def sphere(self, i: int) -> dict:
        sp = self._s.spheres[i]
        return {"center": tuple(sp.center), "radius": sp.radius, "color": tuple(sp.color),
                "reflectivity": sp.reflectivity, "shininess": sp.shininess}

    def light(self, i: int) -> dict:
        L = self._s.lights[i]
        return {"position": tuple(L.position), "color": tuple(L.color), "intensity": L.intensity}

    def camera(self) -> rt_camera:
        cam = rt_camera()
        _check(lib().rt_camera_from_scene(C.byref(self._s), C.byref(cam)), "rt_camera_from_scene")
        return cam

    def close(self):
        if self._owned:
            lib().rt_scene_free(C.byref(self._s))
            self._owned = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_array(cams) -> C.Array:
    """The rt_camera array rt_render_frames_async takes, built once (a caller
    that launches the same frames repeatedly keeps it off its launch path)."""
    return (rt_camera * len(cams))(*cams)


def rows_for_shard(height: int, band: int, rank: int, world: int) -> rt_rows:
    """Cyclic bands of `band` rows: rank r renders bands r, r+G, r+2G, ...
    (rt_rows_for_shard: the one layout ray_hip --gpus and bench.py share)."""
    rows = rt_rows()
    _check(lib().rt_rows_for_shard(height, band, rank, world, C.byref(rows)),
           f"rt_rows_for_shard({height}, {band}, {rank}, {world})")
    return rows


class Renderer:
    """One device context (rt_ctx).  Mirrors GPUResources + launch_gpu_kernel."""

    def __init__(self, device: int = 0, variant: str | None = None):
        """variant: None = the product library; "tuning" / "check" = a test build (VARIANTS)."""
        self._L = variant_lib(variant)
        self.variant = variant
        self._ctx = C.c_void_p()
        _check(self._L.rt_create(device, C.byref(self._ctx)), f"rt_create({device})", L=self._L)
        self.device = device

    @property
    def handle(self):
        return self._ctx

    def set_stream(self, stream_ptr: int | None):
        _check(self._L.rt_set_stream(self._ctx, C.c_void_p(stream_ptr or 0)), "rt_set_stream", self._ctx, L=self._L)

    def set_culling(self, enable: bool):
        _check(self._L.rt_set_culling(self._ctx, int(enable)), "rt_set_culling", self._ctx, L=self._L)

    def upload(self, scene: Scene):
        _check(self._L.rt_upload_scene(self._ctx, C.byref(scene.raw)), "rt_upload_scene", self._ctx, L=self._L)
        self._num_lights = scene.num_lights
        self._num_spheres = scene.num_spheres

    def set_gloss_samples(self, roughness, table):
        """rt_set_gloss_samples: glossy reflections for the multi-sample calls.  `roughness`: num_spheres
        doubles (e.g. scene_roughness(path)); `table`: an [S][B][3] array-like (e.g. gloss_pattern(n, B)), the
        point that bends sample s's reflection ray at bounce b, scaled by the roughness of the sphere it
        leaves; None clears the table.  While it is set, trace_radiance_resolve, render_samples[_async] and
        render_lens_samples[_async] take S samples; upload() clears it."""
        rough, tab, s, b = _gloss_table(roughness, table, getattr(self, "_num_spheres", None))
        _check(self._L.rt_set_gloss_samples(self._ctx, rough, tab, s, b), "rt_set_gloss_samples", self._ctx,
               L=self._L)

    def set_light_samples(self, offsets):
        """rt_set_light_samples: area lights for the multi-sample calls.  `offsets`: an [S][num_lights][3]
        array-like (e.g. light_pattern(n, r, scene.num_lights)), the offset of light l for sample s, added to
        its uploaded position; None clears the table.  While it is set, trace_radiance_resolve,
        render_samples[_async] and render_lens_samples[_async] take S samples and shade sample s under the
        moved lights; upload() clears it."""
        tab, s = _light_table(offsets, getattr(self, "_num_lights", None))
        _check(self._L.rt_set_light_samples(self._ctx, tab, s), "rt_set_light_samples", self._ctx, L=self._L)

    def render(self, cam: rt_camera, width: int, height: int, depth: int, rows: rt_rows | None = None,
               out=None, out_on_device: bool = False) -> tuple[object, rt_stats]:
        """Render into `out` (host bytearray/numpy if None) and return (buffer, stats)."""
        count = rows.count if rows is not None else height
        if out is None:
            out = bytearray(count * width * 3)
        ptr = _addr(out)
        st = rt_stats()
        _check(self._L.rt_render(self._ctx, C.byref(cam), width, height, depth,
                               C.byref(rows) if rows is not None else None, C.c_void_p(ptr), int(out_on_device),
                               C.byref(st)), "rt_render", self._ctx, L=self._L)
        return out, st

    def render_async(self, cam: rt_camera, width: int, height: int, depth: int, rows: rt_rows | None,
                     out_device_ptr: int):
        _check(self._L.rt_render_async(self._ctx, C.byref(cam), width, height, depth,
                                     C.byref(rows) if rows is not None else None, C.c_void_p(out_device_ptr)),
               "rt_render_async", self._ctx, L=self._L)

    def render_frames_async(self, cams, width: int, height: int, depth: int, rows: rt_rows | None,
                            out_device_ptr: int, frame_stride: int):
        """rt_render_frames_async: len(cams) frames (<= MAX_FRAMES) in one launch, frame f
        (seen through cams[f]) at out_device_ptr + f * frame_stride.  `cams` may
        be a ctypes array of rt_camera built beforehand (camera_array)."""
        arr = cams if isinstance(cams, C.Array) else (rt_camera * len(cams))(*cams)
        _check(self._L.rt_render_frames_async(self._ctx, arr, len(cams), width, height, depth,
                                            C.byref(rows) if rows is not None else None,
                                            C.c_void_p(out_device_ptr), frame_stride),
               "rt_render_frames_async", self._ctx, L=self._L)

    def set_antialias(self, samples: int):
        """1 = the serial path, 4 = the reference GPU's `-a` mode (main_gpu.cu:249-333)."""
        _check(self._L.rt_set_antialias(self._ctx, samples), "rt_set_antialias", self._ctx, L=self._L)

    def render_tile(self, cam: rt_camera, width: int, height: int, depth: int, tile_x: int, tile_y: int,
                    tile_w: int, tile_h: int, fb_format: int, fb_device_ptr: int):
        """launch_gpu_kernel tile semantics (kernel.cu:185-200) into a full-image device framebuffer."""
        _check(self._L.rt_render_tile(self._ctx, C.byref(cam), width, height, depth, tile_x, tile_y, tile_w, tile_h,
                                    fb_format, C.c_void_p(fb_device_ptr)), "rt_render_tile", self._ctx, L=self._L)

    def render_tiles(self, cam: rt_camera, width: int, height: int, depth: int, tiles, fb_format: int,
                     fb_device_ptr: int):
        """rt_render_tiles: every (x, y, w, h) tile of `tiles` in ONE launch (the 8x8 blocks covering them)."""
        arr = (rt_tile * max(1, len(tiles)))(*[rt_tile(*t) for t in tiles])
        _check(self._L.rt_render_tiles(self._ctx, C.byref(cam), width, height, depth, arr, len(tiles), fb_format,
                                     C.c_void_p(fb_device_ptr)), "rt_render_tiles", self._ctx, L=self._L)

    def stats(self) -> rt_stats:
        st = rt_stats()
        _check(self._L.rt_render_stats(self._ctx, C.byref(st)), "rt_render_stats", self._ctx, L=self._L)
        return st

    def info(self) -> rt_info:
        """rt_get_info: the host-side builds the render calls made (camera grid, tile order)."""
        inf = rt_info()
        _check(self._L.rt_get_info(self._ctx, C.byref(inf)), "rt_get_info", self._ctx, L=self._L)
        return inf

    def ray_table_info(self) -> rt_ray_table_info:
        """rt_get_ray_table_info: the ray table's builds, and whether the most recent launch read one."""
        inf = rt_ray_table_info()
        _check(self._L.rt_get_ray_table_info(self._ctx, C.byref(inf)), "rt_get_ray_table_info", self._ctx, L=self._L)
        return inf

    def set_ray_table(self, mode: int = 1, budget_bytes: int = -1):
        """rt_set_ray_table: 0 never a ray table, 1 the default rule, 2 also for a first one-frame launch; the
        bytes a table may take (negative: the default)."""
        _check(self._L.rt_set_ray_table(self._ctx, mode, budget_bytes), "rt_set_ray_table", self._ctx, L=self._L)

    def kernel_times(self, max_n: int = 256) -> list[float]:
        """Per-launch kernel durations (ms) since the previous call (syncs the stream)."""
        buf = (C.c_double * max_n)()
        n = C.c_int(0)
        _check(self._L.rt_kernel_times(self._ctx, buf, max_n, C.byref(n)), "rt_kernel_times", self._ctx, L=self._L)
        return list(buf[: n.value])

    def unpermute(self, gathered_ptr: int, image_ptr: int, width: int, height: int, band: int, shards: int,
                  rows_per_shard: int):
        _check(self._L.rt_unpermute_rows(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(image_ptr), width, height,
                                       band, shards, rows_per_shard), "rt_unpermute_rows", self._ctx, L=self._L)

    def trace_rays(self, origins, directions, tmax=None, mode: int = RT_QUERY_CLOSEST):
        """rt_trace_rays from host memory: ray i = Ray(origins[i], directions[i]) (numpy
        [n, 3]; any direction length), tmax a scalar or [n] (None = +inf).  Returns
        (t, sphere, occluded, stats): numpy float64 / int32 / int32 arrays of n and
        the launch's rt_query_stats."""
        import numpy as np

        rays = _pack_rays(origins, directions, np.inf if tmax is None else tmax)
        n = rays.shape[0]
        hits = np.zeros(n, np.dtype([("t", np.float64), ("sphere", np.int32), ("occluded", np.int32)]))
        st = rt_query_stats()
        _check(self._L.rt_trace_rays(self._ctx, mode, C.c_void_p(rays.ctypes.data), n, C.c_void_p(hits.ctypes.data), 0,
                                     C.byref(st)), "rt_trace_rays", self._ctx, L=self._L)
        return hits["t"].copy(), hits["sphere"].copy(), hits["occluded"].copy(), st

    def trace_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, mode: int = RT_QUERY_CLOSEST):
        """rt_trace_rays_async: n rt_ray records at rays_ptr, n rt_hit records written at
        hits_ptr (device memory, 16-byte aligned), enqueued on the context's stream."""
        _check(self._L.rt_trace_rays_async(self._ctx, mode, C.c_void_p(rays_ptr), n, C.c_void_p(hits_ptr)),
               "rt_trace_rays_async", self._ctx, L=self._L)

    def trace_stats(self) -> rt_query_stats:
        """rt_trace_stats: waits for the stream; the most recent query launch."""
        st = rt_query_stats()
        _check(self._L.rt_trace_stats(self._ctx, C.byref(st)), "rt_trace_stats", self._ctx, L=self._L)
        return st

    def camera_rays(self, cam: rt_camera, width: int, height: int, rows: rt_rows | None, rays_ptr: int):
        """rt_camera_rays: the view's camera rays (get_ray's, camera.h:17-25) as rt_ray
        records at rays_ptr (device memory, rows.count * width of them), asynchronously."""
        _check(self._L.rt_camera_rays(self._ctx, C.byref(cam), width, height,
                                      C.byref(rows) if rows is not None else None, C.c_void_p(rays_ptr)),
               "rt_camera_rays", self._ctx, L=self._L)

    def trace_paths(self, origins, directions, depth: int, surfaces: bool = False):
        """rt_trace_paths from host memory: the path of Ray(origins[i], directions[i]) (numpy
        [n, 3]; any direction length) through `depth` levels of trace_ray.  Returns
        (verts, surf, stats): numpy structured arrays shaped [depth, n] of VERTEX_DTYPE and
        SURFACE_DTYPE (surf is None without `surfaces`; the surface records of untraced
        levels are zeros) and the launch's rt_path_stats."""
        import numpy as np

        rays = _pack_rays(origins, directions)
        n = rays.shape[0]
        verts = np.zeros((max(depth, 0), n), _path_dtype("VERTEX_DTYPE"))
        surf = np.zeros((max(depth, 0), n), _path_dtype("SURFACE_DTYPE")) if surfaces else None
        st = rt_path_stats()
        _check(self._L.rt_trace_paths(self._ctx, C.c_void_p(rays.ctypes.data), n, depth, C.c_void_p(verts.ctypes.data),
                                      C.c_void_p(surf.ctypes.data) if surfaces else None, 0, C.byref(st)),
               "rt_trace_paths", self._ctx, L=self._L)
        return verts, surf, st

    def trace_paths_device(self, rays_ptr: int, n: int, depth: int, verts_ptr: int, surf_ptr: int = 0):
        """rt_trace_paths_async: n rt_ray records at rays_ptr; depth * n rt_vertex records written
        at verts_ptr and, with surf_ptr, the traced levels' rt_surface records there (device
        memory, 16-byte aligned, level-major), enqueued on the context's stream."""
        _check(self._L.rt_trace_paths_async(self._ctx, C.c_void_p(rays_ptr), n, depth, C.c_void_p(verts_ptr),
                                            C.c_void_p(surf_ptr) if surf_ptr else None),
               "rt_trace_paths_async", self._ctx, L=self._L)

    def path_stats(self) -> rt_path_stats:
        """rt_path_stats_get: waits for the stream; the most recent path launch."""
        st = rt_path_stats()
        _check(self._L.rt_path_stats_get(self._ctx, C.byref(st)), "rt_path_stats_get", self._ctx, L=self._L)
        return st

    def trace_radiance(self, origins, directions, depth: int, fmt: int = RT_FB_F64X3):
        """rt_trace_radiance from host memory: trace_ray's colour of Ray(origins[i], directions[i])
        (numpy [n, 3]; any direction length) at `depth`.  Returns (colours, stats): a numpy [n, 3]
        array of the format's dtype (float64 for RT_FB_F64X3, float32 for RT_FB_F32X3, uint8 for
        RT_FB_RGB8), ray i in row i, and the launch's rt_radiance_stats."""
        import numpy as np

        rays = _pack_rays(origins, directions)
        n = rays.shape[0]
        out = np.zeros((n, 3), _fb_dtype(fmt, np.float64))
        st = rt_radiance_stats()
        _check(self._L.rt_trace_radiance(self._ctx, C.c_void_p(rays.ctypes.data), n, depth, fmt,
                                         C.c_void_p(out.ctypes.data), 0, C.byref(st)),
               "rt_trace_radiance", self._ctx, L=self._L)
        return out, st

    def trace_radiance_device(self, rays_ptr: int, n: int, depth: int, fmt: int, out_ptr: int):
        """rt_trace_radiance_async: n rt_ray records at rays_ptr, n packed records of `fmt` written
        at out_ptr (device memory, 16-byte aligned), enqueued on the context's stream."""
        _check(self._L.rt_trace_radiance_async(self._ctx, C.c_void_p(rays_ptr), n, depth, fmt, C.c_void_p(out_ptr)),
               "rt_trace_radiance_async", self._ctx, L=self._L)

    def radiance_stats(self) -> rt_radiance_stats:
        """rt_radiance_stats_get: waits for the stream; the most recent radiance launch."""
        st = rt_radiance_stats()
        _check(self._L.rt_radiance_stats_get(self._ctx, C.byref(st)), "rt_radiance_stats_get", self._ctx, L=self._L)
        return st

    def camera_sample_rays(self, cam: rt_camera, width: int, height: int, rows: rt_rows | None, offsets,
                           rays_ptr: int):
        """rt_camera_sample_rays: len(offsets) rays per pixel ((ox, oy) pairs, e.g. grid_pattern(n)) as
        rt_ray records at rays_ptr (device memory, rows.count * width * len(offsets) of them, a
        pixel's samples consecutive), asynchronously."""
        off, s = _doubles(offsets, 2)
        _check(self._L.rt_camera_sample_rays(self._ctx, C.byref(cam), width, height,
                                             C.byref(rows) if rows is not None else None, off, s,
                                             C.c_void_p(rays_ptr)),
               "rt_camera_sample_rays", self._ctx, L=self._L)

    def trace_radiance_resolve(self, origins, directions, samples: int, depth: int, weights=None,
                               fmt: int = RT_FB_F64X3):
        """rt_trace_radiance_resolve from host memory: numpy [n_pixels * samples, 3] origins and
        directions, pixel p's samples in rows p*samples .. p*samples + samples - 1; weights None (the
        box filter) or `samples` doubles.  Returns (pixels, stats): a numpy [n_pixels, 3] array of
        the format's dtype and the launch's rt_radiance_stats."""
        import numpy as np

        rays = _pack_rays(origins, directions)
        n = rays.shape[0]
        if samples >= 1 and n % samples:
            raise ValueError(f"{n} rays are not a multiple of {samples} samples")
        npix = n // samples if samples >= 1 else n
        out = np.zeros((npix, 3), _fb_dtype(fmt, np.float64))
        w = _sample_weights(weights, samples)
        st = rt_radiance_stats()
        _check(self._L.rt_trace_radiance_resolve(self._ctx, C.c_void_p(rays.ctypes.data), npix, samples, w, depth,
                                                 fmt, C.c_void_p(out.ctypes.data), 0, C.byref(st)),
               "rt_trace_radiance_resolve", self._ctx, L=self._L)
        return out, st

    def trace_radiance_resolve_device(self, rays_ptr: int, n_pixels: int, samples: int, depth: int, fmt: int,
                                      out_ptr: int, weights=None):
        """rt_trace_radiance_resolve_async: n_pixels * samples rt_ray records at rays_ptr, n_pixels
        packed records of `fmt` written at out_ptr (device memory, 16-byte aligned), enqueued on
        the context's stream."""
        w = _sample_weights(weights, samples)
        _check(self._L.rt_trace_radiance_resolve_async(self._ctx, C.c_void_p(rays_ptr), n_pixels, samples, w, depth,
                                                       fmt, C.c_void_p(out_ptr)),
               "rt_trace_radiance_resolve_async", self._ctx, L=self._L)

    def render_samples(self, cam: rt_camera, width: int, height: int, depth: int, offsets, weights=None,
                       rows: rt_rows | None = None, fmt: int = RT_FB_RGB8, out=None, out_on_device: bool = False,
                       max_ray_bytes: int = 0):
        """rt_render_samples: the pixels of `rows` (None = the full frame) in PPM row order, each
        resolved from len(offsets) samples ((ox, oy) pairs; weights None = the box filter).  `out`:
        None (a host numpy [count * width, 3] array of the format's dtype is made), a host buffer,
        or with out_on_device a device buffer / pointer.  Returns (out, stats), the stats summed
        over the call's chunks of at most max_ray_bytes of rays (0 = the library's default)."""
        off, s = _doubles(offsets, 2)
        w = _sample_weights(weights, s)
        count = rows.count if rows is not None else height
        if out is None:
            import numpy as np

            out = np.zeros((max(count, 0) * width, 3), _fb_dtype(fmt, np.uint8))
        ptr = out if isinstance(out, int) else _addr(out)
        st = rt_radiance_stats()
        _check(self._L.rt_render_samples(self._ctx, C.byref(cam), width, height, depth,
                                         C.byref(rows) if rows is not None else None, off, s, w, fmt,
                                         C.c_void_p(ptr), int(out_on_device), max_ray_bytes, C.byref(st)),
               "rt_render_samples", self._ctx, L=self._L)
        return out, st

    def render_samples_async(self, cam: rt_camera, width: int, height: int, depth: int, offsets, out_ptr: int,
                             weights=None, rows: rt_rows | None = None, fmt: int = RT_FB_RGB8):
        """rt_render_samples_async: render_samples' records of `rows` (None = the full frame) written
        at out_ptr (device memory, 16-byte aligned) by one launch that forms its own rays, enqueued
        on the context's stream; radiance_stats() afterwards reports it."""
        off, s = _doubles(offsets, 2)
        w = _sample_weights(weights, s)
        _check(self._L.rt_render_samples_async(self._ctx, C.byref(cam), width, height, depth,
                                               C.byref(rows) if rows is not None else None, off, s, w, fmt,
                                               C.c_void_p(out_ptr)),
               "rt_render_samples_async", self._ctx, L=self._L)

    def camera_lens_rays(self, cam: rt_camera, width: int, height: int, rows: rt_rows | None, offsets, lens,
                         focus: float, rays_ptr: int):
        """rt_camera_lens_rays: camera_sample_rays through a thin lens.  Sample s leaves the lens point
        lens[s] ((lx, ly) pairs in scene units along the camera's right and up, e.g. lens_pattern(n, r))
        towards the point its pinhole ray meets on the plane `focus` along forward."""
        off, s = _doubles(offsets, 2)
        ln = _lens_points(lens, s)
        _check(self._L.rt_camera_lens_rays(self._ctx, C.byref(cam), width, height,
                                           C.byref(rows) if rows is not None else None, off, ln, float(focus), s,
                                           C.c_void_p(rays_ptr)),
               "rt_camera_lens_rays", self._ctx, L=self._L)

    def render_lens_samples(self, cam: rt_camera, width: int, height: int, depth: int, offsets, lens, focus: float,
                            weights=None, rows: rt_rows | None = None, fmt: int = RT_FB_RGB8, out=None,
                            out_on_device: bool = False):
        """rt_render_lens_samples: render_samples with depth of field, as one fused launch.  `lens`:
        one (lx, ly) pair per offset; `focus`: the distance of the plane that stays sharp.  `out` as
        render_samples'.  Returns (out, stats), the stats that one launch's."""
        off, s = _doubles(offsets, 2)
        ln = _lens_points(lens, s)
        w = _sample_weights(weights, s)
        count = rows.count if rows is not None else height
        if out is None:
            import numpy as np

            out = np.zeros((max(count, 0) * width, 3), _fb_dtype(fmt, np.uint8))
        ptr = out if isinstance(out, int) else _addr(out)
        st = rt_radiance_stats()
        _check(self._L.rt_render_lens_samples(self._ctx, C.byref(cam), width, height, depth,
                                              C.byref(rows) if rows is not None else None, off, ln, float(focus), s,
                                              w, fmt, C.c_void_p(ptr), int(out_on_device), C.byref(st)),
               "rt_render_lens_samples", self._ctx, L=self._L)
        return out, st

    def render_lens_samples_async(self, cam: rt_camera, width: int, height: int, depth: int, offsets, lens,
                                  focus: float, out_ptr: int, weights=None, rows: rt_rows | None = None,
                                  fmt: int = RT_FB_RGB8):
        """rt_render_lens_samples_async: render_samples_async through the lens of render_lens_samples,
        enqueued on the context's stream; radiance_stats() afterwards reports it."""
        off, s = _doubles(offsets, 2)
        ln = _lens_points(lens, s)
        w = _sample_weights(weights, s)
        _check(self._L.rt_render_lens_samples_async(self._ctx, C.byref(cam), width, height, depth,
                                                    C.byref(rows) if rows is not None else None, off, ln,
                                                    float(focus), s, w, fmt, C.c_void_p(out_ptr)),
               "rt_render_lens_samples_async", self._ctx, L=self._L)

    def close(self):
        if self._ctx:
            self._L.rt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """A device group (rt_group): one image rendered as len(devices) cyclic row
    shards of `band` rows, one per member, assembled on devices[0].  A device
    may repeat ([0, 0, 0] is three shards on one GPU).  What ray_hip --gpus does
    with RCCL (render_multi, csrc/ray_hip.cpp), as one library call."""

    def __init__(self, devices, band: int = 8, variant: str | None = None):
        """variant: None = the product library; "tuning" / "check" = a test build (VARIANTS)."""
        self._L = variant_lib(variant)
        self.variant = variant
        self._grp = C.c_void_p()
        self.devices = [int(d) for d in devices]
        self.band = band
        arr = (C.c_int * max(1, len(self.devices)))(*self.devices)
        _check(self._L.rt_group_create(arr, len(self.devices), band, C.byref(self._grp)),
               f"rt_group_create({self.devices}, band={band})", L=self._L)

    def _check_grp(self, rc: int, what: str):
        if rc != 0:
            raise RtError(rc, what, self._L.rt_group_last_error(self._grp).decode())

    @property
    def size(self) -> int:
        return self._L.rt_group_size(self._grp)

    def upload(self, scene: Scene):
        self._check_grp(self._L.rt_group_upload_scene(self._grp, C.byref(scene.raw)), "rt_group_upload_scene")
        self._num_lights = scene.num_lights
        self._num_spheres = scene.num_spheres

    def set_gloss_samples(self, roughness, table):
        """rt_group_set_gloss_samples: Renderer.set_gloss_samples on every member."""
        rough, tab, s, b = _gloss_table(roughness, table, getattr(self, "_num_spheres", None))
        self._check_grp(self._L.rt_group_set_gloss_samples(self._grp, rough, tab, s, b), "rt_group_set_gloss_samples")

    def set_light_samples(self, offsets):
        """rt_group_set_light_samples: Renderer.set_light_samples on every member."""
        tab, s = _light_table(offsets, getattr(self, "_num_lights", None))
        self._check_grp(self._L.rt_group_set_light_samples(self._grp, tab, s), "rt_group_set_light_samples")

    def set_antialias(self, samples: int):
        self._check_grp(self._L.rt_group_set_antialias(self._grp, samples), "rt_group_set_antialias")

    def render(self, cam: rt_camera, width: int, height: int, depth: int, out=None,
               out_on_device: bool = False) -> tuple[object, rt_stats]:
        """Render the whole image into `out` (a host bytearray if None; with
        out_on_device a buffer of devices[0]) and return (buffer, stats): the ray
        counts summed over the members, kernel_ms their maximum."""
        if out is None:
            out = bytearray(height * width * 3)
        st = rt_stats()
        self._check_grp(self._L.rt_group_render(self._grp, C.byref(cam), width, height, depth, C.c_void_p(_addr(out)),
                                            int(out_on_device), C.byref(st)), "rt_group_render")
        return out, st

    def render_frames(self, cams, width: int, height: int, depth: int, batch: int = 0, out=None,
                      out_on_device: bool = False, frame_stride: int | None = None) -> tuple[object, rt_stats]:
        """rt_group_render_frames: len(cams) frames (any number), frame f seen through
        cams[f] and sharded as render() shards one, at `out` + f * frame_stride
        (height * width * 3 if None; `out` a host bytearray if None, with
        out_on_device a buffer of devices[0]).  The members render launches of at
        most `batch` frames (0 = MAX_FRAMES) while the previous batch is assembled.
        `cams` may be a ctypes array built beforehand (camera_array).  Returns
        (buffer, stats): the ray counts summed over frames and members, kernel_ms
        the largest member's sum over its launches."""
        n = len(cams)
        image = height * width * 3
        if frame_stride is None:
            frame_stride = image
        if out is None:
            out = bytearray(max(0, n - 1) * frame_stride + image)
        arr = cams if isinstance(cams, C.Array) else camera_array(cams)
        st = rt_stats()
        self._check_grp(self._L.rt_group_render_frames(self._grp, arr, n, width, height, depth, batch,
                                                       C.c_void_p(_addr(out)), int(out_on_device), frame_stride,
                                                       C.byref(st)), "rt_group_render_frames")
        return out, st

    def render_samples(self, cam: rt_camera, width: int, height: int, depth: int, offsets, weights=None,
                       fmt: int = RT_FB_RGB8, out=None, out_on_device: bool = False):
        """rt_group_render_samples: Renderer.render_samples of the full frame, sharded as render()
        shards one.  `out`: None (a host numpy [height * width, 3] array of the format's dtype is
        made), a host buffer, or with out_on_device a buffer / pointer of devices[0].  Returns
        (out, rt_radiance_stats): the counts summed over the members, kernel_ms their maximum."""
        off, s = _doubles(offsets, 2)
        w = _sample_weights(weights, s)
        if out is None:
            import numpy as np

            out = np.zeros((height * width, 3), _fb_dtype(fmt, np.uint8))
        ptr = out if isinstance(out, int) else _addr(out)
        st = rt_radiance_stats()
        self._check_grp(self._L.rt_group_render_samples(self._grp, C.byref(cam), width, height, depth, off, s, w, fmt,
                                                        C.c_void_p(ptr), int(out_on_device), C.byref(st)),
                        "rt_group_render_samples")
        return out, st

    def render_lens_samples(self, cam: rt_camera, width: int, height: int, depth: int, offsets, lens, focus: float,
                            weights=None, fmt: int = RT_FB_RGB8, out=None, out_on_device: bool = False):
        """rt_group_render_lens_samples: Renderer.render_lens_samples of the full frame, sharded as
        render_samples shards one; `out` and the return value as render_samples'."""
        off, s = _doubles(offsets, 2)
        ln = _lens_points(lens, s)
        w = _sample_weights(weights, s)
        if out is None:
            import numpy as np

            out = np.zeros((height * width, 3), _fb_dtype(fmt, np.uint8))
        ptr = out if isinstance(out, int) else _addr(out)
        st = rt_radiance_stats()
        self._check_grp(self._L.rt_group_render_lens_samples(self._grp, C.byref(cam), width, height, depth, off, ln,
                                                             float(focus), s, w, fmt, C.c_void_p(ptr),
                                                             int(out_on_device), C.byref(st)),
                        "rt_group_render_lens_samples")
        return out, st

    def member(self, i: int):
        """The borrowed rt_ctx of member i (rt_group_member)."""
        ctx = self._L.rt_group_member(self._grp, i)
        if not ctx:
            raise IndexError(f"group member {i} of {self.size}")
        return C.c_void_p(ctx)

    def member_stats(self, i: int) -> rt_stats:
        """rt_render_stats of member i: its shard of the most recent render."""
        ctx = self.member(i)
        st = rt_stats()
        _check(self._L.rt_render_stats(ctx, C.byref(st)), f"rt_render_stats(member {i})", ctx, L=self._L)
        return st

    def close(self):
        if self._grp:
            self._L.rt_group_destroy(self._grp)
            self._grp = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_pattern(n: int) -> list[tuple[float, float]]:
    """The n x n sample offsets (a/n, b/n), a fastest: what Renderer.camera_sample_rays and
    render_samples take.  grid_pattern(2) is the antialias pattern (main_gpu.cu:253-256) exactly:
    (0,0) (.5,0) (0,.5) (.5,.5)."""
    if n < 1:
        raise ValueError(f"grid_pattern({n})")
    return [(a / n, b / n) for b in range(n) for a in range(n)]


def lens_pattern(n: int, aperture: float) -> list[tuple[float, float]]:
    """The n x n lens points that go with grid_pattern(n): a lens disk of radius `aperture` (scene
    units).  Sample s takes grid cell n*n-1-s (reversed, so that a sample's pixel offset and its lens
    point are not aligned); the cell is (a, b), a fastest, its centre (u, v) = ((a+.5)/n*2-1,
    (b+.5)/n*2-1) in the square [-1, 1]^2, mapped to the unit disk as (u*sqrt(1 - v*v/2),
    v*sqrt(1 - u*u/2)) and multiplied by `aperture`.  Only correctly rounded operations, in this
    order: ray_hip --aperture computes the same doubles."""
    if n < 1:
        raise ValueError(f"lens_pattern({n})")
    import math

    pts = []
    for s in range(n * n):
        c = n * n - 1 - s
        a, b = c % n, c // n
        u = (a + 0.5) / n * 2.0 - 1.0
        v = (b + 0.5) / n * 2.0 - 1.0
        pts.append((u * math.sqrt(1.0 - v * v / 2.0) * aperture, v * math.sqrt(1.0 - u * u / 2.0) * aperture))
    return pts


def light_pattern(n: int, radius: float, num_lights: int) -> list[list[tuple[float, float, float]]]:
    """The n*n light offsets that go with grid_pattern(n), as set_light_samples takes them: sample s of
    light l is point (s + 17*l) % (n*n) of lens_pattern(n, radius), a disk of radius `radius` (scene
    units), laid in the horizontal plane as (x, 0, z).  The rotation by 17*l decorrelates the lights
    from each other.  ray_hip --light-radius computes the same doubles."""
    if num_lights < 0:
        raise ValueError(f"light_pattern(num_lights={num_lights})")
    disk = lens_pattern(n, radius)
    return [[(disk[(s + 17 * l) % (n * n)][0], 0.0, disk[(s + 17 * l) % (n * n)][1]) for l in range(num_lights)]
            for s in range(n * n)]


def _light_table(offsets, num_lights):
    """(the `light_xyz` argument, samples) of the light-table setters: `offsets` an [S][num_lights][3]
    array-like, or None (the table is cleared).  num_lights: the uploaded scene's, None before an upload
    (the call then reports the missing scene)."""
    if offsets is None:
        return None, 0
    rows = [[tuple(float(x) for x in o) for o in row] for row in offsets]
    nl = num_lights if num_lights is not None else (len(rows[0]) if rows else 0)
    for row in rows:
        if len(row) != nl or any(len(o) != 3 for o in row):
            raise ValueError(f"light offsets are not [samples][{nl}][3]")
    flat = [x for row in rows for o in row for x in o]
    return (C.c_double * max(1, len(flat)))(*flat), len(rows)


def gloss_pattern(n: int, bounces: int) -> list[list[tuple[float, float, float]]]:
    """The n*n x bounces points of the unit ball that go with grid_pattern(n), as set_gloss_samples takes
    them.  For sample s and bounce b: i = (s + 17*(b+1)) % (n*n), (x, y) point i of lens_pattern(n, 1.0),
    h = (2*((7*i + 3) % (n*n)) + 1)/(n*n) - 1 in (-1, 1), z = h*sqrt(max(0, 1 - x*x - y*y)): the disk point
    lifted to a height inside the ball above it.  The rotation by 17*(b+1) decorrelates the bounces from
    each other and from the lens.  Only correctly rounded operations, in this order: ray_hip --gloss
    computes the same doubles."""
    if bounces < 1:
        raise ValueError(f"gloss_pattern(bounces={bounces})")
    import math

    disk = lens_pattern(n, 1.0)
    nn = n * n
    pts = []
    for s in range(nn):
        row = []
        for b in range(bounces):
            i = (s + 17 * (b + 1)) % nn
            x, y = disk[i]
            h = (2 * ((7 * i + 3) % nn) + 1) / nn - 1.0
            row.append((x, y, h * math.sqrt(max(0.0, 1.0 - x * x - y * y))))
        pts.append(row)
    return pts


def scene_roughness(path_or_text: str) -> list[float]:
    """Column 9 ("roughness") of a scene's accepted sphere records, in file order: entry i belongs to sphere i
    of Scene.load / Scene.parse of the same argument (rt_scene_load_roughness / rt_scene_parse_roughness).  A
    string with a newline, or one that names no file, is scene text."""
    L = lib()
    is_text = "\n" in path_or_text or not os.path.exists(path_or_text)
    call, arg = ((L.rt_scene_parse_roughness, path_or_text.encode()) if is_text else
                 (L.rt_scene_load_roughness, os.fsencode(path_or_text)))
    n = C.c_int(0)
    _check(call(arg, None, 0, C.byref(n)), "rt_scene_roughness")  # the sizing call
    out = (C.c_double * max(1, n.value))()
    _check(call(arg, out, n.value, C.byref(n)), "rt_scene_roughness")
    return list(out[:n.value])


def _gloss_table(roughness, table, num_spheres):
    """(roughness, `gloss_xyz`, samples, bounces) of the gloss-table setters: `table` an [S][B][3] array-like
    or None (the table is cleared), `roughness` num_spheres doubles.  num_spheres: the uploaded scene's, None
    before an upload (the call then reports the missing scene)."""
    if table is None:
        return None, None, 0, 0
    rough = [float(x) for x in roughness]
    if num_spheres is not None and len(rough) != num_spheres:
        raise ValueError(f"{len(rough)} roughness values for {num_spheres} spheres")
    rows = [[tuple(float(x) for x in g) for g in row] for row in table]
    nb = len(rows[0]) if rows else 0
    for row in rows:
        if len(row) != nb or any(len(g) != 3 for g in row):
            raise ValueError(f"gloss points are not [samples][{nb}][3]")
    flat = [x for row in rows for g in row for x in g]
    return ((C.c_double * max(1, len(rough)))(*rough), (C.c_double * max(1, len(flat)))(*flat), len(rows), nb)


def _lens_points(lens, samples: int):
    """The `lens_xy` argument of the lens calls: one (lx, ly) pair per sample."""
    ln, n = _doubles(lens, 2)
    if n != samples:
        raise ValueError(f"{n} lens points for {samples} samples")
    return ln


def _doubles(values, width: int):
    """(ctypes double array, records): `values` flattened, `width` doubles per record."""
    flat = []
    for v in values:
        flat.extend(v) if width > 1 else flat.append(v)
    flat = [float(x) for x in flat]
    if len(flat) % width:
        raise ValueError(f"{len(flat)} values are not records of {width}")
    return (C.c_double * max(1, len(flat)))(*flat), len(flat) // width


def _sample_weights(weights, samples: int):
    """The `weights` argument of the resolving calls: None (the box filter) or `samples` doubles."""
    if weights is None:
        return None
    w, n = _doubles(weights, 1)
    if n != samples:
        raise ValueError(f"{n} weights for {samples} samples")
    return w


def _pack_rays(origins, directions, tmax=None):
    """The [n, 8] float64 rt_ray records (origin, direction, tmax, reserved) of Ray(origins[i],
    directions[i]); tmax a scalar or [n], None = 0 (the calls that ignore it)."""
    import numpy as np

    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError(f"{n} origins, {d.shape[0]} directions")
    rays = np.zeros((n, 8), np.float64)
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    if tmax is not None:
        rays[:, 6] = np.broadcast_to(np.asarray(tmax, np.float64), (n,))
    return rays


def _fb_dtype(fmt: int, default):
    """The numpy dtype of a record format's channels; `default` for an unknown one (the call rejects it)."""
    import numpy as np

    return {RT_FB_RGB8: np.uint8, RT_FB_F32X3: np.float32, RT_FB_F64X3: np.float64}.get(fmt, default)


def _addr(buf) -> int:
    if isinstance(buf, bytes):
        return C.cast(C.c_char_p(buf), C.c_void_p).value
    if isinstance(buf, bytearray):
        return C.addressof((C.c_char * len(buf)).from_buffer(buf))
    if hasattr(buf, "ctypes"):  # numpy
        return buf.ctypes.data
    if hasattr(buf, "data_ptr"):  # torch
        return buf.data_ptr()
    raise TypeError(type(buf))


def write_ppm(path: str, rgb, width: int, height: int, binary: bool = False):
    _check(lib().rt_write_ppm(os.fsencode(path), C.c_void_p(_addr(rgb)), width, height, int(binary)), "rt_write_ppm")


def device_count() -> int:
    n = C.c_int(0)
    lib().rt_device_count(C.byref(n))
    return n.value
