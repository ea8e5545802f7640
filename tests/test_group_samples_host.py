"""rt_render_samples_async, rt_group_render_samples and ray_hip --sample-devices: what is decided
before any HIP call, so it holds on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG

import rt_hip

RT_ERR_INVALID_ARG = 1
W, H = 8, 8


@pytest.fixture()
def args():
    """Valid arguments but for the handle: no context or group exists without a GPU."""
    cam = rt_hip.rt_camera()
    off = (C.c_double * 8)()
    out = C.create_string_buffer(W * H * 24)
    return cam, off, C.cast(out, C.c_void_p)


def test_null_group(args):
    cam, off, out = args
    rc = rt_hip.lib().rt_group_render_samples(None, C.byref(cam), W, H, 1, off, 4, None, rt_hip.RT_FB_RGB8, out, 0, None)
    assert rc == RT_ERR_INVALID_ARG


def test_null_context(args):
    cam, off, out = args
    rc = rt_hip.lib().rt_render_samples_async(None, C.byref(cam), W, H, 1, None, off, 4, None, rt_hip.RT_FB_RGB8, out)
    assert rc == RT_ERR_INVALID_ARG


def test_group_arguments_before_the_group_is_read(args):
    """A zeroed block for a group: the argument checks come before anything of it is read; a call that
    got past them would report RT_ERR_NO_SCENE (5) from the zeroed block."""
    cam, off, out = args
    grp = C.cast(C.create_string_buffer(4096), C.c_void_p)
    L = rt_hip.lib()
    fmt = rt_hip.RT_FB_RGB8
    assert L.rt_group_render_samples(grp, None, W, H, 1, off, 4, None, fmt, out, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_render_samples(grp, C.byref(cam), W, H, 1, None, 4, None, fmt, out, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_render_samples(grp, C.byref(cam), W, H, 1, off, 4, None, fmt, None, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_render_samples(grp, C.byref(cam), 0, H, 1, off, 4, None, fmt, out, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_render_samples(grp, C.byref(cam), W, -1, 1, off, 4, None, fmt, out, 0, None) == RT_ERR_INVALID_ARG


def test_python_binding_has_the_new_calls():
    assert "rt_render_samples_async" in rt_hip.SIGNATURES and "rt_group_render_samples" in rt_hip.SIGNATURES
    assert callable(rt_hip.Renderer.render_samples_async) and callable(rt_hip.Group.render_samples)
    assert rt_hip.lib().rt_abi_version() == rt_hip.ABI_VERSION == 12  # new symbols only


def _ray_hip(*args):
    return subprocess.run([os.path.join(PKG, "ray_hip"), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [("--sample-devices", "0,0"),
                                  ("--supersample", "2", "--sample-devices", "0,0", "--devices", "0,0"),
                                  ("--supersample", "2", "--sample-devices", "0,0", "--gpus", "2"),
                                  ("--supersample", "2", "--sample-devices", "0,0", "--gpus", "1"),
                                  ("--supersample", "2", "--sample-devices", "0,0", "-a"),
                                  ("--supersample", "2", "--sample-devices", "0,,0"),
                                  ("--supersample", "2", "--sample-devices", "0,x"),
                                  ("--supersample", "2", "--sample-devices", ""),
                                  ("--supersample", "2", "--sample-devices", "-1"),
                                  ("--supersample", "2", "--sample-devices")],
                         ids=["without_supersample", "with_devices", "with_gpus2", "with_gpus1", "with_a", "empty_item",
                              "not_a_number", "empty_list", "negative", "missing"])
def test_cli_sample_devices_usage_errors(args):
    r = _ray_hip(*args, "scene.txt") if args[-1] != "--sample-devices" else _ray_hip("scene.txt", *args)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "usage" in r.stderr
    assert "Testing scene loader" not in r.stdout  # refused before anything is loaded or rendered


def test_cli_help_mentions_sample_devices():
    r = _ray_hip("--help")
    assert r.returncode == 2 and "--sample-devices" in r.stderr
