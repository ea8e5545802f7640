"""rt_group_render_frames and ray_hip --frames: what is decided before any HIP
call, so it holds on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG

import rt_hip

RT_ERR_INVALID_ARG = 1
W, H = 8, 8


def _call(grp, cams, nframes, batch, out, stride=W * H * 3):
    return rt_hip.lib().rt_group_render_frames(grp, cams, nframes, W, H, 1, batch, out, 0, stride, None)


@pytest.fixture()
def args():
    """Valid arguments but for the group: no group exists without a GPU, so the
    handle is a zeroed block.  The argument checks come before anything of the
    group is read; a call that got past them would report RT_ERR_NO_SCENE (5)
    from the zeroed block, not RT_ERR_INVALID_ARG."""
    fake = C.create_string_buffer(4096)
    cams = rt_hip.camera_array([rt_hip.rt_camera()] * 4)
    out = C.create_string_buffer(4 * W * H * 3)
    return C.cast(fake, C.c_void_p), cams, C.cast(out, C.c_void_p)


def test_null_group(args):
    _, cams, out = args
    assert _call(None, cams, 4, 2, out) == RT_ERR_INVALID_ARG


@pytest.mark.parametrize("nframes", [0, -1])
def test_nframes_below_one(args, nframes):
    grp, cams, out = args
    assert _call(grp, cams, nframes, 2, out) == RT_ERR_INVALID_ARG


@pytest.mark.parametrize("batch", [-1, rt_hip.MAX_FRAMES + 1])
def test_batch_out_of_range(args, batch):
    assert rt_hip.MAX_FRAMES == 32
    grp, cams, out = args
    assert _call(grp, cams, 4, batch, out) == RT_ERR_INVALID_ARG


def test_null_cams(args):
    grp, _, out = args
    assert _call(grp, None, 4, 2, out) == RT_ERR_INVALID_ARG


def test_null_output(args):
    grp, cams, _ = args
    assert _call(grp, cams, 4, 2, None) == RT_ERR_INVALID_ARG


def test_bad_image_size_and_short_stride(args):
    grp, cams, out = args
    L = rt_hip.lib()
    assert L.rt_group_render_frames(grp, cams, 4, 0, H, 1, 2, out, 0, W * H * 3, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_render_frames(grp, cams, 4, W, -1, 1, 2, out, 0, W * H * 3, None) == RT_ERR_INVALID_ARG
    assert _call(grp, cams, 2, 2, out, stride=W * H * 3 - 1) == RT_ERR_INVALID_ARG


def test_python_binding_has_render_frames():
    assert "rt_group_render_frames" in rt_hip.SIGNATURES
    assert callable(rt_hip.Group.render_frames)


def _ray_hip(*args):
    return subprocess.run([os.path.join(PKG, "ray_hip"), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [("--frames", "3"), ("--devices", "0,0", "--frames", "0"),
                                  ("--devices", "0,0", "--frames", "3", "--batch", "40"),
                                  ("--devices", "0,0", "--batch", "2"), ("--devices", "0,0", "--frames"),
                                  ("--devices", "0,0", "--frames", "3", "--batch", "-1")],
                         ids=["frames_without_devices", "frames0", "batch40", "batch_without_frames", "missing",
                              "batch_negative"])
def test_cli_frames_usage_errors(args):
    r = _ray_hip(*args, "scene.txt")
    assert r.returncode == 2, r.stdout + r.stderr
    assert "usage" in r.stderr
    assert "Testing scene loader" not in r.stdout  # refused before anything is loaded or rendered


def test_cli_help_mentions_frames():
    r = _ray_hip("--help")
    assert r.returncode == 2 and "--frames" in r.stderr and "--batch" in r.stderr
