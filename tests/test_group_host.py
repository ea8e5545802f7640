"""The device group's host side (rt_group_*, ray_hip --devices): what is decided
before any HIP call, so it holds on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG

import rt_hip

RT_ERR_INVALID_ARG = 1


@pytest.mark.parametrize("devices,n,band", [((0,), 0, 8), ((0,), -1, 8), (None, 1, 8), ((0,), 1, 0), ((0, 0), 2, -3)],
                         ids=["n0", "n_negative", "null_devices", "band0", "band_negative"])
def test_group_create_rejects_bad_arguments(devices, n, band):
    L = rt_hip.lib()
    arr = (C.c_int * len(devices))(*devices) if devices is not None else None
    out = C.c_void_p(0xDEAD)  # overwritten: a failed create leaves NULL, never a stale handle
    assert L.rt_group_create(arr, n, band, C.byref(out)) == RT_ERR_INVALID_ARG
    assert not out.value


def test_group_create_null_out():
    assert rt_hip.lib().rt_group_create((C.c_int * 1)(0), 1, 8, None) == RT_ERR_INVALID_ARG


def test_group_null_handle_is_harmless():
    L = rt_hip.lib()
    assert L.rt_group_size(None) == 0
    L.rt_group_destroy(None)
    assert L.rt_group_member(None, 0) is None
    assert L.rt_group_last_error(None)  # a message, not a crash
    assert L.rt_group_upload_scene(None, None) == RT_ERR_INVALID_ARG
    assert L.rt_group_set_antialias(None, 4) == RT_ERR_INVALID_ARG
    assert L.rt_group_render(None, None, 8, 8, 1, None, 0, None) == RT_ERR_INVALID_ARG


def test_python_group_rejects_an_empty_device_list():
    with pytest.raises(rt_hip.RtError) as e:
        rt_hip.Group([])
    assert e.value.status == RT_ERR_INVALID_ARG


def _ray_hip(*args):
    return subprocess.run([os.path.join(PKG, "ray_hip"), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [("--devices", "0,x"), ("--devices", ""), ("--devices", "0,"), ("--devices", "-1"),
                                  ("--devices",), ("--devices", "0", "--gpus", "2"),
                                  ("--gpus", "2", "--devices", "0,0"), ("--devices", "0", "--force-gather")],
                         ids=["not_a_number", "empty", "trailing_comma", "negative", "missing", "with_gpus",
                              "gpus_first", "with_force_gather"])
def test_cli_devices_usage_errors(args):
    r = _ray_hip(*args, "scene.txt")
    assert r.returncode == 2, r.stdout + r.stderr
    assert "usage" in r.stderr
    assert "Testing scene loader" not in r.stdout  # refused before anything is loaded or rendered


def test_cli_help_mentions_devices():
    r = _ray_hip("--help")
    assert r.returncode == 2 and "--devices" in r.stderr
