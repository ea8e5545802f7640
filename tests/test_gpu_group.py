"""The device group (rt_group_*, rt_hip.Group, ray_hip --devices) on one GPU:
every member lives on device 0, which runs the code a list of distinct
devices runs (rt_group.hip has one path wherever a member lives).  Bar: the
assembled image is byte-identical to the golden / the CPU oracle, the summed
ray counts are the full frame's, and every member traced exactly its own rows.

Shapes: 97x61 has odd row bytes (291: the byte-copy path) and, at (8,16), four
members whose shards are all padding; 1x1 and 2x2 have H < band; 100x75 has
300-byte rows (4-byte copies), 64x48 192-byte rows (16-byte copies)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, diff_summary, golden_rgb, manifest, scene_path

pytestmark = pytest.mark.gpu

GOLDEN_CASES = [("complex_97x61_d4", G, band) for G, band in
                [(1, 8), (2, 8), (3, 8), (8, 8), (5, 1), (4, 16), (8, 16)]] + [
    ("simple_1x1_d10", 3, 8), ("simple_2x2_d10", 3, 8), ("complex_1920x1080_d4", 8, 8), ("synth10k_384x216_d6", 2, 8)]
ORACLE_CASES = [(100, 75, 2), (64, 48, 3)]  # complex at W x H, depth


@functools.lru_cache(maxsize=None)
def _scene(name):
    import rt_hip

    return rt_hip.Scene.load(scene_path(name))


@functools.lru_cache(maxsize=None)
def _oracle(W, H, depth):
    """complex at W x H from the CPU oracle, computed once: (rgb bytes, counts)."""
    import orc

    rgb, counts, _ = orc.OracleScene(scene_path("complex")).render(W, H, depth, threads=4)
    return rgb, {k: counts[k] for k in ("primary", "shadow", "reflect")}


def _group(G, band=8, scene=None, variant=None):
    import rt_hip

    g = rt_hip.Group([0] * G, band=band, variant=variant)
    assert g.size == G
    if scene is not None:
        g.upload(_scene(scene))
    return g


def _counts(st):
    return {"primary": st.rays_primary, "shadow": st.rays_shadow, "reflect": st.rays_reflect}


def _real_rows(H, band, i, G):
    """Image rows of member i: the rows of the cyclic bands i, i + G, ... (rt_rows)."""
    return sum(1 for y in range(H) if (y // band) % G == i)


def _check_members(g, st, W, H, band, samples=1):
    G = g.size
    members = [g.member_stats(i) for i in range(G)]
    for i, ms in enumerate(members):
        assert ms.rays_primary == W * _real_rows(H, band, i, G) * samples, f"member {i} of {G}"
    assert st.rays_shadow == sum(ms.rays_shadow for ms in members)
    assert st.rays_reflect == sum(ms.rays_reflect for ms in members)
    assert st.kernel_ms == max(ms.kernel_ms for ms in members)
    assert st.negative_clamped == 0


def _render_golden(g, name, band):
    m = manifest()[name]
    rgb, st = g.render(_scene(m["scene"]).camera(), m["width"], m["height"], m["depth"])
    want = golden_rgb(name)
    assert bytes(rgb) == want, f"{name} G={g.size} band={band}: {diff_summary(bytes(rgb), want)}"
    assert _counts(st) == m["rays"]
    _check_members(g, st, m["width"], m["height"], band)


@pytest.mark.parametrize("name,G,band", GOLDEN_CASES, ids=[f"{n}-G{G}-b{b}" for n, G, b in GOLDEN_CASES])
def test_group_matches_golden(name, G, band):
    g = _group(G, band, manifest()[name]["scene"])
    try:
        _render_golden(g, name, band)
    finally:
        g.close()


@pytest.mark.parametrize("W,H,depth", ORACLE_CASES, ids=["100x75-4B", "64x48-16B"])
def test_group_matches_oracle(W, H, depth):
    want, counts = _oracle(W, H, depth)
    g = _group(3, 8, "complex")
    try:
        rgb, st = g.render(_scene("complex").camera(), W, H, depth)
        assert bytes(rgb) == want, diff_summary(bytes(rgb), want)
        assert _counts(st) == counts
        _check_members(g, st, W, H, 8)
    finally:
        g.close()


def _render_into_tensor(g, cam, W, H, depth, off):
    """Renders into device memory `off` bytes into a 0xAA-filled tensor; returns
    (image bytes, every other byte of the tensor)."""
    import torch

    n, lead = H * W * 3, 64
    buf = torch.full((lead + off + n + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # the fill has landed before the group's streams start
    view = buf[lead + off:lead + off + n]
    out, st = g.render(cam, W, H, depth, out=view, out_on_device=True)
    assert out is view
    host = buf.cpu().numpy()
    return host[lead + off:lead + off + n].tobytes(), np.concatenate([host[:lead + off], host[lead + off + n:]]), st


@pytest.mark.parametrize("off", [0, 4])
def test_group_out_on_device(off):
    name = "complex_97x61_d4"
    m = manifest()[name]
    g = _group(3, 8, "complex")
    try:
        got, outside, st = _render_into_tensor(g, _scene("complex").camera(), m["width"], m["height"], m["depth"], off)
        assert got == golden_rgb(name)
        assert (outside == 0xAA).all(), "bytes outside H*W*3 were written"
        assert _counts(st) == m["rays"]
    finally:
        g.close()


@pytest.mark.parametrize("off", [0, 4, 1], ids=["dst16", "dst4", "dst1"])
def test_group_out_on_device_copy_widths(off):
    """64x48 rows are 192 bytes: the destination's alignment alone picks the 16-byte,
    4-byte or byte copies of the placement."""
    W, H, depth = 64, 48, 3
    want, counts = _oracle(W, H, depth)
    g = _group(3, 8, "complex")
    try:
        got, outside, st = _render_into_tensor(g, _scene("complex").camera(), W, H, depth, off)
        assert got == want
        assert (outside == 0xAA).all(), "bytes outside H*W*3 were written"
        assert _counts(st) == counts
    finally:
        g.close()


def test_group_buffers_regrow():
    """One group across image sizes: its shard, staging and image buffers grow
    (97x61 -> 1080p) and are reused when a smaller image follows."""
    g = _group(3, 8)
    try:
        for name in ("complex_97x61_d4", "simple_2x2_d10", "complex_1920x1080_d4", "complex_97x61_d4"):
            g.upload(_scene(manifest()[name]["scene"]))
            _render_golden(g, name, 8)
    finally:
        g.close()


def test_group_antialias():
    import orc

    W, H, depth = 96, 54, 4
    want, counts, _ = orc.OracleScene(scene_path("complex")).render_aa(W, H, depth, samples=4, threads=4)
    g = _group(3, 8, "complex")
    try:
        g.set_antialias(4)
        rgb, st = g.render(_scene("complex").camera(), W, H, depth)
        assert bytes(rgb) == want, diff_summary(bytes(rgb), want)
        assert _counts(st) == {k: counts[k] for k in ("primary", "shadow", "reflect")}
        _check_members(g, st, W, H, 8, samples=4)
    finally:
        g.close()


def test_group_scene_reupload():
    g = _group(3, 8, "complex")
    try:
        _render_golden(g, "complex_97x61_d4", 8)
        g.upload(_scene("simple"))
        _render_golden(g, "simple_800x600_d10", 8)
    finally:
        g.close()


def test_group_check_build():
    """The bounds-checked build: three contexts on one device share its g_check
    record; a clean render leaves it empty for every member."""
    g = _group(3, 8, "complex", variant="check")
    try:
        _render_golden(g, "complex_97x61_d4", 8)
    finally:
        g.close()


def test_group_render_errors():
    import rt_hip

    cam = _scene("complex").camera()
    g = _group(2, 8)
    try:
        with pytest.raises(rt_hip.RtError) as e:
            g.render(cam, 16, 16, 2)
        assert e.value.status == 5  # RT_ERR_NO_SCENE
        g.upload(_scene("complex"))
        with pytest.raises(rt_hip.RtError) as e:
            g.render(cam, 16, 16, rt_hip.RT_MAX_DEPTH + 1)
        assert e.value.status == 7  # RT_ERR_DEPTH
        with pytest.raises(rt_hip.RtError) as e:
            g.render(cam, 0, 16, 2)
        assert e.value.status == 1
        with pytest.raises(IndexError):
            g.member_stats(2)
        _render_golden(g, "complex_97x61_d4", 8)  # the group is still usable
    finally:
        g.close()


def test_group_create_fails_on_an_absent_device():
    """The second member cannot be created: the first is destroyed again, no handle is returned."""
    import torch
    import rt_hip

    with pytest.raises(rt_hip.RtError) as e:
        rt_hip.Group([0, torch.cuda.device_count()])
    assert e.value.status == 1
    # and the failure leaves no HIP error behind for the thread's next launch to trip over
    g = _group(2, 8, "complex")
    try:
        _render_golden(g, "complex_97x61_d4", 8)
    finally:
        g.close()


def _cli(tmp_path, *args):
    r = subprocess.run([os.path.join(PKG, "ray_hip"), "--devices", "0,0,0", "--width", "1920", "--height", "1080",
                        "--depth", "4", "--p6", *args, scene_path("complex")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(tmp_path / "output_gpu.ppm", "rb").read()
    head = b"P6\n1920 1080\n255\n"
    assert data.startswith(head) and data[len(head):] == golden_rgb("complex_1920x1080_d4")
    assert "GPU rendering time:" in r.stdout
    return r.stdout


def test_cli_devices(tmp_path):
    _cli(tmp_path)


def test_cli_devices_json(tmp_path):
    out = _cli(tmp_path, "--json")
    rec = json.loads(next(line for line in out.splitlines() if line.startswith("{")))
    rays = manifest()["complex_1920x1080_d4"]["rays"]
    assert rec["gpus"] == 3
    assert {k: rec[k] for k in ("primary", "shadow", "reflect")} == rays
    assert rec["rays"] == sum(rays.values())
