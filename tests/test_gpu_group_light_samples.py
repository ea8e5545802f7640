"""GPU: rt_group_set_light_samples (include/rt_hip.h, rt_hip.Group.set_light_samples) on one GPU: every
member lives on device 0, which runs the code a list of distinct devices runs.  Bar: with a light table on
every member the two group sample renders assemble, byte for byte, the frame the single-context calls
write under the same table (which test_gpu_light_samples.py holds against the shifted scenes), and the
summed counts are the full frame's.

37 x 21 and three members: H is no multiple of the band, the last shard has padding rows, and the rows
are 111 bytes in RGB8, 444 in F32X3 (the placement's 4-byte copies) and 888 in F64X3."""
import functools

import numpy as np
import pytest

from conftest import golden_rgb, manifest
from test_gpu_group_samples import AA, F32X3, F64X3, RGB8, _group, _scene, _weights, counts
from test_gpu_samples import same_bits

pytestmark = pytest.mark.gpu

W, H, D, N = 37, 21, 4, 3
FOCUS, APERTURE, RADIUS = 7.25, 0.3, 0.5


def _patterns():
    import rt_hip

    return (rt_hip.grid_pattern(N), rt_hip.lens_pattern(N, APERTURE),
            rt_hip.light_pattern(N, RADIUS, _scene("complex").num_lights))


@functools.lru_cache(maxsize=None)
def _one_context(form, table_on, weighted, fmt):
    """The single-context synchronous call of the full frame, with or without the table, once."""
    import rt_hip

    pattern, lens, table = _patterns()
    w = _weights(N * N) if weighted else None
    r = rt_hip.Renderer(0)
    try:
        r.upload(_scene("complex"))
        if table_on:
            r.set_light_samples(table)
        cam = _scene("complex").camera()
        if form == "lens":
            rec, st = r.render_lens_samples(cam, W, H, D, pattern, lens, FOCUS, w, None, fmt)
        else:
            rec, st = r.render_samples(cam, W, H, D, pattern, w, None, fmt)
    finally:
        r.close()
    rec.setflags(write=False)
    return rec, counts(st)


def _check(g, form, table_on, weighted, fmt):
    pattern, lens, _ = _patterns()
    w = _weights(N * N) if weighted else None
    cam = _scene("complex").camera()
    want, cnt = _one_context(form, table_on, weighted, fmt)
    if form == "lens":
        got, st = g.render_lens_samples(cam, W, H, D, pattern, lens, FOCUS, w, fmt)
    else:
        got, st = g.render_samples(cam, W, H, D, pattern, w, fmt)
    assert got.dtype == want.dtype and got.shape == want.shape
    same = np.array_equal(got, want) if fmt == RGB8 else bool(same_bits(got, want).all())
    assert same, (form, table_on, fmt)
    assert counts(st) == cnt and st.rays == N * N * W * H
    return got


@pytest.mark.parametrize("fmt", [RGB8, F32X3, F64X3])
def test_group_matches_one_context_under_the_table(fmt):
    g = _group(3, 8, "complex")
    try:
        g.set_light_samples(_patterns()[2])
        for form in ("pinhole", "lens"):
            soft = _check(g, form, True, fmt == F32X3, fmt)
            assert soft.tobytes() != _one_context(form, False, fmt == F32X3, fmt)[0].tobytes()  # the table is read
    finally:
        g.close()


def test_the_group_calls_in_any_order_and_with_the_table_cleared():
    """The group render calls share the buffers and events of slot 0: frames, samples, lens samples under
    the table, then again with the table cleared, and once more after an upload cleared it."""
    m = manifest()[AA]
    cam = _scene("complex").camera()
    g = _group(3, 8, "complex")
    try:
        g.set_light_samples(_patterns()[2])
        for table_on in (True, False, True, False):
            frames, _ = g.render_frames([cam] * 2, m["width"], m["height"], m["depth"], batch=1)
            n = m["width"] * m["height"] * 3
            assert all(bytes(frames[f * n:(f + 1) * n]) == golden_rgb(AA) for f in range(2))  # no table is read
            _check(g, "pinhole", table_on, False, RGB8)
            _check(g, "lens", table_on, True, F64X3)
            rgb, _ = g.render(cam, m["width"], m["height"], m["depth"])
            assert bytes(rgb) == golden_rgb(AA)
            _check(g, "pinhole", table_on, True, F32X3)
            if table_on:
                g.set_light_samples(None)
            else:
                g.set_light_samples(_patterns()[2])
        # rt_group_upload_scene clears the table on every member
        g.upload(_scene("complex"))
        _check(g, "pinhole", False, False, RGB8)
        _check(g, "lens", False, False, RGB8)
    finally:
        g.close()
