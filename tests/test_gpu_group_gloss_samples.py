"""GPU: rt_group_set_gloss_samples (include/rt_hip.h, rt_hip.Group.set_gloss_samples) on one GPU: every
member lives on device 0, which runs the code a list of distinct devices runs.  Bar: with a gloss table on
every member the two group sample renders assemble, byte for byte, the frame the single-context calls
write under the same table (which test_gpu_gloss_samples.py holds against the level-by-level chain), and
the summed counts are the full frame's.

37 x 21 and three members: H is no multiple of the band, the last shard has padding rows."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_gloss_samples import MEDIUM_FOCUS, MIXED, fixture
from test_gpu_group_samples import F32X3, F64X3, RGB8, _weights, counts
from test_gpu_samples import same_bits

pytestmark = pytest.mark.gpu

W, H, D, N, B = 37, 21, 4, 3, 2
INVALID = 1


def _patterns():
    import rt_hip

    return rt_hip.grid_pattern(N), rt_hip.lens_pattern(N, 0.05), rt_hip.gloss_pattern(N, B)


def _group():
    import rt_hip

    g = rt_hip.Group([0, 0, 0], band=8)
    g.upload(fixture(MIXED, 2.5)[0])
    return g


@functools.lru_cache(maxsize=None)
def _one_context(form, table_on, weighted, fmt):
    """The single-context synchronous call of the full frame, with or without the table, once."""
    import rt_hip

    pattern, lens, table = _patterns()
    sc, _, rough = fixture(MIXED, 2.5)
    w = _weights(N * N) if weighted else None
    r = rt_hip.Renderer(0)
    try:
        r.upload(sc)
        if table_on:
            r.set_gloss_samples(rough, table)
        if form == "lens":
            rec, st = r.render_lens_samples(sc.camera(), W, H, D, pattern, lens, MEDIUM_FOCUS, w, None, fmt)
        else:
            rec, st = r.render_samples(sc.camera(), W, H, D, pattern, w, None, fmt)
    finally:
        r.close()
    rec.setflags(write=False)
    return rec, counts(st)


def _check(g, form, table_on, weighted, fmt):
    pattern, lens, _ = _patterns()
    w = _weights(N * N) if weighted else None
    cam = fixture(MIXED, 2.5)[0].camera()
    want, cnt = _one_context(form, table_on, weighted, fmt)
    if form == "lens":
        got, st = g.render_lens_samples(cam, W, H, D, pattern, lens, MEDIUM_FOCUS, w, fmt)
    else:
        got, st = g.render_samples(cam, W, H, D, pattern, w, fmt)
    assert got.dtype == want.dtype and got.shape == want.shape
    same = np.array_equal(got, want) if fmt == RGB8 else bool(same_bits(got, want).all())
    assert same, (form, table_on, fmt)
    assert counts(st) == cnt and st.rays == N * N * W * H
    return got


@pytest.mark.parametrize("fmt", [RGB8, F32X3, F64X3])
def test_group_matches_one_context_under_the_table(fmt):
    g = _group()
    try:
        g.set_gloss_samples(fixture(MIXED, 2.5)[2], _patterns()[2])
        for form in ("pinhole", "lens"):
            soft = _check(g, form, True, fmt == F32X3, fmt)
            assert soft.tobytes() != _one_context(form, False, fmt == F32X3, fmt)[0].tobytes()  # the table is read
    finally:
        g.close()


def test_upload_clears_the_table_and_a_mismatch_names_the_counts():
    import rt_hip

    sc, _, rough = fixture(MIXED, 2.5)
    g = _group()
    try:
        g.set_gloss_samples(rough, _patterns()[2])
        _check(g, "pinhole", True, False, RGB8)
        # nine samples in the table, four in the call
        off = (C.c_double * 8)()
        host = np.zeros((W * H, 3), np.float64)
        st = rt_hip.rt_radiance_stats()
        rc = g._L.rt_group_render_samples(g._grp, C.byref(sc.camera()), W, H, D, off, 4, None, F64X3,
                                          C.c_void_p(host.ctypes.data), 0, C.byref(st))
        err = g._L.rt_group_last_error(g._grp).decode()
        assert rc == INVALID and "rt_group_render_samples" in err and "gloss table" in err, err
        assert "(4)" in err and "(9," in err, err
        assert (host == 0).all()
        # cleared by hand, set again, then cleared by rt_group_upload_scene on every member
        g.set_gloss_samples(None, None)
        _check(g, "pinhole", False, False, RGB8)
        g.set_gloss_samples(rough, _patterns()[2])
        g.upload(sc)
        _check(g, "pinhole", False, False, RGB8)
        _check(g, "lens", False, True, F64X3)
        got, _ = g.render_samples(sc.camera(), W, H, D, rt_hip.grid_pattern(2))  # any count again
        assert got.shape == (W * H, 3)
    finally:
        g.close()
