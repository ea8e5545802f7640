"""numpy restatement of the thin-lens ray formation, the checker of the lens tests
(rt_camera_lens_rays, rt_render_lens_samples[_async], rt_group_render_lens_samples):

  dir0 = camera_dir(cam, x + ox_s, j + oy_s, W, H)     camera.h:17-25, unnormalised, forward component 1
  lv   = right * lx_s + up * ly_s
  o    = position + lv
  dir  = normalized(dir0 * focus - lv)

Elementwise fp64 in that operand order, as sample_ref.py: numpy neither contracts nor
reassociates."""
from __future__ import annotations

import numpy as np

import ray_ref


def camera_dir(cam, W, H, j, ox, oy):
    """camera_dir of row j's W pixels at the offset (ox, oy): [W, 3], unnormalised."""
    fwd, right, up = (np.array(list(v), np.float64) for v in (cam.forward, cam.right, cam.up))
    xs = np.arange(W, dtype=np.float64)
    with np.errstate(all="ignore"):
        u = (xs + np.float64(ox)) / np.float64(W - 1)
        v = (np.float64(j) + np.float64(oy)) / np.float64(H - 1)
        su = ((u - 0.5) * cam.scale) * 1.0
        sv = (v - 0.5) * cam.scale
        return (fwd[None, :] + right[None, :] * su[:, None]) + up[None, :] * sv


def lens_ray(cam, dir0, lx, ly, focus):
    """(origin [3], direction [n, 3]) of the rays through dir0 [n, 3] from the lens point (lx, ly)."""
    pos, right, up = (np.array(list(v), np.float64) for v in (cam.position, cam.right, cam.up))
    with np.errstate(all="ignore"):
        lv = right * np.float64(lx) + up * np.float64(ly)
        o = pos + lv
        d = ray_ref.normalize(dir0 * np.float64(focus) - lv[None, :])
    return o, d


def camera_lens_rays(cam, W, H, offsets, lens, focus, rows=None):
    """The lens rays of output rows `rows` (an rt_rows; None = every row) as [count*W*S, 8] rt_ray
    records in sample_ref.camera_sample_rays' layout: sample s pairs offsets[s] with lens[s];
    tmax = +inf, reserved = 0; padding rows (y >= H) are all zero."""
    band, first, stride, count = (rows.band, rows.first, rows.stride, rows.count) if rows is not None else (1, 0, 1, H)
    off = np.asarray(offsets, np.float64).reshape(-1, 2)
    ln = np.asarray(lens, np.float64).reshape(-1, 2)
    S = off.shape[0]
    if ln.shape[0] != S:
        raise ValueError("%d lens points for %d offsets" % (ln.shape[0], S))
    out = np.zeros((count, W, S, 8), np.float64)
    for k in range(count):
        y = (k // band) * band * stride + first * band + k % band
        if y >= H:
            continue
        j = H - 1 - y
        for s in range(S):
            o, d = lens_ray(cam, camera_dir(cam, W, H, j, off[s, 0], off[s, 1]), ln[s, 0], ln[s, 1], focus)
            out[k, :, s, 0:3] = o
            out[k, :, s, 3:6] = d
        out[k, :, :, 6] = np.inf
    return out.reshape(count * W * S, 8)
