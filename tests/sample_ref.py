"""numpy restatement of the multi-sample entries' arithmetic, the checker of the
sample tests (rt_camera_sample_rays, rt_trace_radiance_resolve, rt_render_samples):

  the antialias sample rays   src/main_gpu.cu:253-256 on camera.h:17-25 -> camera_sample_rays
  the sample sum and scale    src/main_gpu.cu:250, 327, 331             -> resolve

Elementwise fp64 in the reference's operand order, as ray_ref.py: numpy neither
contracts nor reassociates, and the loop over the samples is sequential."""
from __future__ import annotations

import numpy as np

import ray_ref

AA_PATTERN = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))  # main_gpu.cu:253-256, rt_hip.grid_pattern(2)


def camera_sample_rays(cam, W, H, offsets, rows=None):
    """The sample rays of output rows `rows` (an rt_rows; None = every row) as [count*W*S, 8]
    rt_ray records, pixel-major with a pixel's samples consecutive: origin, the once-normalised
    direction of camera_dir(x + ox, j + oy) -- the offset added before the division by W-1 and
    H-1 --, tmax = +inf, reserved = 0; padding rows (y >= H) are all zero."""
    band, first, stride, count = (rows.band, rows.first, rows.stride, rows.count) if rows is not None else (1, 0, 1, H)
    off = np.asarray(offsets, np.float64).reshape(-1, 2)
    S = off.shape[0]
    out = np.zeros((count, W, S, 8), np.float64)
    fwd, right, up = (np.array(list(v), np.float64) for v in (cam.forward, cam.right, cam.up))
    xs = np.arange(W, dtype=np.float64)
    for k in range(count):
        y = (k // band) * band * stride + first * band + k % band
        if y >= H:
            continue
        j = H - 1 - y
        for s in range(S):
            with np.errstate(all="ignore"):
                u = (xs + off[s, 0]) / np.float64(W - 1)
                v = (np.float64(j) + off[s, 1]) / np.float64(H - 1)
                su = ((u - 0.5) * cam.scale) * 1.0
                sv = (v - 0.5) * cam.scale
                d = (fwd[None, :] + right[None, :] * su[:, None]) + up[None, :] * sv
            out[k, :, s, 3:6] = ray_ref.normalize(d)
        out[k, :, :, 0:3] = np.array(list(cam.position), np.float64)
        out[k, :, :, 6] = np.inf
    return out.reshape(count * W * S, 8)


def resolve(colours, weights=None):
    """The pixel values [n_pixels, 3] of colours [n_pixels, S, 3]:
      weights None, S == 1: the colour itself (a -0.0 stays -0.0);
      weights None, S > 1:  acc = 0; acc = acc + c_s in order; acc * (1.0 / S);
      weights given:        acc = 0; acc = acc + c_s * w_s in order (the product rounded, then the
                            sum), no final scale."""
    c = np.asarray(colours, np.float64)
    n, S = c.shape[0], c.shape[1]
    if weights is None and S == 1:
        return c[:, 0, :].copy()
    acc = np.zeros((n, 3), np.float64)
    with np.errstate(all="ignore"):
        if weights is None:
            for s in range(S):
                acc = acc + c[:, s, :]
            return acc * (np.float64(1.0) / np.float64(S))
        w = np.asarray(weights, np.float64).reshape(S)
        for s in range(S):
            acc = acc + c[:, s, :] * w[s]
    return acc
