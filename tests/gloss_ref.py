"""The yardstick of the gloss table's tests (include/rt_hip.h, "samples with glossy reflections"): a
sample's chain run level by level with calls that exist without the feature, the reflection ray bent on the
host in between -- numpy fp64, elementwise, in the operand order of rt_device.h's mk / add / scale / dot,
as path_ref.py and ray_ref.py restate the reference (numpy neither contracts nor reassociates).

  bend          the rule itself: rd, rp, the `use` test, the direction handed to the next level
  host_chain    the chain's geometry on the CPU alone (path_ref's closest hit): which hits spawn, which
                are bent, which perturbations are refused -- what the tests assert their fixtures contain
  device_chain  the yardstick: per level one rt_trace_paths (depth 1, surfaces) for the sphere, the stored
                direction, the hit point and the normal, one rt_trace_radiance (depth 1, RT_FB_F64X3) for
                the level's colour -- the sky, the shade, or A = shade*(1 - refl), which is what a launch
                writes for a reflective hit with no depth left --, then bend, and the composite innermost
                first, res = A + res*refl (trace_wave's unwind)
"""
from __future__ import annotations

import numpy as np

import path_ref
import ray_ref

EPSILON = path_ref.EPSILON


def bend(d, nrm, rough, points, k):
    """The reflection rays of one level.  d, nrm [n,3]: the level's stored direction and normal; rough [n]:
    the roughness of the sphere each ray leaves; points: the sample's [bounces, 3] table rows, or None
    (no table); k: the level.  Returns (chosen [n,3], use [n] bool): the unnormalised direction of the
    next level's ray -- the query normalises it once -- and where that is the perturbed one."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        rd = d - (nrm * 2.0) * path_ref.dot(d, nrm)[:, None]  # main.cpp:45: today's mirror direction
        use = np.zeros(d.shape[0], bool)
        if points is None or k >= len(points):
            return rd, use  # no table, or a bounce beyond it: a mirror, and the table is not read
        g = np.asarray(points[k], np.float64).reshape(1, 3)
        r = np.asarray(rough, np.float64).reshape(-1)
        rp = rd + g * r[:, None]  # the product rounded, then the sum
        use = (r != 0.0) & (path_ref.dot(rp, nrm) * path_ref.dot(rd, nrm) > 0.0)
    return np.where(use[:, None], rp, rd), use


def host_chain(o, d, depth, sa, rough, points):
    """The geometry of trace_ray's chain under the gloss rule, on the CPU: a list of levels, each a dict
    over the n rays of `traced`, `sphere`, `spawn` (a reflection ray left), `glossy` (it left a sphere of
    roughness != 0 at a level inside the table) and `use` (it was bent; glossy & ~use: refused)."""
    rough = np.asarray(rough, np.float64)
    org = np.array(np.asarray(o, np.float64).reshape(-1, 3))
    dirs = ray_ref.normalize(d)
    n = org.shape[0]
    alive = np.ones(n, bool)
    levels = []
    for k in range(depth):
        lv = {"traced": alive.copy(), "sphere": np.full(n, -1, np.int32), "spawn": np.zeros(n, bool),
              "glossy": np.zeros(n, bool), "use": np.zeros(n, bool)}
        idx = np.flatnonzero(alive)
        nxt = np.zeros(n, bool)
        if idx.size:
            with np.errstate(all="ignore"):
                t, s = path_ref._closest_stored(org[idx], dirs[idx], sa)
                lv["sphere"][idx] = s
                h = np.flatnonzero((s >= 0) & (sa.refl[np.maximum(s, 0)] > 0) & (depth - (k + 1) >= 1))
                hi, sph = idx[h], s[h]
                hit = org[hi] + dirs[hi] * t[h, None]
                nrm = ray_ref.normalize(hit - sa.centers[sph])
                chosen, use = bend(dirs[hi], nrm, rough[sph], points, k)
                org[hi] = hit + nrm * EPSILON
                dirs[hi] = ray_ref.normalize(chosen)
                lv["spawn"][hi] = True
                lv["glossy"][hi] = (rough[sph] != 0.0) & (points is not None and k < len(points))
                lv["use"][hi] = use
                nxt[hi] = True
        alive = nxt
        levels.append(lv)
    return levels


def coverage(levels):
    """(reflective hits that spawn off a sphere of roughness != 0 inside the table, of them refused,
    spawning hits on a sphere of roughness 0 or beyond the table) of host_chain's levels."""
    glossy = sum(int(lv["glossy"].sum()) for lv in levels)
    refused = sum(int((lv["glossy"] & ~lv["use"]).sum()) for lv in levels)
    mirror = sum(int((lv["spawn"] & ~lv["glossy"]).sum()) for lv in levels)
    return glossy, refused, mirror


def device_chain(paths, radiance, sa, rough, points, o, d, depth):
    """The yardstick for one sample's rays (o, d [n,3], d as the ray records hold it).  paths, radiance:
    the contexts rt_trace_paths and rt_trace_radiance run on (the same one, or for a sample under a light
    table a second one that holds this sample's moved lights: the geometry is the same).  Returns (colours
    [n,3] fp64, {rays, segments, hits, shadow_rays}, and two [n] bool arrays: `glossy`, the chain spawned a
    reflection ray off a sphere of roughness != 0 at a level inside the table, and `bent`, one was bent)."""
    rough = np.asarray(rough, np.float64)
    o = np.array(np.asarray(o, np.float64).reshape(-1, 3))  # copies: the levels overwrite them
    d = np.array(np.asarray(d, np.float64).reshape(-1, 3))
    n = o.shape[0]
    cnt = {"rays": n, "segments": 0, "hits": 0, "shadow_rays": 0}
    bent, glossy = np.zeros(n, bool), np.zeros(n, bool)
    idx = np.arange(n)
    stack = []  # per level: (the rays' indices, their colour or A, refl where a ray went on, else NaN)
    for k in range(depth):
        if idx.size == 0:
            break
        verts, surf, _ = paths.trace_paths(o[idx], d[idx], 1, surfaces=True)
        col, st = radiance.trace_radiance(o[idx], d[idx], 1)
        for key in ("segments", "hits", "shadow_rays"):
            cnt[key] += getattr(st, key)
        sphere = verts[0]["sphere"]
        refl = np.where(sphere >= 0, sa.refl[np.maximum(sphere, 0)], 0.0)
        spawn = (sphere >= 0) & (refl > 0) & (depth - (k + 1) >= 1)  # main.cpp:43, :17: unchanged
        stack.append((idx, col, np.where(spawn, refl, np.nan)))
        sp = np.flatnonzero(spawn)
        nrm = surf[0]["normal"][sp]
        chosen, use = bend(surf[0]["dir"][sp], nrm, rough[sphere[sp]], points, k)
        bent[idx[sp]] |= use
        if points is not None and k < len(points):
            glossy[idx[sp]] |= rough[sphere[sp]] != 0.0
        with np.errstate(all="ignore"):
            o[idx[sp]] = surf[0]["hit"][sp] + nrm * EPSILON  # main.cpp:48
        d[idx[sp]] = chosen
        idx = idx[sp]
    res = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for ids, col, refl in reversed(stack):  # innermost first
            went_on = ~np.isnan(refl)
            res[ids] = np.where(went_on[:, None], col + res[ids] * np.where(went_on, refl, 0.0)[:, None], col)
    return res, cnt, {"glossy": glossy, "bent": bent}
