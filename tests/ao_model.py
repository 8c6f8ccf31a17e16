"""The expectation side of the ambient occlusion tests, independent of the pass's kernel: the
contract of yrt_render_ao (include/yrt.h) restated in NumPy at one sample per pixel, every
intermediate held in float32, over the library's existing position, normal and ids AOV planes
(at one sample they hold eval_pos / eval_norm of the hit exactly), the oracle's camera rays, the
shapes' kinds and the two tables; every occlusion ray is answered by the CPU oracle's
intersect_any."""
import ctypes as C

import numpy as np

from helpers import Oracle, oracle_lib

FLT_MAX = np.float32(3.4028234663852886e38)
F1 = np.float32(1.0)

_geometry = {}


def camera_dirs(path, res, width, s=1):
    """the camera rays' directions from oracle_camera_ray, (s, s, H, W, 3) float32 indexed [jj, ii, j, i]"""
    orc, lib = Oracle(path), oracle_lib()
    W, H = orc.image_size(res)
    W = width or W
    d = np.zeros((s, s, H, W, 3), np.float32)
    ray8 = (C.c_float * 8)()
    for jj in range(s):
        for ii in range(s):
            for j in range(H):
                for i in range(W):
                    assert lib.oracle_camera_ray(orc.h, 0, res, width, s, i, j, ii, jj, ray8) == 0
                    d[jj, ii, j, i] = ray8[3:6]
    return d


def geometry(yrt, scene, path, res, width, key):
    """the one-sample frame's hit points, normals, shape ids and camera directions, made once per frame"""
    k = (key, res, width)
    if k not in _geometry:
        aov = yrt.render_aovs(scene, res, 1, width=width, aovs=("position", "normal", "ids"))
        _geometry[k] = dict(pos=aov["position"][..., :3].copy(), nrm=aov["normal"][..., :3].copy(),
                            hit=aov["position"][..., 3] == 1, shape=aov["ids"][..., 3].copy(),
                            d=camera_dirs(path, res, width)[0, 0])
        for a in _geometry[k].values():
            a.setflags(write=False)
    return _geometry[k]


def default_rotation(H, W):
    """step 3 at one sample per pixel: r = (i & 3) | (j & 3) << 2"""
    j, i = np.mgrid[0:H, 0:W]
    return ((i & 3) | (j & 3) << 2).astype(np.int64)


def dot32(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + a[..., 2] * b[..., 2]).astype(np.float32)


def occlusion_rays(p, n, d, r, dirs, rots, K, bias, distance):
    """steps 1 to 4 for N hits: p, n, d (N, 3) float32, r (N,) -> rays (N, K, 8) float32 and the
    (N,) mask of the hits whose normal the face-forward test flipped"""
    p, n, d = (np.asarray(a, np.float32) for a in (p, n, d))
    flip = dot32(n, d) > np.float32(0)  # false on NaN
    n = np.where(flip[:, None], -n, n).astype(np.float32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sg = np.where(nz >= np.float32(0), F1, -F1).astype(np.float32)
    a = (-F1 / (sg + nz).astype(np.float32)).astype(np.float32)
    b = ((nx * ny).astype(np.float32) * a).astype(np.float32)
    b1 = np.stack([(F1 + (((sg * nx).astype(np.float32) * nx).astype(np.float32) * a).astype(np.float32)),
                   sg * b, (-sg) * nx], 1).astype(np.float32)
    b2 = np.stack([b, sg + ((ny * ny).astype(np.float32) * a).astype(np.float32), -ny], 1).astype(np.float32)
    c, sn = rots[r, 0].astype(np.float32), rots[r, 1].astype(np.float32)
    rays = np.zeros((len(p), K, 8), np.float32)
    for k in range(K):
        tx, ty, tz = (np.float32(v) for v in dirs[k])
        x = ((c * tx).astype(np.float32) - (sn * ty).astype(np.float32)).astype(np.float32)
        y = ((sn * tx).astype(np.float32) + (c * ty).astype(np.float32)).astype(np.float32)
        t = ((b1 * x[:, None]).astype(np.float32) + (b2 * y[:, None]).astype(np.float32)).astype(np.float32)
        rays[:, k, 0:3] = p
        rays[:, k, 3:6] = (t + (n * tz).astype(np.float32)).astype(np.float32)
    rays[:, :, 6] = np.float32(bias)
    rays[:, :, 7] = min(np.float32(distance), FLT_MAX)
    assert rays.dtype == np.float32
    return rays, flip


def ao_model(yrt, scene, host_scene, path, res, width, K, distance, bias, r=None, key=None):
    """What yrt_render_ao must give at one sample per pixel: {"plane" (H, W, 4) float32, "count"
    (H, W) the unoccluded rays, "hit", "tri", "flip" (H, W) bool, "kind" (H, W) int (-1 on a miss)}.
    `scene` is what render_aovs takes, `host_scene` the Scene (its shape_kinds), `path` the
    scene's file for the oracle. `r` (H, W) replaces the rotation index of step 3."""
    g = geometry(yrt, scene, path, res, width, key or str(path))
    dirs, rots = yrt.ao_tables()
    hit = g["hit"]
    H, W = hit.shape
    kinds = np.asarray(host_scene.shape_kinds(), np.int64)
    kind = np.where(hit, kinds[np.where(hit, g["shape"], 0)], -1)
    tri = hit & (kind == 0)
    r = default_rotation(H, W) if r is None else np.asarray(r, np.int64)
    assert r.shape == (H, W) and r.min() >= 0 and r.max() < 16
    rays, flipped = occlusion_rays(g["pos"][tri], g["nrm"][tri], g["d"][tri], r[tri], dirs, rots, K, bias, distance)
    # the precondition of comparing bits: apart from the sign choice sg, the sign of a zero could
    # only matter in a direction with a zero component (the AOV planes launder -0 to +0)
    assert np.isfinite(rays[:, :, 3:6]).all() and (rays[:, :, 3:6] != 0).all(), "a direction with a zero or non-finite component"
    occ = Oracle(path).trace(rays.reshape(-1, 8), any_hit=True)["hit"].reshape(-1, K)
    count = np.zeros((H, W), np.int64)
    count[tri] = (~occ).sum(axis=1)
    count[hit & ~tri] = K  # a line or a point: no ray, K unoccluded
    flip = np.zeros((H, W), bool)
    flip[tri] = flipped
    a = (count.astype(np.float32) / np.float32(K)).astype(np.float32)
    plane = np.stack([a, a, a, hit.astype(np.float32)], -1).astype(np.float32)
    return dict(plane=plane, count=count, hit=hit, tri=tri, flip=flip, kind=kind)
