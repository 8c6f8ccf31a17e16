"""The scenes and ray batches of tests/test_gpu_shade_rays.py and tests/shade_rays_worker.py (not
a test module).

"built" is tests/passes_scene.py's scene with two more cameras after its own: camera 1 looks at
the two mirrors from the side, camera 2 down on the floor from the other side, so the three
cameras' rays start at three different points. The rays are the reference's eval_camera rays
(oracle_camera_ray, helpers.oracle_lib()) in the order (j, i, jj, ii): a pixel's s*s samples are
consecutive, jj outer and ii inner, which is the order raytrace() sums them in.
"""
import ctypes as C

import numpy as np

import passes_scene as PS
from helpers import Oracle, oracle_lib

RES, WIDTH = 24, 37
NCAMERAS = 3


def look_at(eye, target):
    """a camera frame (x, y, z, o: the camera looks along -z) at `eye` towards `target`"""
    eye, target = np.asarray(eye, np.float32), np.asarray(target, np.float32)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0, 1, 0], z).astype(np.float32)
    x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(np.float32)
    return np.concatenate([x, y, z, eye]).astype(np.float32), float(np.linalg.norm(eye - target))


def build(yrt):
    """passes_scene.build(yrt) (BVH not built) with cameras 1 and 2 added"""
    s = PS.build(yrt)
    for eye, target, fovy in (((6.5, 1.8, 1.0), (0.0, 1.0, -1.5), 0.8), ((-3.0, 4.0, 6.0), (0.0, 0.5, 0.0), 0.6)):
        f, focus = look_at(eye, target)
        s.add_camera(f, fovy=fovy, aspect=PS.ASPECT, focus=focus)
    assert s.info()["cameras"] == NCAMERAS
    return s


def camera_rays(name_or_path, s, camera=0, res=RES, width=WIDTH):
    """(res * width * s * s, 8) float32: the reference's camera rays of the frame, (j, i, jj, ii)"""
    orc = Oracle(name_or_path)
    lib = oracle_lib()
    rays = np.zeros((res, width, s, s, 8), np.float32)
    ray8 = (C.c_float * 8)()
    for j in range(res):
        for i in range(width):
            for jj in range(s):
                for ii in range(s):
                    assert lib.oracle_camera_ray(orc.h, camera, res, width, s, i, j, ii, jj, ray8) == 0
                    rays[j, i, jj, ii] = ray8
    return rays.reshape(-1, 8)


def box_filter(colours, s, res=RES, width=WIDTH):
    """raytrace.cpp:232-249 on per-ray colours in camera_rays' order: per pixel the float32 sum
    over jj (outer) and ii (inner) from +0, divided by float32(s * s), alpha 1"""
    c = np.asarray(colours, np.float32).reshape(res, width, s, s, 4)
    acc = np.zeros((res, width, 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for jj in range(s):
            for ii in range(s):
                acc = (acc + c[:, :, jj, ii, :3]).astype(np.float32)
        img = np.ones((res, width, 4), np.float32)
        img[..., :3] = acc / np.float32(s * s)
    return img
