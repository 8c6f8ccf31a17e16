"""The camera models of yrt_render_camera / yrt_camera_rays restated in numpy (not a test module):
include/yrt.h's formulas, the text of csrc/camera_models.h.

rays() is float32 throughout, evaluated in the header's order, so PERSPECTIVE and ORTHOGRAPHIC
equal the host's and the device's rays bit for bit (numpy neither fuses a*b+c nor reorders; sqrt
and the division are correctly rounded everywhere). The camera's h comes from libm's tanf through
ctypes, the call make_dev_camera makes: np.tan may differ by an ulp. EQUIRECT calls sinf and
cosf, which differ between libms, so its yardstick is rays64(): the same formulas in float64 with
the exact pi, from the float32 camera.

Rays are (H, W, ns * ns, 8) {o.xyz, d.xyz, tmin, tmax}: a pixel's samples in the order q = jj *
ns + ii. quad_image() renders the lens test's scene of axis-aligned quads from such rays.
"""
import ctypes as C

import numpy as np

F = np.float32
PERSPECTIVE, ORTHOGRAPHIC, EQUIRECT = 0, 1, 2
MODELS = {"perspective": PERSPECTIVE, "orthographic": ORTHOGRAPHIC, "equirect": EQUIRECT}
RAY_EPS, FLT_MAX = F(1e-4), np.finfo(np.float32).max

_libm = C.CDLL("libm.so.6")
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]


def tables():
    """(dirs (64, 3), rots (16, 2)) float32: the library's tables (yrt_ao_tables, host only)"""
    import yocto_raytracing_amd as yrt

    return yrt.ao_tables()


def dev_camera(frame, fovy, aspect, focus):
    """make_dev_camera (csrc/device_scene.cpp): o, x, y = frame.y * -1, z, h, w, focus"""
    f = np.asarray(frame, F).reshape(4, 3)
    focus = F(focus)
    h = F(F(F(2.0) * focus) * F(_libm.tanf(float(F(fovy) / F(2.0)))))
    return {"x": f[0], "y": (f[1] * F(-1)).astype(F), "z": f[2], "o": f[3], "h": h, "w": F(h * F(aspect)), "focus": focus}


def scene_camera(cam: dict, focus=None):
    """dev_camera of Scene.camera()'s dict, with the focus replaced when given (> 0)"""
    return dev_camera(cam["frame"], cam["fovy"], cam["aspect"], cam["focus"] if focus is None else focus)


def _normalize(a):
    """yrt_math.h normalize: a * (1 / sqrt(a.x*a.x + a.y*a.y + a.z*a.z)), a itself at length 0"""
    l = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        n = a * (F(1) / l)[..., None]
    return np.where((l == 0)[..., None], a, n).astype(F)


def _grid(W, H, ns, window):
    x0, y0, tw, th = window if window is not None else (0, 0, W, H)
    j, i, q = np.meshgrid(np.arange(y0, y0 + th), np.arange(x0, x0 + tw), np.arange(ns * ns), indexing="ij")
    return i, j, q, q % ns, q // ns


def rays(cam, model, W, H, ns, aperture=0.0, window=None, tabs=None):
    """(h, w, ns * ns, 8) float32: the rays of camera_model_eval for the window (x0, y0, w, h) of
    the W x H frame (default: all of it). `aperture` is the resolved lens diameter."""
    i, j, q, ii, jj = _grid(W, H, ns, window)
    u = (i.astype(F) + (ii.astype(F) + F(0.5)) / F(ns)) / F(W)
    v = (j.astype(F) + (jj.astype(F) + F(0.5)) / F(ns)) / F(H)
    assert u.dtype == F and v.dtype == F
    o, x, y, z = cam["o"], cam["x"], cam["y"], cam["z"]
    uw, vh = ((u - F(0.5)) * cam["w"])[..., None], ((v - F(0.5)) * cam["h"])[..., None]
    out = np.zeros(u.shape + (8,), F)
    out[..., 6], out[..., 7] = RAY_EPS, FLT_MAX
    if model == ORTHOGRAPHIC:
        out[..., 0:3] = (o + uw * x) + vh * y
        out[..., 3:6] = _normalize(np.broadcast_to(-z, u.shape + (3,)))
    elif model == EQUIRECT:
        phi, th = (u - F(0.5)) * F(6.2831855), v * F(3.1415927)
        st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(phi), np.cos(phi)
        a, g = (st * sp)[..., None], (st * cp)[..., None]
        out[..., 0:3] = o
        out[..., 3:6] = _normalize(((a * x - ct[..., None] * y) - g * z).astype(F))
    else:
        Q = ((o + uw * x) + vh * y) - cam["focus"] * z
        e = np.broadcast_to(o, Q.shape)
        if not F(aperture) == 0:
            dirs, rots = tabs if tabs is not None else tables()
            R = F(aperture) * F(0.5)
            k = q & 63
            tx, ty = dirs[k, 0], dirs[k, 1]
            r = (((i & 3) | ((j & 3) << 2)) ^ (q >> 6)) & 15
            c, sn = rots[r, 0], rots[r, 1]
            lx, ly = (R * (c * tx - sn * ty))[..., None], (R * (sn * tx + c * ty))[..., None]
            e = (o + lx * x) + ly * y
        assert Q.dtype == F and e.dtype == F
        out[..., 0:3] = e
        out[..., 3:6] = _normalize(Q - e)
    return out


def rays64(cam, W, H, ns, window=None):
    """EQUIRECT's directions in float64, (h, w, ns * ns, 3): the formulas with the exact pi, from
    the float32 camera (the origins are cam["o"] exactly)"""
    i, j, q, ii, jj = _grid(W, H, ns, window)
    u = (i + (ii + 0.5) / ns) / W
    v = (j + (jj + 0.5) / ns) / H
    x, y, z = (cam[k].astype(np.float64) for k in "xyz")
    phi, th = (u - 0.5) * (2 * np.pi), v * np.pi
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(phi), np.cos(phi)
    d = ((st * sp)[..., None] * x - ct[..., None] * y) - (st * cp)[..., None] * z
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- the cameras and the bound the CPU and GPU tests share ----
# EQUIRECT against rays64, per direction component: 2^-18 is 64 ulp of 1. The angles carry at most
# 4 roundings at magnitude <= 2 pi (<~ 1.5e-6), sinf and cosf add <= 2 ulp, the remaining ~8
# roundings <~ 5e-7: about 2.1e-6, below 3.8e-6.
PANORAMA_BOUND = 2.0 ** -18
HAND_FOVY, HAND_ASPECT, HAND_FOCUS = 0.9, 1.5, 3.0


def hand_frame():
    """the hand-made camera's frame: rotated, off the origin, not axis aligned in any component"""
    from shade_rays_scene import look_at

    return look_at((1.0, 2.0, 3.0), (0.25, 0.5, -1.0))[0]


def lens_test_camera():
    """the lens test's camera as Scene.camera() gives one: at the origin looking down -z,
    tan(fovy / 2) = 0.5, aspect 1"""
    return dict(frame=np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0].astype(F), fovy=float(F(2 * np.arctan(0.5))), aspect=1.0,
                aperture=0.0, focus=2.0)


# ---- the lens test's scene: quads across the view axis of a camera at the origin looking down -z ----
# (z, x from, x to, half height, kd): a quad [x from, x to] x [-half height, half height] at depth z
LENS_QUADS = ((-2.0, -10.0, 0.0, 10.0, 1.0), (-6.0, 1.5, 30.0, 30.0, 1.0), (-12.0, -60.0, 60.0, 60.0, 0.0))
LENS_BEHIND = (6.0, -4.0, 4.0, 4.0, 1.0)  # the panorama test's quad behind the camera


def quad_image(r, quads=LENS_QUADS):
    """(h, w) float64: per pixel the mean over its samples of the kd of the nearest quad a ray
    hits (0 on a miss): what raytrace gives for unlit quads under ambient 1, from an analytic
    ray/plane hit"""
    o, d = r[..., 0:3].astype(np.float64), r[..., 3:6].astype(np.float64)
    best = np.full(r.shape[:-1], np.inf)
    val = np.zeros(r.shape[:-1])
    for z, x0, x1, hy, kd in quads:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (z - o[..., 2]) / d[..., 2]
        px, py = o[..., 0] + t * d[..., 0], o[..., 1] + t * d[..., 1]
        hit = (t > 1e-4) & (px >= x0) & (px <= x1) & (np.abs(py) <= hy) & (t < best)
        best = np.where(hit, t, best)
        val = np.where(hit, kd, val)
    return val.mean(axis=-1)


def transitional(row, lo, hi):
    """the pixels of row[lo:hi] that lie strictly between the plateaus: more than 1/32 away from
    both 0 and 1"""
    seg = np.asarray(row)[lo:hi]
    return int(((seg > 1 / 32) & (seg < 31 / 32)).sum())
