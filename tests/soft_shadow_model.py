"""The expectation side of the soft shadow tests, independent of the feature's kernels: the
contract of yrt_shade_rays_soft / yrt_render_soft_shadows (include/yrt.h) restated in NumPy at one
sample per pixel, every intermediate held in float32.

  * The hit points come from the library's existing `position` AOV plane (at one sample it holds
    eval_pos of the hit exactly, the fact tests/ao_model.py builds on).
  * The K shadow rays per (hit, light) come from steps 1 to 5 below; every ray is answered by the
    CPU oracle's intersect_any.
  * The unshadowed per-light term T_li = ld + ls and the ambient la come from code that exists
    without the feature: yrt.render_light_groups, one light per group plus the ambient plane, on a
    twin scene that is the test scene without its blocker, at the pixels whose camera hit is the
    floor in both scenes (so that p, n, v and the material are the same and nothing shadows).
"""
import numpy as np

from helpers import Oracle

F0, F1 = np.float32(0.0), np.float32(1.0)
FLT_MAX = np.float32(3.4028234663852886e38)
TMIN = np.float32(0.01)


def f32(a):
    return np.asarray(a, np.float32)


def dot32(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + a[..., 2] * b[..., 2]).astype(np.float32)


def normalize_len(a):
    """yrt_math.h normalize and length: l = sqrtf(dot(a, a)), n = a * (1 / l), a itself at l == 0"""
    a = f32(a)
    ln = np.sqrt(dot32(a, a)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F1 / ln).astype(np.float32)
        n = (a * inv[..., None]).astype(np.float32)
    return np.where((ln == 0)[..., None], a, n).astype(np.float32), ln


def light_point(p, frame, lp0):
    """step 1's tp = transform_point(lf, lp0 - p): ((x * b.x + y * b.y) + z * b.z) + o"""
    frame, lp0, p = f32(frame), f32(lp0), f32(p)
    x, y, z, o = frame[0:3], frame[3:6], frame[6:9], frame[9:12]
    b = (lp0 - p).astype(np.float32)
    t = ((x * b[..., 0:1]).astype(np.float32) + (y * b[..., 1:2]).astype(np.float32)).astype(np.float32)
    t = (t + (z * b[..., 2:3]).astype(np.float32)).astype(np.float32)
    return (t + o).astype(np.float32)


def rot_index(p, li):
    """step 3: the rotation index of hit points p (N, 3) under light li"""
    q = (f32(p) + F0).astype(np.float32)  # -0 + 0 = +0
    b = q.view(np.uint32)
    u = b[..., 0] ^ b[..., 1] ^ b[..., 2]
    u = u ^ (u >> np.uint32(16))
    u = u ^ (u >> np.uint32(8))
    u = u ^ (u >> np.uint32(4))
    return ((u ^ np.uint32(li)) & np.uint32(15)).astype(np.int64)


def basis(l):
    """step 4: Duff et al. about l (N, 3)"""
    lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
    sg = np.where(lz >= F0, F1, -F1).astype(np.float32)
    a = (-F1 / (sg + lz).astype(np.float32)).astype(np.float32)
    b = ((lx * ly).astype(np.float32) * a).astype(np.float32)
    b1 = np.stack([(F1 + (((sg * lx).astype(np.float32) * lx).astype(np.float32) * a).astype(np.float32)),
                   sg * b, (-sg) * lx], 1).astype(np.float32)
    b2 = np.stack([b, sg + ((ly * ly).astype(np.float32) * a).astype(np.float32), -ly], 1).astype(np.float32)
    return b1, b2


def shadow_rays(p, frame, lp0, R, K, li, dirs, rots):
    """steps 1 to 5 for hit points p (N, 3) and one light: (N, K', 8) float32 rays, K' = K, or 1
    when R == 0 (step 2: the hard shadow ray, no basis and no offset)"""
    p = f32(p).reshape(-1, 3)
    R = np.float32(R)
    tp = light_point(p, frame, lp0)
    l, r = normalize_len(tp)
    n = len(p)
    if R == 0:
        rays = np.zeros((n, 1, 8), np.float32)
        rays[:, 0, 0:3], rays[:, 0, 3:6], rays[:, 0, 6], rays[:, 0, 7] = p, l, TMIN, (r - TMIN).astype(np.float32)
        return rays
    rot = rot_index(p, li)
    c, sn = f32(rots)[rot, 0], f32(rots)[rot, 1]
    b1, b2 = basis(l)
    rays = np.zeros((n, K, 8), np.float32)
    for k in range(K):
        tx, ty = np.float32(dirs[k][0]), np.float32(dirs[k][1])
        x = ((c * tx).astype(np.float32) - (sn * ty).astype(np.float32)).astype(np.float32)
        y = ((sn * tx).astype(np.float32) + (c * ty).astype(np.float32)).astype(np.float32)
        off = ((b1 * x[:, None]).astype(np.float32) + (b2 * y[:, None]).astype(np.float32)).astype(np.float32)
        tq = (tp + (off * R).astype(np.float32)).astype(np.float32)
        lq, rq = normalize_len(tq)
        rays[:, k, 0:3], rays[:, k, 3:6], rays[:, k, 6], rays[:, k, 7] = p, lq, TMIN, (rq - TMIN).astype(np.float32)
    assert rays.dtype == np.float32
    return rays


def open_counts(path, p, lights, radii, K, tables):
    """(nlights, N) int64: per light the unoccluded rays of hit points p (N, 3), 0..K; a light of
    radius 0 gives K or 0. lights: [(frame12, lp0)] in scene order; path: the scene's file"""
    dirs, rots = tables
    orc = Oracle(path)
    out = np.zeros((len(lights), len(p)), np.int64)
    for li, (frame, lp0) in enumerate(lights):
        rays = shadow_rays(p, frame, lp0, radii[li], K, li, dirs, rots)
        assert np.isfinite(rays).all()
        occ = orc.trace(rays.reshape(-1, 8), any_hit=True)["hit"].reshape(len(p), -1)
        out[li] = (~occ).sum(axis=1) * (K if np.float32(radii[li]) == 0 else 1)
    return out


def shaded(T, la, opens, K):
    """step 6 and the ambient: c = +0; per light in order c = c + T_li * f_li, skipped at
    open == 0; then c + la. T (nlights, N, 3), la (N, 3), opens (nlights, N) -> (N, 3), and c"""
    c = np.zeros_like(f32(la))
    for li in range(len(T)):
        f = (opens[li].astype(np.float32) / np.float32(K)).astype(np.float32)
        term = (f32(T[li]) * f[:, None]).astype(np.float32)
        c = np.where((opens[li] > 0)[:, None], (c + term).astype(np.float32), c)
    return (c + f32(la)).astype(np.float32), c


def scene_lights(path, light_instances):
    """[(frame12, lp0)] of the instances `light_instances` (Scene.lights()) of a .yrtscene file
    (csrc/scene_io.cpp save_yrtscene: gzip; cameras, textures, materials, shapes, instances, each
    behind a u32 count): the instance's frame and its shape's first vertex, what shade() takes a
    light's position from (raytrace.cpp:129-130)"""
    import gzip
    import struct

    d = gzip.open(path, "rb").read()
    assert d[:8] == b"YRTSCN1\0"
    at = [8]

    def u32():
        at[0] += 4
        return struct.unpack_from("<I", d, at[0] - 4)[0]

    ncam = u32()
    at[0] += ncam * 64  # cameras: frame, fovy, aspect, aperture, focus
    for _ in range(u32()):  # textures: width, height, RGBA8 pixels
        w, h = u32(), u32()
        at[0] += w * h * 4
    materials = []
    for _ in range(u32()):  # ke, kd, ks, kr, rs, kd_txt, ks_txt
        materials.append(np.frombuffer(d, np.float32, 3, at[0]))
        at[0] += 60
    first = []
    for _ in range(u32()):  # pos, norm, texcoord, radius, points, lines, triangles
        for k, size in enumerate((12, 12, 8, 4, 4, 8, 12)):
            n = u32()
            if k == 0:
                first.append(np.frombuffer(d, np.float32, 3, at[0]).copy() if n else None)
            at[0] += n * size
    lights, emitters = [], []
    for k in range(u32()):
        frame = np.frombuffer(d, np.float32, 12, at[0]).copy()
        shp, mat = struct.unpack_from("<ii", d, at[0] + 48)
        at[0] += 56
        if (materials[mat] > 0).all():
            emitters.append(k)
        if k in light_instances:
            lights.append((frame, first[shp]))
    assert at[0] == len(d) and emitters == list(light_instances), "the file's emitters are not Scene.lights()"
    return lights


def hard_shadowed_model(yrt, ds, path, lights, radii, K, amb, res, width=0, camera=0):
    """What yrt_render_soft_shadows must give at one sample per pixel and max_depth = 1 on any
    scene, without a twin: the per-light term comes from render_light_groups on the scene itself,
    where a group's plane is T_li when the hard shadow ray is open and +0 when it is not. So the
    expected colour is known on the hit pixels where every light with open > 0 also has its hard
    ray open: {"rgba", "known" (H, W) bool, "open", "hard" (nlights, H, W)}."""
    a = yrt.render_aovs(ds, res, 1, width=width, camera=camera, aovs=("position",))["position"]
    hit = a[..., 3] == 1
    p = a[..., :3][hit]
    tables = yrt.ao_tables()
    opens = open_counts(path, p, lights, radii, K, tables)
    hard = open_counts(path, p, lights, [0.0] * len(lights), K, tables)
    g = yrt.render_light_groups(ds, amb, res, 1, groups=list(range(len(lights))), ambient=True, beauty=False, width=width,
                                max_depth=1, camera=camera)
    T = np.stack([pl[..., :3][hit] for pl in g["groups"]])
    rgb, _ = shaded(T, g["ambient"][..., :3][hit], opens, K)
    known_hit = ((opens == 0) | (hard > 0)).all(axis=0)
    H, W = hit.shape
    out = np.zeros((H, W, 4), np.float32)
    out[hit, :3], out[hit, 3] = rgb, F1
    known = np.zeros((H, W), bool)
    known[hit] = known_hit
    full = np.zeros((2, len(lights), H, W), np.int64)
    full[0][:, hit], full[1][:, hit] = opens, hard
    return dict(rgba=out, known=known, hit=hit, open=full[0], hard=full[1])


_frames = {}


def frame_terms(yrt, ds, twin, amb, res, width, key):
    """the one-sample frame's data, made once per (key, frame): pos, nrm (H, W, 3), floor (H, W)
    bool -- the camera hit is instance 0 in both scenes --, T (nlights, H, W, 3), la (H, W, 3)"""
    k = (key, res, width, tuple(amb))
    if k not in _frames:
        a = yrt.render_aovs(ds, res, 1, width=width, aovs=("position", "normal", "ids"))
        b = yrt.render_aovs(twin, res, 1, width=width, aovs=("position", "ids"))
        floor = (a["position"][..., 3] == 1) & (a["ids"][..., 0] == 0) & (b["position"][..., 3] == 1) & (b["ids"][..., 0] == 0)
        assert np.array_equal(a["position"][floor].view(np.uint32), b["position"][floor].view(np.uint32))
        host = twin.host if hasattr(twin, "host") else twin
        n = len(host.lights())
        g = yrt.render_light_groups(twin, amb, res, 1, groups=list(range(n)), ambient=True, beauty=False, width=width,
                                    max_depth=1)
        _frames[k] = dict(pos=a["position"][..., :3].copy(), nrm=a["normal"][..., :3].copy(), floor=floor,
                          T=np.stack([pl[..., :3] for pl in g["groups"]]).copy(), la=g["ambient"][..., :3].copy())
        for v in _frames[k].values():
            v.setflags(write=False)
    return _frames[k]


def soft_model(yrt, ds, twin, path, lights, radii, K, amb, res, width, key):
    """What yrt_render_soft_shadows must give at one sample per pixel on the floor pixels:
    {"rgba" (H, W, 4) float32 (zeros off the floor), "floor" (H, W) bool, "open" (nlights, H, W),
    "c" the light sum, "la", "pos", "nrm"}"""
    g = frame_terms(yrt, ds, twin, amb, res, width, key)
    floor = g["floor"]
    opens = open_counts(path, g["pos"][floor], lights, radii, K, yrt.ao_tables())
    rgb, c = shaded(g["T"][:, floor], g["la"][floor], opens, K)
    H, W = floor.shape
    out = np.zeros((H, W, 4), np.float32)
    out[floor, :3], out[floor, 3] = rgb, F1
    full_open = np.zeros((len(lights), H, W), np.int64)
    full_open[:, floor] = opens
    full_c = np.zeros((H, W, 3), np.float32)
    full_c[floor] = c
    return dict(rgba=out, floor=floor, open=full_open, c=full_c, la=g["la"], pos=g["pos"], nrm=g["nrm"])
