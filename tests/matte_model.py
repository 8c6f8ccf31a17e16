"""The expectation side of the ID-matte tests: the oracle's intersect_first of every camera
sample (as tests/test_gpu_aov.py::oracle_samples builds it), the matte contract of
include/yrt.h written once as a model over those samples, and the built scene of
tests/test_gpu_aov.py made again. No GPU and no libyrt kernels here."""
import ctypes as C

import numpy as np

from helpers import Oracle, oracle_lib

KEYS = ("instance", "material", "shape")

_traces = {}


def oracle_samples(name_or_path, res, width, s, key=None):
    """the oracle's intersect_first of every camera sample: dict of (s, s, H, W[, 4]) arrays
    indexed [jj, ii, j, i], rays built by oracle_camera_ray (oracle.c eval_camera)"""
    key = (key or name_or_path, res, width, s)
    if key in _traces:
        return _traces[key]
    orc = Oracle(name_or_path)
    lib = oracle_lib()
    W, H = orc.image_size(res)
    W = width or W
    rays = np.zeros((s, s, H, W, 8), np.float32)
    ray8 = (C.c_float * 8)()
    for jj in range(s):
        for ii in range(s):
            for j in range(H):
                for i in range(W):
                    assert lib.oracle_camera_ray(orc.h, 0, res, width, s, i, j, ii, jj, ray8) == 0
                    rays[jj, ii, j, i] = ray8
    t = orc.trace(rays.reshape(-1, 8))
    out = {k: v.reshape((s, s, H, W) + v.shape[1:]) for k, v in t.items()}
    _traces[key] = out
    return out


def key_values(t, instances):
    """per key the id of every sample, (s, s, H, W) int32, -1 on a miss: the instance index, and
    through `instances` = [(shape, material)] in scene order the material and the shape"""
    hit, inst = t["hit"], t["inst"]
    shp = np.array([sm[0] for sm in instances], np.int32)
    mat = np.array([sm[1] for sm in instances], np.int32)
    safe = np.where(hit, inst, 0)
    return {"instance": np.where(hit, inst, -1).astype(np.int32),
            "material": np.where(hit, mat[safe], -1).astype(np.int32),
            "shape": np.where(hit, shp[safe], -1).astype(np.int32)}


def matte_tables(values, hit, ranks):
    """the contract, sample by sample: per pixel a table of `ranks` entries, empty at first; a
    miss does nothing; a hit whose id is in the table adds one to its count, else takes a free
    entry with count 1, else is dropped. Then the entries by count descending, ties by id
    ascending. Returns ids (H, W, ranks) int32 (-1 unused), counts (H, W, ranks) int32,
    dropped (H, W) int64 and distinct (H, W) int: the pixel's number of different ids."""
    s, _, H, W = hit.shape
    ids = np.full((H, W, ranks), -1, np.int32)
    counts = np.zeros((H, W, ranks), np.int32)
    dropped = np.zeros((H, W), np.int64)
    distinct = np.zeros((H, W), np.int64)
    for j in range(H):
        for i in range(W):
            table = []  # [id, count] in order of first appearance
            seen = set()
            for jj in range(s):
                for ii in range(s):
                    if not hit[jj, ii, j, i]:
                        continue
                    v = int(values[jj, ii, j, i])
                    seen.add(v)
                    entry = next((e for e in table if e[0] == v), None)
                    if entry is not None:
                        entry[1] += 1
                    elif len(table) < ranks:
                        table.append([v, 1])
                    else:
                        dropped[j, i] += 1
            table.sort(key=lambda e: (-e[1], e[0]))
            for r, (v, n) in enumerate(table):
                ids[j, i, r], counts[j, i, r] = v, n
            distinct[j, i] = len(seen)
    return ids, counts, dropped, distinct


def coverage_of(counts, s):
    """rank r's coverage: float(count) / float(s * s) in float32; +0.0 for an unused rank"""
    return (counts.astype(np.float32) / np.float32(s * s)).astype(np.float32)


_models = {}


def matte_model(name_or_path, instances, res, width, s, ranks, key=None):
    """{key: {"ids", "coverage", "counts", "dropped" (per pixel), "distinct"}} plus "hits" (H, W):
    what yrt_render_mattes must give for the scene, computed once per case"""
    k = (key or name_or_path, res, width, s, ranks)
    if k in _models:
        return _models[k]
    t = oracle_samples(name_or_path, res, width, s, key=key)
    vals = key_values(t, instances)
    out = {"hits": t["hit"].sum(axis=(0, 1)).astype(np.int64)}
    for name in KEYS:
        ids, counts, dropped, distinct = matte_tables(vals[name], t["hit"], ranks)
        out[name] = {"ids": ids, "coverage": coverage_of(counts, s), "counts": counts, "dropped": dropped,
                     "distinct": distinct}
    _models[k] = out
    return out


# ---- the built scene of tests/test_gpu_aov.py: every primitive kind, a texture, a rotated
# instance, two instances of one shape and two of one material ----
def rot_y(a):
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], np.float32)


def frame(rot=None, o=(0, 0, 0)):
    r = np.eye(3, dtype=np.float32) if rot is None else rot
    return np.concatenate([r.reshape(-1), np.asarray(o, np.float32)]).astype(np.float32)


class Built:
    """the built scene, the (shape, material) its instances were added with, and its file"""


_built = {}


def built_scene(yrt, tmp_path_factory):
    if _built:
        return _built["b"]
    rng = np.random.default_rng(2024)
    b = Built()
    s = yrt.Scene.create()
    eye = np.array([0.5, 2.5, 7], np.float32)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0, 1, 0], z).astype(np.float32)
    x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(np.float32)
    s.add_camera(np.concatenate([x, y, z, eye]).astype(np.float32), fovy=0.7, aspect=37 / 24,
                 focus=float(np.linalg.norm(eye)))
    tex = rng.integers(0, 256, (16, 8, 4)).astype(np.uint8)
    t0 = s.add_texture(tex)
    mats = [dict(kd=(0.5, 0.25, 0.125), ks=(0.1, 0.1, 0.1), rs=0.3),
            dict(kd=(0.9, 0.8, 0.7), ks=(0.2, 0.2, 0.2), rs=0.5, kd_txt=t0),
            dict(kd=(0.3, 0.6, 0.2), rs=0.2),
            dict(kd=(0.2, 0.3, 0.8), rs=0.4)]
    m_floor, m_tex, m_line, m_dot = [s.add_material(**m) for m in mats]
    b.insts = []
    nshapes = [0]

    def shape(kind, pos, norm, tc, elems, radius=None):
        pos, norm, tc = (np.asarray(a, np.float32) for a in (pos, norm, tc))
        idx = s.add_shape(pos, norm=norm, texcoord=tc, radius=radius, **{kind: np.asarray(elems, np.int32)})
        assert idx == nshapes[0]
        nshapes[0] += 1
        return idx

    def instance(fr, shp, mat):
        assert s.add_instance(fr, shp, mat) == len(b.insts)
        b.insts.append((shp, mat))

    g = np.linspace(-4, 4, 5, dtype=np.float32)
    gx, gz = np.meshgrid(g, g)
    fpos = np.stack([gx.ravel(), 0.1 * np.sin(gx.ravel() + gz.ravel()), gz.ravel()], 1)
    fnorm = np.array([0, 1.5, 0], np.float32) + rng.uniform(-0.3, 0.3, (25, 3)).astype(np.float32)
    tris = []
    for j in range(4):
        for i in range(4):
            a, q, c, d = j * 5 + i, j * 5 + i + 1, (j + 1) * 5 + i + 1, (j + 1) * 5 + i
            tris += [(a, d, c), (a, c, q)]
    floor = shape("triangles", fpos, fnorm, fpos[:, [0, 2]] / 8 + 0.5, tris)
    qpos = [[-1.5, 0, 0], [1.5, 0, 0], [1.5, 2, 0], [-1.5, 2, 0]]
    quad = shape("triangles", qpos, [[0, 0.2, 1], [0.2, 0, 1], [0, -0.2, 1], [-0.2, 0, 1]],
                 [[0, 0], [2.5, 0], [2.5, 1.5], [0, 1.5]], [[0, 1, 2], [0, 2, 3]])
    lpos = [[-3, 0.3, 1], [-2.2, 1.6, 1.2], [-1.6, 0.4, 2], [2.2, 0.3, 1.5], [3, 1.8, 1]]
    lines = shape("lines", lpos, rng.normal(size=(5, 3)), rng.uniform(0, 1, (5, 2)), [[0, 1], [1, 2], [3, 4]],
                  radius=np.array([0.2, 0.1, 0.15, 0.12, 0.25], np.float32))
    ppos = rng.uniform([-3, 0.5, -2], [3, 2.5, 3], (12, 3))
    dots = shape("points", ppos, rng.normal(size=(12, 3)), rng.uniform(0, 1, (12, 2)), np.arange(12),
                 radius=rng.uniform(0.2, 0.4, 12).astype(np.float32))
    instance(frame(), floor, m_floor)
    instance(frame(rot_y(0.7), (0.5, 0.3, -1.0)), quad, m_tex)
    instance(frame(o=(0, 0, 0.5)), lines, m_line)
    instance(frame(), dots, m_dot)
    instance(frame(rot_y(-0.4), (-2.5, 0.2, 0.5)), quad, m_floor)  # the quad's shape and the floor's material again
    b.path = tmp_path_factory.mktemp("mattes") / "built.yrtscene"
    s.save(str(b.path))
    yrt.build_bvh(s)
    b.scene = s
    _built["b"] = b
    return b
