"""The AOV pass on the GPU (yrt_render_aovs, aov.hip k_aov): depth, ids and the sample order
against the oracle bit for bit; albedo against the oracle's own shading of a scene whose
shade() reduces to kd; position, normal and uv against eval_pos / eval_norm / eval_texcoord
recomputed in float32 NumPy; windows, band shards, row stride, absent planes, edge scenes,
isolation from yrt_render, host planes and the CLI's .npy files."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import ATOL, ROOT, RTOL, Oracle, assert_same_floats, close_mask, oracle_lib, scene_path

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
FLOAT_AOVS = ("depth", "position", "normal", "texcoord", "albedo")
ALL_AOVS = FLOAT_AOVS + ("ids",)
RES, WIDTH = 24, 37  # 37 columns, 24 rows: partial 8 x 8 tiles on both axes, three blocks across


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


_scenes = {}


def dev_scene(yrt, name):
    if name not in _scenes:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][1]


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


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


def ordered_sum(values, hit, s):
    """the float32 sum over (jj, ii) in that order of the hit samples' values, started from
    0.0f, a miss adding nothing, divided by float(s * s)"""
    acc = np.zeros(values.shape[2:], np.float32)
    for jj in range(s):
        for ii in range(s):
            h = hit[jj, ii]
            acc[h] = (acc[h] + values[jj, ii][h]).astype(np.float32)
    return (acc / np.float32(s * s)).astype(np.float32)


def expected_ids01(t):
    hit = t["hit"][0, 0]
    return np.stack([np.where(hit, t["inst"][0, 0], -1), np.where(hit, t["ei"][0, 0], -1)], -1).astype(np.int32)


# ---- 1. depth and ids against the oracle ----
@pytest.mark.parametrize("name", ["simple", "lines", "instance1k", "mirrors"])
def test_depth_coverage_and_ids_equal_the_oracle(yrt, name):
    t = oracle_samples(name, RES, WIDTH, 1)
    aov = yrt.render_aovs(dev_scene(yrt, name), RES, 1, width=WIDTH, aovs=("depth", "ids"))
    hit = t["hit"][0, 0]
    assert aov["depth"].shape == (RES, WIDTH, 4) and aov["ids"].dtype == np.int32
    assert hit.any()
    assert_same_floats(aov["depth"][..., 0], np.where(hit, t["dist"][0, 0], np.float32(0)))
    assert_same_floats(aov["depth"][..., 3], hit.astype(np.float32))
    assert not aov["depth"][..., 1:3].any()
    np.testing.assert_array_equal(aov["ids"][..., 0:2], expected_ids01(t))
    np.testing.assert_array_equal(aov["ids"][~hit], -1)
    assert (aov["ids"][hit] >= 0).all()


# ---- 2. the sample order ----
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["simple", "lines"])
def test_samples_are_summed_in_the_reference_order(yrt, name, s):
    t = oracle_samples(name, RES, WIDTH, s)
    aov = yrt.render_aovs(dev_scene(yrt, name), RES, s, width=WIDTH, aovs=("depth", "ids"))
    assert_same_floats(aov["depth"][..., 0], ordered_sum(t["dist"], t["hit"], s))
    assert_same_floats(aov["depth"][..., 3], ordered_sum(np.ones_like(t["dist"]), t["hit"], s))
    if name == "lines":  # (every sample of `simple` hits its walls)
        partial = (aov["depth"][..., 3] > 0) & (aov["depth"][..., 3] < 1)
        assert partial.any(), "no pixel with partial coverage: a miss's place in the order is not exercised"
    np.testing.assert_array_equal(aov["ids"][..., 0:2], expected_ids01(t))


# ---- 3./4. a built scene: every primitive kind, a texture, a rotated instance ----
def rot_y(a):
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], np.float32)


def frame(rot=None, o=(0, 0, 0)):
    r = np.eye(3, dtype=np.float32) if rot is None else rot
    return np.concatenate([r.reshape(-1), np.asarray(o, np.float32)]).astype(np.float32)


class Built:
    """the scene of tests 3 and 4 and the arrays it was made from"""


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
    # no emissive material and no mirror: shade() is amb * kd (* its texture)
    mats = [dict(kd=(0.5, 0.25, 0.125), ks=(0.1, 0.1, 0.1), rs=0.3),
            dict(kd=(0.9, 0.8, 0.7), ks=(0.2, 0.2, 0.2), rs=0.5, kd_txt=t0),
            dict(kd=(0.3, 0.6, 0.2), rs=0.2),
            dict(kd=(0.2, 0.3, 0.8), rs=0.4)]
    m_floor, m_tex, m_line, m_dot = [s.add_material(**m) for m in mats]
    b.shapes, b.insts = [], []

    def shape(kind, pos, norm, tc, elems, radius=None):
        pos, norm, tc = (np.asarray(a, np.float32) for a in (pos, norm, tc))
        elems = np.asarray(elems, np.int32)
        idx = s.add_shape(pos, norm=norm, texcoord=tc, radius=radius, **{kind: elems})
        assert idx == len(b.shapes)
        b.shapes.append(dict(kind=kind, pos=pos, norm=norm, tc=tc, elems=elems.reshape(len(elems), -1)))
        return idx

    def instance(fr, shp, mat):
        assert s.add_instance(fr, shp, mat) == len(b.insts)
        b.insts.append((fr, shp, mat))

    # an untextured floor grid with tilted, unnormalised vertex normals
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
    # a textured quad whose uv run past 1 (the lookup wraps)
    qpos = [[-1.5, 0, 0], [1.5, 0, 0], [1.5, 2, 0], [-1.5, 2, 0]]
    quad = shape("triangles", qpos, [[0, 0.2, 1], [0.2, 0, 1], [0, -0.2, 1], [-0.2, 0, 1]],
                 [[0, 0], [2.5, 0], [2.5, 1.5], [0, 1.5]], [[0, 1, 2], [0, 2, 3]])
    # thick line segments and point spheres
    lpos = [[-3, 0.3, 1], [-2.2, 1.6, 1.2], [-1.6, 0.4, 2], [2.2, 0.3, 1.5], [3, 1.8, 1]]
    lines = shape("lines", lpos, rng.normal(size=(5, 3)), rng.uniform(0, 1, (5, 2)), [[0, 1], [1, 2], [3, 4]],
                  radius=np.array([0.2, 0.1, 0.15, 0.12, 0.25], np.float32))
    ppos = rng.uniform([-3, 0.5, -2], [3, 2.5, 3], (12, 3))
    dots = shape("points", ppos, rng.normal(size=(12, 3)), rng.uniform(0, 1, (12, 2)), np.arange(12),
                 radius=rng.uniform(0.2, 0.4, 12).astype(np.float32))
    instance(frame(), floor, m_floor)
    instance(frame(rot_y(0.7), (0.5, 0.3, -1.0)), quad, m_tex)  # the rotated orthonormal frame
    instance(frame(o=(0, 0, 0.5)), lines, m_line)
    instance(frame(), dots, m_dot)
    instance(frame(rot_y(-0.4), (-2.5, 0.2, 0.5)), quad, m_floor)  # the quad's shape again, untextured
    b.kd = np.array([m["kd"] for m in mats], np.float32)
    b.path = tmp_path_factory.mktemp("aov") / "built.yrtscene"
    s.save(str(b.path))
    yrt.build_bvh(s)
    b.scene = s
    _built["b"] = b
    return b


@pytest.mark.parametrize("s", [1, 3])
def test_albedo_equals_the_oracles_shading(yrt, tmp_path_factory, s):
    """without emission, lights and mirrors, shade() with amb = 1 returns (0 + la) with
    la = 1.0f * kd (* the kd_txt lookup): the albedo AOV's .xyz, sample sums included"""
    b = built_scene(yrt, tmp_path_factory)
    want, _, _ = Oracle(b.path).render(RES, s, amb=1.0)
    aov = yrt.render_aovs(b.scene, RES, s, aovs=("albedo", "ids"))
    got = aov["albedo"][..., :3]
    assert got.shape == want[..., :3].shape == (RES, WIDTH, 3)
    both_zero = (got == 0) & (want[..., :3] == 0)  # -0 + 0: a miss is +0 on both sides anyway
    assert_same_floats(np.where(both_zero, np.float32(0), got), np.where(both_zero, np.float32(0), want[..., :3]))
    mats_seen = set(np.unique(aov["ids"][..., 2])) - {-1}
    assert mats_seen == {0, 1, 2, 3}, mats_seen  # every material, the textured one included
    assert (got > 0).any() and (aov["albedo"][..., 3] == 0).any()


def normalize32(v):
    l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(np.float32)).astype(np.float32)
    return (v / l[:, None]).astype(np.float32)


def test_position_normal_uv_equal_the_eval_functions(yrt, tmp_path_factory):
    b = built_scene(yrt, tmp_path_factory)
    t = oracle_samples(b.path, RES, 0, 1, key="built")
    hit, inst, ei, ew = (t[k][0, 0] for k in ("hit", "inst", "ei", "ew"))
    H, W = hit.shape
    assert (H, W) == (RES, WIDTH)
    want = {n: np.zeros((H, W, 4), np.float32) for n in ("position", "normal", "texcoord")}
    ids = np.full((H, W, 4), -1, np.int32)
    kinds = set()
    for k, (fr, shp, mat) in enumerate(b.insts):
        sel = hit & (inst == k)
        if not sel.any():
            continue
        sh = b.shapes[shp]
        kinds.add(sh["kind"])
        el, w = sh["elems"][ei[sel]], ew[sel]
        n = el.shape[1]  # 1, 2 or 3 vertices per element
        lp = sum((sh["pos"][el[:, c]] * w[:, c:c + 1]).astype(np.float32) for c in range(n)).astype(np.float32)
        ln = sum((sh["norm"][el[:, c]] * w[:, c:c + 1]).astype(np.float32) for c in range(n)).astype(np.float32)
        uv = sum((sh["tc"][el[:, c]] * w[:, c:c + 1]).astype(np.float32) for c in range(n)).astype(np.float32)
        if sh["kind"] == "points":  # eval_pos / eval_norm of a point: the vertex itself; no texcoord
            lp, ln, uv = sh["pos"][el[:, 0]], sh["norm"][el[:, 0]], np.zeros((len(el), 2), np.float32)
        else:
            ln = normalize32(ln)
        fx, fy, fz, fo = fr[0:3], fr[3:6], fr[6:9], fr[9:12]
        xf = lambda v: (fx * v[:, 0:1] + fy * v[:, 1:2] + fz * v[:, 2:3]).astype(np.float32)  # noqa: E731
        want["position"][sel] = np.concatenate([(xf(lp) + fo).astype(np.float32), np.ones((len(el), 1), np.float32)], 1)
        want["normal"][sel] = np.concatenate([normalize32(xf(ln)), np.ones((len(el), 1), np.float32)], 1)
        want["texcoord"][sel] = np.concatenate([uv, np.zeros((len(el), 1), np.float32),
                                                np.ones((len(el), 1), np.float32)], 1)
        ids[sel] = np.stack([inst[sel], ei[sel], np.full(len(el), mat), np.full(len(el), shp)], 1)
    assert kinds == {"triangles", "lines", "points"}, kinds
    aov = yrt.render_aovs(b.scene, RES, 1, aovs=("position", "normal", "texcoord", "ids"))
    for name, ref in want.items():
        ok = close_mask(aov[name], ref, ATOL, RTOL)
        exact = (aov[name].view(np.uint32) == ref.view(np.uint32)).mean()
        print(f"{name}: {exact:.4f} of the channels bit-exact, max |diff| {np.abs(aov[name] - ref).max():.3g}")
        assert ok.all(), (name, np.argwhere(~ok)[:5], aov[name][~ok][:5], ref[~ok][:5])
    np.testing.assert_array_equal(aov["ids"], ids)


# ---- 5. windows, bands, stride, absent planes ----
def full_planes(yrt, s=2):
    key = ("full", s)
    if key not in _traces:
        _traces[key] = yrt.render_aovs(dev_scene(yrt, "simple"), RES, s, width=WIDTH, aovs=ALL_AOVS)
    return _traces[key]


def host_planes(shape):
    return {n: np.zeros(shape + (4,), np.int32 if n == "ids" else np.float32) for n in ALL_AOVS}


def test_window_equals_the_crop(yrt):
    full = full_planes(yrt)
    win = yrt.render_aovs(dev_scene(yrt, "simple"), RES, 2, width=WIDTH, aovs=ALL_AOVS, window=(5, 3, 19, 11))
    for n in ALL_AOVS:
        assert full[n][..., :3].any()
        same_bits(win[n], np.ascontiguousarray(full[n][3:14, 5:24]))


@pytest.mark.parametrize("res,band", [(24, 8), (24, 3), (20, 8), (20, 3)])
def test_band_shards_reassemble(yrt, res, band):
    """shards of stride 3 at every offset; 20 rows end in a partial band of 4 (band 8) or 2 (band 3)"""
    ds = dev_scene(yrt, "simple")
    full = full_planes(yrt) if res == RES else yrt.render_aovs(ds, res, 2, width=WIDTH, aovs=ALL_AOVS)
    got = {n: np.full_like(full[n], 77) for n in ALL_AOVS}
    seen = np.zeros(res, int)
    for off in range(3):
        p = yrt.render_params(resolution=res, samples=2, width=WIDTH, band=(band, 3, off))
        bands_total = -(-res // band)
        th = len(range(off, bands_total, 3)) * band
        planes = host_planes((th, WIDTH))
        ds.render_aovs_into(p, {n: a.ctypes.data for n, a in planes.items()}, device_memory=False)
        for ly in range(th):
            j = ((ly // band) * 3 + off) * band + ly % band
            if j < res:
                seen[j] += 1
                for n in ALL_AOVS:
                    got[n][j] = planes[n][ly]
            else:  # local rows past the image edge (the partial last band) read as zeros, ids -1
                for n in ALL_AOVS:
                    assert (planes[n][ly] == (-1 if n == "ids" else 0)).all()
    assert (seen == 1).all()
    for n in ALL_AOVS:
        same_bits(got[n], full[n])


def test_row_padding_is_not_written(yrt):
    import torch

    full = full_planes(yrt)
    x0, y0, tw, th = 5, 3, 19, 11
    stride = tw + 5
    p = yrt.render_params(resolution=RES, samples=2, width=WIDTH, window=(x0, y0, tw, th))
    p.out_stride = stride
    dev = {n: torch.full((th, stride, 4), float("nan"), dtype=torch.float32, device="cuda:0") for n in ALL_AOVS}
    nan_bits = dev["ids"][0, 0, 0].cpu().numpy().view(np.uint32)
    dev_scene(yrt, "simple").render_aovs_into(p, {n: a.data_ptr() for n, a in dev.items()}, device_memory=True)
    torch.cuda.synchronize()
    host = {n: np.zeros((th, stride, 4), np.float32) for n in ALL_AOVS}
    for a in host.values():
        a.view(np.uint32)[...] = 0x7fc01234  # the caller's bytes of a host plane's padding
    dev_scene(yrt, "simple").render_aovs_into(p, {n: a.ctypes.data for n, a in host.items()}, device_memory=False)
    for n in ALL_AOVS:
        a = dev[n].cpu().numpy()
        assert (a[:, tw:].view(np.uint32) == nan_bits).all(), n
        np.testing.assert_array_equal(a[:, :tw].view(np.uint32), full[n][y0:y0 + th, x0:x0 + tw].view(np.uint32))
        assert (host[n][:, tw:].view(np.uint32) == 0x7fc01234).all(), n
        np.testing.assert_array_equal(host[n][:, :tw].view(np.uint32), full[n][y0:y0 + th, x0:x0 + tw].view(np.uint32))


def test_normal_alone_with_every_other_plane_null(yrt):
    full = full_planes(yrt)
    only = yrt.render_aovs(dev_scene(yrt, "simple"), RES, 2, width=WIDTH, aovs=("normal",))
    assert list(only) == ["normal"]
    same_bits(only["normal"], full["normal"])


def test_invalid_arguments(yrt):
    from yocto_raytracing_amd import _native as N

    ds = dev_scene(yrt, "simple")
    p = yrt.render_params(resolution=8)
    buf = np.zeros((8, 16, 4), np.float32)
    planes = N.AovPlanes()
    planes.plane[0] = buf.ctypes.data
    call = lambda prm, mask: N.lib.yrt_render_aovs(ds.handle, C.byref(prm), mask, C.byref(planes), 0, None)  # noqa: E731
    assert call(p, 0) == 1
    assert call(p, 1 << N.YRT_AOV_COUNT) == 1
    assert call(p, 0b11) == 1  # position requested, its plane null
    p.camera = 5
    assert call(p, 1) == 1 and b"camera index out of range" in N.lib.yrt_last_error()
    assert not buf.any()


# ---- 6. edges ----
@pytest.mark.parametrize("name", ["edge_sky", "edge_empty"])
def test_scenes_where_every_ray_misses(yrt, name):
    aov = yrt.render_aovs(dev_scene(yrt, name), 12, 2, width=19, aovs=ALL_AOVS)
    for n in FLOAT_AOVS:
        same_bits(aov[n], np.zeros((12, 19, 4), np.float32))
    np.testing.assert_array_equal(aov["ids"], -1)


def test_empty_band_offset_writes_nothing_and_counts_nothing(yrt):
    ds = dev_scene(yrt, "simple")
    res, s = 12, 2
    yrt.render_aovs(ds, res, s, width=WIDTH, aovs=("depth",))
    assert ds.last_stats()["rays"] == WIDTH * res * s * s  # the counters an empty call must not repeat
    # 12 rows are two bands of 8: offset 2 of 3 has none
    p = yrt.render_params(resolution=res, samples=s, width=WIDTH, band=(8, 3, 2))
    planes = {n: np.full((8, WIDTH, 4), 77, np.int32 if n == "ids" else np.float32) for n in ALL_AOVS}
    ds.render_aovs_into(p, {n: a.ctypes.data for n, a in planes.items()}, device_memory=False)
    st = ds.last_stats()
    assert st["rays"] == 0 and st["camera_samples"] == 0
    for a in planes.values():
        assert (a == 77).all()
    yrt.render_aovs(ds, res, s, width=WIDTH, aovs=ALL_AOVS)
    st = ds.last_stats()
    assert st["rays"] == st["camera_samples"] == WIDTH * res * s * s and st["shadow_rays"] == 0


# ---- 7. isolation from yrt_render ----
def test_the_pass_leaves_yrt_render_alone(yrt):
    ds = dev_scene(yrt, "simple")
    before = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    lists = ds.tile_lists()
    yrt.render_aovs(ds, RES, 3, aovs=ALL_AOVS)
    assert ds.tile_lists() == lists
    after = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    same_bits(after, before)
    assert ds.tile_lists() == lists


# ---- 8. host planes, device planes, the CLI's files ----
def test_host_planes_equal_device_planes(yrt):
    import torch

    full = full_planes(yrt)
    p = yrt.render_params(resolution=RES, samples=2, width=WIDTH)
    dev = {n: torch.zeros((RES, WIDTH, 4), dtype=torch.int32 if n == "ids" else torch.float32, device="cuda:0")
           for n in ALL_AOVS}
    torch.cuda.synchronize()
    dev_scene(yrt, "simple").render_aovs_into(p, {n: a.data_ptr() for n, a in dev.items()}, device_memory=True)
    torch.cuda.synchronize()
    for n in ALL_AOVS:
        same_bits(dev[n].cpu().numpy(), full[n])


def test_cli_writes_npy_files(yrt, tmp_path):
    out = tmp_path / "o.png"
    r = subprocess.run([str(CLI), "--aov", ",".join(ALL_AOVS), "-r", "36", "-s", "2", "-o", str(out),
                        str(scene_path("simple"))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.exists()
    want = yrt.render_aovs(dev_scene(yrt, "simple"), 36, 2, aovs=ALL_AOVS)
    for n in ALL_AOVS:
        f = tmp_path / f"o.{n}.npy"
        head = f.read_bytes()[:10]
        assert head[:8] == b"\x93NUMPY\x01\x00" and (10 + head[8] + 256 * head[9]) % 64 == 0
        a = np.load(f)
        assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.dtype("<i4") if n == "ids" else np.dtype("<f4"))
        same_bits(a, want[n])
