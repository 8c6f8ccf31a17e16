"""The ID-matte pass on the GPU (yrt_render_mattes, mattes.hip k_matte): ids and coverages
against the contract's model over the oracle's intersect_first results (tests/matte_model.py)
bit for bit, tables that overflow, one sample per pixel against the ids AOV, the accounting
against the depth AOV's coverage, key subsets, windows, band shards, row stride, host planes,
edge scenes, isolation from yrt_render, invalid arguments and the CLI's .npy files."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import ROOT, scene_path
from matte_model import KEYS, built_scene, matte_model

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
RES, WIDTH = 24, 37  # 37 columns, 24 rows: partial 8 x 8 tiles on both axes, three blocks across


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


_scenes = {}


def host_scene(yrt, name):
    if name not in _scenes:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][0]


def dev_scene(yrt, name):
    host_scene(yrt, name)
    return _scenes[name][1]


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


_renders = {}


def rendered(yrt, name, res, width, s, ranks):
    """all three keys from one call, once per case"""
    key = (name, res, width, s, ranks)
    if key not in _renders:
        _renders[key] = yrt.render_mattes(dev_scene(yrt, name), res, s, keys=KEYS, ranks=ranks, width=width)
    return _renders[key]


def model_of(yrt, name, res, width, s, ranks):
    return matte_model(name, host_scene(yrt, name).instances(), res, width, s, ranks)


def assert_equals_model(got, want, ranks):
    for k in KEYS:
        assert got[k]["ids"].shape == want[k]["ids"].shape == got[k]["coverage"].shape
        assert got[k]["ids"].shape[-1] == ranks
        assert got[k]["ids"].dtype == np.int32 and got[k]["coverage"].dtype == np.float32
        np.testing.assert_array_equal(got[k]["ids"], want[k]["ids"], err_msg=k)
        same_bits(got[k]["coverage"], want[k]["coverage"])
        assert got["dropped"][k] == int(want[k]["dropped"].sum()), k


def empty_ranks(m):
    """unused ranks are (-1, +0.0f), used ones an id >= 0 with a coverage above 0"""
    unused = m["ids"] == -1
    return unused, (m["coverage"].view(np.uint32)[unused] == 0).all() and (m["coverage"][~unused] > 0).all()


def samples_of(m, ids, s):
    """the samples per pixel that the entries of `ids` hold: their counts, from the coverages"""
    counts = np.rint(m["coverage"].astype(np.float64) * (s * s)).astype(np.int64)
    return np.where(np.isin(m["ids"], list(ids)), counts, 0).sum(-1)


# ---- 1. against the oracle ----
def test_lines_equals_the_model_with_ties_and_partial_pixels(yrt):
    s = 3
    got, want = rendered(yrt, "lines", RES, WIDTH, s, 4), model_of(yrt, "lines", RES, WIDTH, s, 4)
    assert_equals_model(got, want, 4)
    assert got["dropped"] == {"instance": 0, "material": 0, "shape": 0}
    c = want["instance"]["counts"]
    assert ((c[..., :-1] == c[..., 1:]) & (c[..., 1:] > 0)).any(), "no tie: the order by id is not exercised"
    assert ((want["hits"] > 0) & (want["hits"] < s * s)).any(), "no partially covered pixel"
    assert want["instance"]["distinct"].max() == 4 and want["instance"]["distinct"].min() == 0
    for k in KEYS:
        assert empty_ranks(got[k])[1]


def test_instance1k_eight_ranks_holds_every_id(yrt):
    got, want = rendered(yrt, "instance1k", 8, 13, 6, 8), model_of(yrt, "instance1k", 8, 13, 6, 8)
    assert got["instance"]["ids"].shape == (8, 13, 8)
    assert_equals_model(got, want, 8)
    assert got["dropped"] == {"instance": 0, "material": 0, "shape": 0}
    assert (got["instance"]["ids"][..., 4:] >= 0).any(), "no pixel uses the second layer"
    assert want["instance"]["distinct"].max() > 4


def test_instance1k_four_ranks_drops_what_does_not_fit(yrt):
    got, want = rendered(yrt, "instance1k", 8, 13, 6, 4), model_of(yrt, "instance1k", 8, 13, 6, 4)
    assert_equals_model(got, want, 4)
    assert got["dropped"]["instance"] > 0
    # a pixel with at most four ids has the table of the eight-rank call
    got8 = rendered(yrt, "instance1k", 8, 13, 6, 8)
    for k in KEYS:
        few = want[k]["distinct"] <= 4
        assert few.any() and (k != "instance" or not few.all())
        np.testing.assert_array_equal(got[k]["ids"][few], got8[k]["ids"][few][:, :4])
        same_bits(got[k]["coverage"][few], got8[k]["coverage"][few][:, :4])
        assert (got8[k]["ids"][few][:, 4:] == -1).all()


def test_instance100k_every_pixel_overflows_eight_ranks(yrt):
    got, want = rendered(yrt, "instance100k", 8, 13, 4, 8), model_of(yrt, "instance100k", 8, 13, 4, 8)
    assert (want["instance"]["dropped"] > 0).all() and want["instance"]["distinct"].min() > 8
    assert_equals_model(got, want, 8)
    assert got["dropped"]["instance"] >= 8 * 13
    assert (got["instance"]["ids"] >= 0).all()


def test_built_scene_material_and_shape_follow_the_construction(yrt, tmp_path_factory):
    b = built_scene(yrt, tmp_path_factory)
    assert b.scene.instances() == b.insts
    s = 3
    want = matte_model(str(b.path), b.insts, RES, 0, s, 4, key="built")  # the construction's own mapping
    got = yrt.render_mattes(b.scene, RES, s, keys=KEYS, ranks=4)
    assert got["instance"]["ids"].shape == (RES, WIDTH, 4)
    assert_equals_model(got, want, 4)
    assert got["dropped"] == {"instance": 0, "material": 0, "shape": 0}
    assert set(np.unique(got["instance"]["ids"])) == {-1, 0, 1, 2, 3, 4}
    # instances 0 and 4 share a material, 1 and 4 a shape: one entry, with their samples added up
    by_mat = {m: [k for k, sm in enumerate(b.insts) if sm[1] == m] for m in {sm[1] for sm in b.insts}}
    by_shp = {h: [k for k, sm in enumerate(b.insts) if sm[0] == h] for h in {sm[0] for sm in b.insts}}
    assert by_mat[0] == [0, 4] and by_shp[1] == [1, 4]
    for key, groups in (("material", by_mat), ("shape", by_shp)):
        for v, members in groups.items():
            np.testing.assert_array_equal(samples_of(got[key], [v], s), samples_of(got["instance"], members, s))
            assert ((got[key]["ids"] == v).sum(-1) <= 1).all()
    merged = want["material"]["distinct"] < want["instance"]["distinct"]
    assert merged.any(), "no pixel where two instances of one material meet"
    j, i = np.argwhere(merged)[0]
    assert (got["material"]["ids"][j, i] >= 0).sum() < (got["instance"]["ids"][j, i] >= 0).sum()


# ---- 2. one sample per pixel: the ids AOV ----
@pytest.mark.parametrize("name", ["lines", "instance1k"])
def test_one_sample_is_the_ids_aov(yrt, name):
    ds = dev_scene(yrt, name)
    ids = yrt.render_aovs(ds, RES, 1, width=WIDTH, aovs=("ids",))["ids"]
    got = yrt.render_mattes(ds, RES, 1, keys=KEYS, ranks=8, width=WIDTH)
    hit = ids[..., 0] >= 0
    assert hit.any() and (name != "lines" or (~hit).any())
    for k, channel in (("instance", 0), ("material", 2), ("shape", 3)):
        np.testing.assert_array_equal(got[k]["ids"][..., 0], ids[..., channel])
        same_bits(got[k]["coverage"][..., 0], hit.astype(np.float32))
        assert (got[k]["ids"][..., 1:] == -1).all()
        assert (got[k]["coverage"][..., 1:].view(np.uint32) == 0).all()
        assert (got[k]["ids"][~hit] == -1).all() and (got[k]["coverage"][~hit].view(np.uint32) == 0).all()
    assert got["dropped"] == {"instance": 0, "material": 0, "shape": 0}


# ---- 3. accounting against the depth AOV's coverage ----
@pytest.mark.parametrize("name,res,width,s,ranks", [("lines", RES, WIDTH, 3, 4), ("instance1k", 8, 13, 6, 4),
                                                    ("instance100k", 8, 13, 4, 8)])
def test_counts_and_dropped_add_up_to_the_hits(yrt, name, res, width, s, ranks):
    got, want = rendered(yrt, name, res, width, s, ranks), model_of(yrt, name, res, width, s, ranks)
    depth = yrt.render_aovs(dev_scene(yrt, name), res, s, width=width, aovs=("depth",))["depth"]
    hits = np.rint(depth[..., 3].astype(np.float64) * (s * s)).astype(np.int64)
    np.testing.assert_array_equal(hits, want["hits"])
    for k in KEYS:
        counts = np.rint(got[k]["coverage"].astype(np.float64) * (s * s)).astype(np.int64)
        np.testing.assert_array_equal(counts.sum(-1) + want[k]["dropped"], hits, err_msg=k)


# ---- 4. key subsets ----
def test_each_key_alone_equals_the_all_keys_call(yrt):
    import torch

    ds = dev_scene(yrt, "instance1k")
    res, width, s = 8, 13, 6
    for ranks in (4, 8):
        full = rendered(yrt, "instance1k", res, width, s, ranks)
        yrt.render_mattes(ds, res, s, keys=KEYS, ranks=ranks, width=width)
        st = ds.last_stats()
        assert st["rays"] == st["camera_samples"] == res * width * s * s and st["shadow_rays"] == 0
        for k in KEYS:
            one = yrt.render_mattes(ds, res, s, keys=(k,), ranks=ranks, width=width)
            st = ds.last_stats()
            assert st["rays"] == st["camera_samples"] == res * width * s * s
            assert list(one) == [k, "dropped"] and one["dropped"] == {k: full["dropped"][k]}
            np.testing.assert_array_equal(one[k]["ids"], full[k]["ids"])
            same_bits(one[k]["coverage"], full[k]["coverage"])
            assert ds.matte_dropped() == {q: (full["dropped"][q] if q == k else 0) for q in KEYS}
    # the planes of a key that is not requested are not touched: two keys, the third's planes NaN
    layers = 2
    dev = {k: {n: [torch.full((res, width, 4), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(layers)]
               for n in ("ids", "coverage")} for k in KEYS}
    nan_bits = dev["shape"]["ids"][0][0, 0, 0].cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    p = yrt.render_params(resolution=res, samples=s, width=width)
    from yocto_raytracing_amd import _native as N

    mp = N.MattePlanes()
    for k in KEYS:
        for l in range(layers):
            mp.ids[N.MATTE_KEYS[k]][l] = dev[k]["ids"][l].data_ptr()
            mp.coverage[N.MATTE_KEYS[k]][l] = dev[k]["coverage"][l].data_ptr()
    assert N.lib.yrt_render_mattes(ds.handle, C.byref(p), 0b101, layers, C.byref(mp), N.YRT_MEM_DEVICE, None) == 0
    torch.cuda.synchronize()
    full = rendered(yrt, "instance1k", res, width, s, 8)
    for n in ("ids", "coverage"):
        for l in range(layers):
            assert (dev["material"][n][l].cpu().numpy().view(np.uint32) == nan_bits).all()
            for k in ("instance", "shape"):
                np.testing.assert_array_equal(dev[k][n][l].cpu().numpy().view(np.uint32),
                                              full[k][n][..., 4 * l:4 * l + 4].view(np.uint32))
    # one layer asked of planes that have two: the second layer's are not touched either
    for t in dev["instance"]["ids"] + dev["instance"]["coverage"]:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    assert N.lib.yrt_render_mattes(ds.handle, C.byref(p), 0b001, 1, C.byref(mp), N.YRT_MEM_DEVICE, None) == 0
    torch.cuda.synchronize()
    assert (dev["instance"]["ids"][1].cpu().numpy().view(np.uint32) == nan_bits).all()
    np.testing.assert_array_equal(dev["instance"]["ids"][0].cpu().numpy().view(np.uint32),
                                  rendered(yrt, "instance1k", res, width, s, 4)["instance"]["ids"].view(np.uint32))


# ---- 5. windows, bands, stride, host planes ----
LAYOUT_S, LAYOUT_RANKS = 2, 8
PLANE_NAMES = [(k, n, l) for k in KEYS for n in ("ids", "coverage") for l in range(LAYOUT_RANKS // 4)]


def full_planes(yrt, res=RES):
    """`simple` at 24 x 37 (or res x 37), two samples per axis, as {(key, "ids" | "coverage", layer): (H, W, 4)}"""
    m = rendered(yrt, "simple", res, WIDTH, LAYOUT_S, LAYOUT_RANKS)
    return {(k, n, l): np.ascontiguousarray(m[k][n][..., 4 * l:4 * l + 4]) for k, n, l in PLANE_NAMES}


def host_planes(shape, fill):
    return {(k, n, l): np.full(shape + (4,), fill, np.int32 if n == "ids" else np.float32) for k, n, l in PLANE_NAMES}


def pointers(planes, ptr):
    return {k: {n: [ptr(planes[k, n, l]) for l in range(LAYOUT_RANKS // 4)] for n in ("ids", "coverage")} for k in KEYS}


def test_window_equals_the_crop(yrt):
    full = rendered(yrt, "simple", RES, WIDTH, LAYOUT_S, LAYOUT_RANKS)
    win = yrt.render_mattes(dev_scene(yrt, "simple"), RES, LAYOUT_S, keys=KEYS, ranks=LAYOUT_RANKS, width=WIDTH,
                            window=(5, 3, 19, 11))
    for k in KEYS:
        assert (full[k]["ids"][..., 1] >= 0).any()  # some pixel of the frame has two ids
        for n in ("ids", "coverage"):
            same_bits(win[k][n], np.ascontiguousarray(full[k][n][3:14, 5:24]))


@pytest.mark.parametrize("res,band", [(24, 8), (24, 3), (20, 8), (20, 3)])
def test_band_shards_reassemble(yrt, res, band):
    """shards of stride 3 at every offset; 20 rows end in a partial band of 4 (band 8) or 2 (band 3)"""
    ds = dev_scene(yrt, "simple")
    full = full_planes(yrt, res)
    got = {q: np.full_like(a, 77) for q, a in full.items()}
    seen = np.zeros(res, int)
    for off in range(3):
        p = yrt.render_params(resolution=res, samples=LAYOUT_S, width=WIDTH, band=(band, 3, off))
        bands_total = -(-res // band)
        th = len(range(off, bands_total, 3)) * band
        planes = host_planes((th, WIDTH), 55)
        ds.render_mattes_into(p, pointers(planes, lambda a: a.ctypes.data), LAYOUT_RANKS // 4, device_memory=False)
        for ly in range(th):
            j = ((ly // band) * 3 + off) * band + ly % band
            if j < res:
                seen[j] += 1
                for q in full:
                    got[q][j] = planes[q][ly]
            else:  # local rows past the image edge (the partial last band): id -1, coverage +0
                for (k, n, l), a in planes.items():
                    assert (a[ly] == -1).all() if n == "ids" else (a[ly].view(np.uint32) == 0).all()
    assert (seen == 1).all()
    for q in full:
        same_bits(got[q], full[q])


def test_row_padding_is_not_written(yrt):
    import torch

    full = full_planes(yrt)
    x0, y0, tw, th = 5, 3, 19, 11
    stride = tw + 5
    p = yrt.render_params(resolution=RES, samples=LAYOUT_S, width=WIDTH, window=(x0, y0, tw, th))
    p.out_stride = stride
    dev = {q: torch.full((th, stride, 4), float("nan"), dtype=torch.float32, device="cuda:0") for q in full}
    nan_bits = next(iter(dev.values()))[0, 0, 0].cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    dev_scene(yrt, "simple").render_mattes_into(p, pointers(dev, lambda t: t.data_ptr()), LAYOUT_RANKS // 4,
                                                device_memory=True)
    torch.cuda.synchronize()
    host = host_planes((th, stride), 0)
    for a in host.values():
        a.view(np.uint32)[...] = 0x7fc01234  # the caller's bytes of a host plane's padding
    dev_scene(yrt, "simple").render_mattes_into(p, pointers(host, lambda a: a.ctypes.data), LAYOUT_RANKS // 4,
                                                device_memory=False)
    for q in full:
        a = dev[q].cpu().numpy()
        assert (a[:, tw:].view(np.uint32) == nan_bits).all(), q
        np.testing.assert_array_equal(a[:, :tw].view(np.uint32), full[q][y0:y0 + th, x0:x0 + tw].view(np.uint32))
        assert (host[q][:, tw:].view(np.uint32) == 0x7fc01234).all(), q
        np.testing.assert_array_equal(host[q][:, :tw].view(np.uint32), full[q][y0:y0 + th, x0:x0 + tw].view(np.uint32))


def test_host_planes_equal_device_planes(yrt):
    import torch

    full = full_planes(yrt)  # (rendered into host planes)
    p = yrt.render_params(resolution=RES, samples=LAYOUT_S, width=WIDTH)
    dev = {q: torch.zeros((RES, WIDTH, 4), dtype=torch.float32, device="cuda:0") for q in full}
    torch.cuda.synchronize()
    dev_scene(yrt, "simple").render_mattes_into(p, pointers(dev, lambda t: t.data_ptr()), LAYOUT_RANKS // 4,
                                                device_memory=True)
    torch.cuda.synchronize()
    for q in full:
        np.testing.assert_array_equal(dev[q].cpu().numpy().view(np.uint32), full[q].view(np.uint32))


def test_empty_band_offset_writes_nothing_and_counts_nothing(yrt):
    ds = dev_scene(yrt, "instance1k")
    res, width, s = 8, 13, 6
    got = yrt.render_mattes(ds, res, s, keys=KEYS, ranks=4, width=width)
    assert ds.last_stats()["rays"] == width * res * s * s and got["dropped"]["instance"] > 0
    assert ds.matte_dropped()["instance"] > 0  # the totals an empty call must not repeat
    # 8 rows are one band of 8: offset 1 of 3 has none
    p = yrt.render_params(resolution=res, samples=s, width=width, band=(8, 3, 1))
    planes = host_planes((8, width), 77)
    ds.render_mattes_into(p, pointers(planes, lambda a: a.ctypes.data), LAYOUT_RANKS // 4, device_memory=False)
    st = ds.last_stats()
    assert st["rays"] == 0 and st["camera_samples"] == 0
    assert ds.matte_dropped() == {"instance": 0, "material": 0, "shape": 0}
    for a in planes.values():
        assert (a == 77).all()
    yrt.render_mattes(ds, res, s, keys=("instance",), ranks=4, width=width)
    st = ds.last_stats()
    assert st["rays"] == st["camera_samples"] == width * res * s * s and st["shadow_rays"] == 0


# ---- 6. edges ----
@pytest.mark.parametrize("name", ["edge_sky", "edge_empty"])
def test_scenes_where_every_ray_misses(yrt, name):
    got = yrt.render_mattes(dev_scene(yrt, name), 12, 2, keys=KEYS, ranks=8, width=19)
    for k in KEYS:
        np.testing.assert_array_equal(got[k]["ids"], np.full((12, 19, 8), -1, np.int32))
        same_bits(got[k]["coverage"], np.zeros((12, 19, 8), np.float32))
    assert got["dropped"] == {"instance": 0, "material": 0, "shape": 0}


# ---- 7. isolation from yrt_render ----
def test_the_pass_leaves_yrt_render_alone(yrt):
    ds = dev_scene(yrt, "simple")
    before = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    lists = ds.tile_lists()
    yrt.render_mattes(ds, RES, 3, keys=KEYS, ranks=8)
    assert ds.tile_lists() == lists
    after = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    same_bits(after, before)
    assert ds.tile_lists() == lists


# ---- 8. invalid arguments with a real handle ----
def test_invalid_arguments(yrt):
    from yocto_raytracing_amd import _native as N

    ds = dev_scene(yrt, "simple")
    p = yrt.render_params(resolution=8, width=16)
    ids, cov = np.zeros((8, 16, 4), np.int32), np.zeros((8, 16, 4), np.float32)
    planes = N.MattePlanes()
    planes.ids[0][0], planes.coverage[0][0] = ids.ctypes.data, cov.ctypes.data

    def call(prm, mask, layers, mem=0):
        return N.lib.yrt_render_mattes(ds.handle, C.byref(prm), mask, layers, C.byref(planes), mem, None)

    assert call(p, 0, 1) == 1
    assert call(p, 1 << 3, 1) == 1
    assert call(p, 0b1001, 1) == 1
    assert call(p, 1, 0) == 1
    assert call(p, 1, 3) == 1
    assert call(p, 0b11, 1) == 1  # the material key requested, its planes null
    assert call(p, 1, 2) == 1  # two layers requested, the second layer's planes null
    assert call(p, 1, 1, mem=2) == 1 and call(p, 1, 1, mem=-1) == 1
    planes.coverage[0][0] = None
    assert call(p, 1, 1) == 1  # the ids plane alone
    planes.coverage[0][0] = cov.ctypes.data
    p.camera = 5
    assert call(p, 1, 1) == 1 and b"camera index out of range" in N.lib.yrt_last_error()
    assert not ids.any() and not cov.any()
    p.camera = 0
    assert call(p, 1, 1) == 0 and ids.any() and cov.any()  # (the same call, once every argument is good)


# ---- 9. the CLI's files ----
@pytest.mark.parametrize("ranks", [4, 8])
def test_cli_writes_npy_files(yrt, tmp_path, ranks):
    out = tmp_path / "o.png"
    extra = [] if ranks == 4 else ["--matte-ranks", "8"]
    r = subprocess.run([str(CLI), "--mattes", ",".join(KEYS), *extra, "-r", "36", "-s", "2", "-o", str(out),
                        str(scene_path("simple"))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.exists() and "dropped" not in r.stderr
    want = yrt.render_mattes(dev_scene(yrt, "simple"), 36, 2, keys=KEYS, ranks=ranks)
    assert want["dropped"] == {"instance": 0, "material": 0, "shape": 0}
    for k in KEYS:
        for n, descr in (("ids", "<i4"), ("coverage", "<f4")):
            f = tmp_path / f"o.matte_{k}.{n}.npy"
            head = f.read_bytes()[:10]
            assert head[:8] == b"\x93NUMPY\x01\x00" and (10 + head[8] + 256 * head[9]) % 64 == 0
            a = np.load(f)
            assert a.flags["C_CONTIGUOUS"] and a.dtype == np.dtype(descr) and a.shape[-1] == ranks
            same_bits(a, want[k][n])
