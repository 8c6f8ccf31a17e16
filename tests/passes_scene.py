"""The scene of tests/test_gpu_passes.py and tests/passes_worker.py (not a test module): one of
every thing the shading passes tell apart, built with the scene builder.

A textured floor (kd_txt), a glossy quad (ks > 0, ns = 510) and a rotated instance of it, a
tapered line strip, a point, a partial mirror (kd > 0, kr > 0), a pure mirror (kd = ks = 0,
three different kr), two point lights of different ke and an emitter whose ke has a zero
component, which shade() (raytrace.cpp:126) does not take for a light.

build(yrt, variant) rewrites the materials: the terms a variant switches off leave the
oracle's beauty of that variant equal to one pass of the unmodified scene.
"""
import numpy as np

NLIGHTS = 2  # the emitters shade() loops over with an unoccluded term (ke > 0 in every component)
PURE_MIRROR = 5  # material index of the pure mirror
ASPECT = 37 / 24

# what each variant sets to zero in every material (and the ambient it is rendered with: see
# VARIANT_AMB); None is the unmodified scene
VARIANTS = {
    None: (),
    "ambient": ("ke", "kr"),
    "diffuse": ("ks", "kr"),
    "specular": ("kd", "kr"),
    "direct": ("kr",),
}
AMB = 0.1
VARIANT_AMB = {"ambient": AMB, "diffuse": 0.0, "specular": 0.0, "direct": 0.0}

MATERIALS = [
    dict(kd=(0.9, 0.8, 0.7), ks=(0.1, 0.1, 0.1), rs=0.5),        # 0 floor (gets kd_txt)
    dict(kd=(0.3, 0.2, 0.4), ks=(0.5, 0.4, 0.3), rs=0.25),       # 1 glossy: ns = 2 / rs^4 - 2 = 510
    dict(kd=(0.3, 0.6, 0.2), ks=(0.2, 0.2, 0.2), rs=0.4),        # 2 line strip
    dict(kd=(0.2, 0.3, 0.8), ks=(0.3, 0.3, 0.3), rs=1.0),        # 3 point: ns = 0
    dict(kd=(0.2, 0.2, 0.3), kr=(0.5, 0.5, 0.5), rs=0.3),        # 4 partial mirror
    dict(kr=(0.9, 0.6, 0.3)),                                     # 5 pure mirror
    dict(ke=(40, 40, 40)),                                        # 6 light
    dict(ke=(10, 20, 30)),                                        # 7 light
    dict(ke=(5, 0, 5), kd=(0.5, 0.5, 0.5)),                       # 8 not a light: ke.y == 0
]


def rot_y(a):
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    return np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], np.float32)


def frame(rot=None, o=(0, 0, 0)):
    r = np.eye(3, dtype=np.float32) if rot is None else rot
    return np.concatenate([r.reshape(-1), np.asarray(o, np.float32)]).astype(np.float32)


def build(yrt, variant=None):
    """the scene (BVH not built) with `variant`'s terms set to zero in every material"""
    rng = np.random.default_rng(7)
    s = yrt.Scene.create()
    eye = np.array([0.5, 2.5, 7], np.float32)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0, 1, 0], z).astype(np.float32)
    x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(np.float32)
    s.add_camera(np.concatenate([x, y, z, eye]).astype(np.float32), fovy=0.7, aspect=ASPECT,
                 focus=float(np.linalg.norm(eye)))
    t0 = s.add_texture(rng.integers(32, 256, (16, 8, 4)).astype(np.uint8))
    mats = []
    for k, m in enumerate(MATERIALS):
        m = dict(m)
        for term in VARIANTS[variant]:
            m[term] = (0, 0, 0)
        if k == 0:
            m["kd_txt"] = t0
        mats.append(s.add_material(**m))

    def quad(pos, n, tc=((0, 0), (1, 0), (1, 1), (0, 1))):
        return s.add_shape(np.asarray(pos, np.float32), norm=np.tile(np.asarray(n, np.float32), (4, 1)),
                           texcoord=np.asarray(tc, np.float32), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32))

    floor = quad([[-5, 0, 5], [5, 0, 5], [5, 0, -5], [-5, 0, -5]], (0, 1, 0), ((0, 0), (2.5, 0), (2.5, 2.5), (0, 2.5)))
    panel = quad([[-0.8, 0, 0], [0.8, 0, 0], [0.8, 1.6, 0], [-0.8, 1.6, 0]], (0, 0, 1))
    mirror = quad([[-1.2, 0, 0], [1.2, 0, 0], [1.2, 2.2, 0], [-1.2, 2.2, 0]], (0, 0, 1))
    lpos = np.array([[-3.2, 0.4, 2.0], [-2.6, 1.5, 2.2], [-1.9, 0.5, 2.6], [-1.5, 1.4, 2.4]], np.float32)
    # every shape carries normals and texture coordinates: eval_norm and eval_texcoord
    # (scene.h:176-206) index them without asking whether they are there. The strip's normals
    # stay well away from both lights' directions and from the half vectors, so that
    # sqrt(1 - |n.l|) and sqrt(1 - |n.h|) (raytrace.cpp:170-171) are never the root of a negative
    lnorm = np.array([[0.3, -0.2, 1.0], [0.2, -0.1, 1.0], [0.35, -0.25, 1.0], [0.25, -0.15, 1.0]], np.float32)
    strip = s.add_shape(lpos, norm=lnorm, texcoord=np.array([[0, 0], [0.3, 0], [0.6, 0], [1, 0]], np.float32),
                        radius=np.array([0.25, 0.12, 0.2, 0.05], np.float32),
                        lines=np.array([[0, 1], [1, 2], [2, 3]], np.int32))

    def point(p, r):
        return s.add_shape(np.asarray([p], np.float32), norm=np.asarray([[0, 1, 0]], np.float32),
                           texcoord=np.asarray([[0.5, 0.5]], np.float32), radius=np.array([r], np.float32),
                           points=np.array([0], np.int32))

    ball = point((0.3, 0.6, 3.0), 0.5)
    s.add_instance(frame(), floor, mats[0])
    s.add_instance(frame(o=(-0.3, 0.0, 0.8)), panel, mats[1])
    s.add_instance(frame(rot_y(0.6), (2.6, 0.0, 1.6)), panel, mats[1])  # the rotated instance
    s.add_instance(frame(), strip, mats[2])
    s.add_instance(frame(), ball, mats[3])
    s.add_instance(frame(rot_y(0.5), (-2.4, 0.0, -1.5)), mirror, mats[4])
    s.add_instance(frame(rot_y(-0.45), (2.2, 0.0, -1.8)), mirror, mats[5])
    # shade() takes a light's position from its shape's first vertex (raytrace.cpp:129)
    s.add_instance(frame(), point((2.0, 4.5, 4.0), 0.002), mats[6])
    s.add_instance(frame(), point((-3.5, 3.0, 4.5), 0.002), mats[7])
    s.add_instance(frame(), point((0.5, 2.6, 0.5), 0.3), mats[8])
    return s
