"""The scene of the light-group tests (tests/test_gpu_light_groups*.py, tests/light_groups_worker.py;
not a test module): passes_scene.build()'s scene with three more point lights appended after
it, so five lights in instance order -- instances 7, 8, 10, 11, 12 -- with the emitter whose
ke.y is 0 (instance 9, not a light) between them.

build(yrt, lit, mirrors) is a variant: the lights not in `lit` get ke = 0 (they are then no
lights, raytrace.cpp:126), and without `mirrors` every kr is 0. A group's plane is the beauty
of the variant that keeps the group's lights, rendered with ambient 0; the ambient plane that of
the variant without any light, rendered with the ambient.
"""
import numpy as np

import passes_scene as PS

# ke and position of the appended lights (radius 0.002 each)
MORE_LIGHTS = [((25, 25, 25), (-1.0, 3.5, 5.5)), ((8, 16, 6), (3.8, 1.2, 2.5)), ((30, 12, 12), (-0.5, 5.0, -2.5))]
BASE_LIGHT_MATERIALS = (6, 7)  # passes_scene.MATERIALS: the two lights, in instance order
LIGHTS = [7, 8, 10, 11, 12]    # instance index of each light
GROUP_OF = [0, 1, 0, -1, 2]
NGROUPS = 3


def lights_of(group_of, g):
    """the lights (indices into the scene's light order) of group g"""
    return tuple(k for k, gk in enumerate(group_of) if gk == g)


def build(yrt, lit=None, mirrors=True, more_lights=True):
    """the scene (BVH not built); `lit`: the lights, by index in light order, that keep their ke
    (None: all of them); more_lights=False: passes_scene's own two lights only"""
    nl = len(BASE_LIGHT_MATERIALS) + (len(MORE_LIGHTS) if more_lights else 0)
    keep = set(range(nl)) if lit is None else set(lit)
    assert keep <= set(range(nl))
    mats = [dict(m) for m in PS.MATERIALS]
    for k, m in enumerate(BASE_LIGHT_MATERIALS):
        if k not in keep:
            mats[m]["ke"] = (0, 0, 0)
    if not mirrors:
        for m in mats:
            m["kr"] = (0, 0, 0)
    # passes_scene.build reads its module's material table when it is called
    saved, PS.MATERIALS = PS.MATERIALS, mats
    try:
        s = PS.build(yrt)
    finally:
        PS.MATERIALS = saved
    for k, (ke, pos) in enumerate(MORE_LIGHTS if more_lights else ()):
        mat = s.add_material(ke=ke if k + len(BASE_LIGHT_MATERIALS) in keep else (0, 0, 0))
        shp = s.add_shape(np.asarray([pos], np.float32), norm=np.asarray([[0, 1, 0]], np.float32),
                          texcoord=np.asarray([[0.5, 0.5]], np.float32), radius=np.array([0.002], np.float32),
                          points=np.array([0], np.int32))
        s.add_instance(PS.frame(), shp, mat)
    return s
