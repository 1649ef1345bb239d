"""The generators' scenes somewhere else, at another size, with another axis up: what the culls owe to where a scene sits.

Placed(scene, scale, shift, rotation) wraps a HostScene, an OracleScene or anything else with the generators' verbs and maps
what they are given through p -> s R p + t: points so, directions through R, lengths (radii, h_distance / v_distance, checker
sizes) times s.  Each component is computed in double and rounded to fp32 once, so the host model and the oracle receive the
same bits.  camera_two_mirrors() places the reference's two-mirrors camera the same way: eye and look-at point through the map,
up = R z, the screen and its distance times s (cameras.camera(), cameras.put()).  The identity placement forwards every call
untouched.  Everything that is no placing verb -- set_* included -- passes through to the wrapped scene.

An improper rotation (det R = -1) gives a valid scene, not the mirror image pixel for pixel: the verbs derive a rectangle's
second axis and the camera's horizontal vector by cross products, which a reflection turns round.

PLACEMENTS is the catalogue the placement tests run under; large_scale() is the scale of its "large" entry."""
import numpy as np

import cameras

F = np.float32
IDENTITY = np.eye(3)


def permutation(*images):
    """the matrix that takes x, y, z to the signed axes `images`: "x" "y" "z" "-x" "-y" "-z" -> float64 (3, 3), exact"""
    m = np.zeros((3, 3))
    for col, image in enumerate(images):
        m["xyz".index(image[-1]), col] = -1.0 if image[0] == "-" else 1.0
    assert abs(abs(np.linalg.det(m)) - 1.0) < 1e-12, images
    return m


def axis_angle(axis, angle):
    """the rotation by `angle` rad about `axis` (Rodrigues' formula) -> float64 (3, 3)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def proper_permutations():
    """the 24 proper signed axis permutations -> [float64 (3, 3)]"""
    out = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            m = np.zeros((3, 3))
            for col in range(3):
                m[p[col], col] = -1.0 if signs >> col & 1 else 1.0
            if np.linalg.det(m) > 0:
                out.append(m)
    return out


OBLIQUE = axis_angle((1.0, 2.0, 3.0), 0.6)       # no rectangle stays axis-aligned, every slab a general plane, every horizon oblique

# name -> (scale, shift, rotation); the scale None: large_scale() of the generator
PLACEMENTS = {
    "identity": (1.0, (0.0, 0.0, 0.0), IDENTITY),
    "tiny": (1.0e-3, (0.0, 0.0, 0.0), IDENTITY),       # the reference's absolute constants (1e-3, 1e-9) are of the geometry's size
    "small": (1.0e-2, (0.0, 0.0, 0.0), IDENTITY),
    "large": (None, (0.0, 0.0, 0.0), IDENTITY),
    "shifted": (1.0, (250.0, -130.0, 40.0), IDENTITY),
    "shifted_far": (1.0, (1.0e4, -2.0e4, 5.0e3), IDENTITY),
    "small_far": (0.05, (3.0e4, 3.0e4, -3.0e4), IDENTITY),
    "x_up": (1.0, (0.0, 0.0, 0.0), permutation("y", "z", "x")),                    # z -> x, x -> y, y -> z
    "y_up_moved": (10.0, (-700.0, 300.0, 900.0), permutation("y", "z", "x") @ permutation("y", "z", "x")),   # x -> z ... z -> y
    "mirrored": (1.0, (40.0, 0.0, 0.0), permutation("-x", "y", "z")),
    "oblique": (3.0, (-90.0, 55.0, 20.0), OBLIQUE),
}
NAMES = tuple(PLACEMENTS)

def large_scale(generator, seed=None):
    """The scale of the "large" placement: the largest power of ten that keeps the generator's objects within the rays' reach
    of 65 535.  Fields, lattices and build_random reach 60 units from the origin: 100.  build_far_grazing's mirror wall is
    1e4 ... 6e4 away already: 1.  build_room(seed) is scaled by scene_gen.room_scale(seed) about the eye already: the largest
    power of ten with own scale x placement <= 1 000 (a room of 1 000 times 100 renders one colour, which tests nothing)."""
    if generator == "far":
        return 1.0
    if not generator.startswith("room"):
        return 100.0
    import scene_gen
    own, scale = scene_gen.room_scale(seed), 1.0
    while own * scale * 10.0 <= 1000.0 * (1.0 + 1e-6):
        scale *= 10.0
    return scale


def placement(name, generator="field", seed=None):
    """the catalogue's entry -> (scale, shift, rotation), "large" resolved for the generator"""
    scale, shift, rotation = PLACEMENTS[name]
    return (large_scale(generator, seed) if scale is None else scale), shift, rotation


def _f32(v):
    return tuple(float(F(c)) for c in v)


class Placed:
    """`scene` under p -> scale * rotation @ p + shift"""

    EYE, LOOK, UP = (0.0, -1.0, 2.5), (0.0, 0.0, 2.5), (0.0, 0.0, 1.0)        # Camera::setSceneTwoMirrors

    def __init__(self, scene, scale=1.0, shift=(0.0, 0.0, 0.0), rotation=IDENTITY):
        self.scene = scene
        self.scale = float(scale)
        self.shift = np.asarray(shift, dtype=np.float64)
        self.rotation = np.asarray(rotation, dtype=np.float64)
        self.identity = self.scale == 1.0 and not self.shift.any() and np.array_equal(self.rotation, IDENTITY)
        self.cam = None

    @classmethod
    def named(cls, scene, name, generator="field", seed=None):
        return cls(scene, *placement(name, generator, seed))

    # -- the map ---------------------------------------------------------------------------------------------------------------
    def point(self, p):
        if self.identity:
            return tuple(p)
        return _f32(self.scale * (self.rotation @ np.asarray(p, dtype=np.float64)) + self.shift)

    def direction(self, d):
        if self.identity:
            return tuple(d)
        return _f32(self.rotation @ np.asarray(d, dtype=np.float64))

    def length(self, l):
        if self.identity:
            return l
        return float(F(self.scale * float(l)))

    # -- the placing verbs -----------------------------------------------------------------------------------------------------
    def _done(self, out):
        self.put()
        return out

    def add_sphere(self, o, r):
        return self._done(self.scene.add_sphere(self.point(o), self.length(r)))

    def add_infinite_plane(self, o, n, h):
        return self._done(self.scene.add_infinite_plane(self.point(o), self.direction(n), self.direction(h)))

    def add_finite_plane_corners(self, o, vc, hc):
        return self._done(self.scene.add_finite_plane_corners(self.point(o), self.point(vc), self.point(hc)))

    def add_finite_plane_axes(self, o, n, h, vd, hd):
        return self._done(self.scene.add_finite_plane_axes(self.point(o), self.direction(n), self.direction(h), self.length(vd),
                                                           self.length(hd)))

    def set_checkerboard(self, i, light, dark, w, h):
        return self._done(self.scene.set_checkerboard(i, light, dark, self.length(w), self.length(h)))

    def camera_two_mirrors(self):
        self.scene.camera_two_mirrors()
        if not self.identity:
            self.cam = cameras.camera(self.point(self.EYE), self.point(self.LOOK), up=self.direction(self.UP),
                                      screen=(self.scale, self.scale), dist=self.scale)
            self.put()

    def put(self):
        """the placed camera onto the wrapped scene again (a HostScene flattens its own camera anew after every change)"""
        if self.cam is not None:
            if hasattr(self.scene, "cam"):
                cameras.put(self.cam, orc=self.scene)
            else:
                cameras.put(self.cam, host=self.scene)
        return self

    # -- everything else -------------------------------------------------------------------------------------------------------
    def __getattr__(self, name):
        attr = getattr(self.scene, name)
        if self.cam is None or not callable(attr) or not name.startswith("set_"):
            return attr
        return lambda *args, **kwargs: self._done(attr(*args, **kwargs))


def placed_pair(build, name, generator, seed, host_cls, orc_cls):
    """build(scene) on a fresh HostScene and a fresh OracleScene under the catalogue's placement `name` -> (host, orc, the
    host's Placed): the wrapped scenes themselves, the placed camera on both"""
    ph = Placed.named(host_cls.empty(), name, generator, seed)
    po = Placed.named(orc_cls(), name, generator, seed)
    build(ph)
    build(po)
    ph.put()
    po.put()
    return ph.scene, po.scene, ph


# ---- the scenes the placement tests place -------------------------------------------------------------------------------------

FAST_SCENES = (("room", 201), ("room", 203), ("room", 206), ("room", 210), ("random", 5), ("random", 9), ("far", 2), ("far", 4),
               ("room_eye", 210))       # room 210 with a half-mirror sphere around the eye: an item that gets the whole image
CLUSTERED_SCENES = (("field", 3), ("field", 7), ("field", 4), ("lattice", 12), ("lattice", 23))
FIELD_SPHERES = {3: 120, 7: 120, 4: 333, 10: 333, 11: 700}
# (generator, seed, placement) whose frame is inert -- the oracle's 64 x 48 depth-4 frame has fewer than 200 distinct colours,
# the count beside each -- and the seed of the same generator that is placed in its stead.  room 201 is a room of 0.01: at
# "tiny" it is 1e-5 units across, far below the reference's 1e-3 offset of plane hits; at "small_far" the screen's pixels are a
# fifth of a float's last place at 3e4 apart, and so are 201's walls and field 4's (333 spheres) few large near spheres.
REPLACED = {
    ("room", 201, "tiny"): 202,           # 3 colours; room 202 is a room of 1
    ("room", 201, "small_far"): 204,      # 118 colours; room 204 is a room of 0.3
    ("field", 4, "small_far"): 10,        # 133 colours; field 10 has 333 spheres too
}


# the counting build's cases: field 4 has 21 leaves (333 spheres in leaves of 16), field 11 has 35 (700 in leaves of 20) -- the
# SHADOW VOXELS are automatic from 24 leaves on (csrc/rt_tables.h: RT_SVOX_MIN_LEAVES)
ENGAGED_SCENES = (("field", 4), ("field", 11))
ENGAGED_PLACEMENTS = ("identity", "shifted_far", "x_up", "y_up_moved")


def gpu_cases(scenes, names=NAMES):
    """[(generator, seed, placement)] of `scenes` under `names`, the inert ones replaced"""
    return [(g, REPLACED.get((g, s, n), s), n) for g, s in scenes for n in names]


def builder(generator, seed):
    """the generator's scene `seed` as a function of the (wrapped) scene it is built on"""
    import scene_gen
    if generator == "room":
        return lambda s: scene_gen.build_room(s, seed)
    if generator == "room_eye":
        def room_eye(s):
            scene_gen.build_room(s, seed)
            i = s.add_sphere((0.0, -1.0, 2.5), scene_gen.f32(0.5 * scene_gen.room_scale(seed)))
            s.set_reflective(i, 0.5)
            s.set_diffuse(i, 0.5)
            return s
        return room_eye
    if generator == "random":
        return lambda s: scene_gen.build_random(s, seed)
    if generator == "far":
        return lambda s: scene_gen.build_far_grazing(s, seed)
    if generator == "field":
        return lambda s: scene_gen.build_sphere_field(s, seed, n_spheres=FIELD_SPHERES[seed])
    assert generator == "lattice", generator
    return lambda s: scene_gen.build_lattice(s, seed)
