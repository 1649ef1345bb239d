"""One scene, three builders -- TEST INFRASTRUCTURE ONLY.

A Recorder takes the building verbs OracleScene and HostScene share, forwards them to an oracle scene and (optionally) a host
scene, and writes them down as a scene file: one verb per line, every float as the 8 hex digits of its bit pattern, so that
nothing is rounded on the way.  oracle/_ref/ref_harness (`make -C oracle ref`: a build of the reference itself, see
oracle/Makefile) builds the same scene through the reference's public API from that file; run_reference() starts it as a child
process.  load_scene() rebuilds an OracleScene or a HostScene from a committed scene file.  One more verb exists in scene
files only, `grid N SHADOWS`: build_grid()'s verbs in one line, expanded before the reference sees it.

Also here, because the fixtures' generator (golden/make_ref_pins.py), the CPU pins and the GPU pins must agree on them: the
named scenes, the ray and segment batches, and the cases of the digest sweep.  Nothing here needs the reference's sources or
its binary except run_reference()."""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

import oracle_lib
import scene_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BINARY = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
REFERENCE_DIR = os.environ.get("REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_REF = os.path.join(GOLDEN, "ref")
F = np.float32
HIT_DTYPE = np.dtype([("object", "<i4"), ("distance", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)),
                      ("color", "<f4", (3,)), ("flags", "<i4")])
MAX_FIXTURE_BYTES = 49152
if ROOT not in sys.path:          # the product package (HostScene), for a script that is started outside pytest
    sys.path.insert(0, ROOT)


def _host_scene():
    """HostScene, imported when first wanted"""
    from tilecoderaytracer_amd import HostScene
    return HostScene


def have_binary():
    return os.path.exists(REF_BINARY)


def have_reference():
    return os.path.isdir(os.path.join(REFERENCE_DIR, "src"))


def fhex(x):
    return struct.pack("<f", float(x))[::-1].hex()


def unhex(t):
    return struct.unpack("<f", bytes.fromhex(t)[::-1])[0]


# ---- the recorder ---------------------------------------------------------------------------------------------------------------

class Recorder:
    """The shared verbs, forwarded to `oracle` (an OracleScene, made if None) and `host` (a HostScene or None) and written down.
    scene_gen's builders and the tests' own take it in place of either."""

    def __init__(self, oracle=None, host=None):
        self.oracle = oracle_lib.OracleScene() if oracle is None else oracle
        self.host = host
        self.lines = []
        self.short = None          # a one-line form of the whole scene ("grid N SHADOWS"), written in place of the lines

    @classmethod
    def named(cls, name, host=False):
        """'builtin' | 'twomirrors': the reference's own scenes, one verb each"""
        self = cls(oracle_lib.OracleScene.named(name), _host_scene().named(name) if host else None)
        self.lines.append(name)
        return self

    def _both(self, verb, *args):
        out = getattr(self.oracle, verb)(*args)
        if self.host is not None:
            other = getattr(self.host, verb)(*args)
            assert other == out or out is None, (verb, out, other)
        return out

    def _line(self, verb, *fields):
        words = [verb]
        for f in fields:
            if isinstance(f, (tuple, list, np.ndarray)):
                words += [fhex(c) for c in f]
            elif isinstance(f, (int, np.integer)) and not isinstance(f, bool):
                words.append(str(int(f)))
            else:
                words.append(fhex(f))
        self.lines.append(" ".join(words))

    def add_sphere(self, o, r):
        self._line("S", o, float(r))
        return self._both("add_sphere", o, r)

    def add_infinite_plane(self, o, n, h):
        self._line("I", o, n, h)
        return self._both("add_infinite_plane", o, n, h)

    def add_finite_plane_corners(self, o, vc, hc):
        self._line("C", o, vc, hc)
        return self._both("add_finite_plane_corners", o, vc, hc)

    def add_finite_plane_axes(self, o, n, h, vd, hd):
        self._line("A", o, n, h, float(vd), float(hd))
        return self._both("add_finite_plane_axes", o, n, h, vd, hd)

    def set_color(self, i, c):
        self._line("color", int(i), c)
        self._both("set_color", i, c)

    def set_diffuse(self, i, f):
        self._line("diffuse", int(i), float(f))
        self._both("set_diffuse", i, f)

    def set_specular(self, i, f):
        self._line("specular", int(i), float(f))
        self._both("set_specular", i, f)

    def set_reflective(self, i, f):
        self._line("reflective", int(i), float(f))
        self._both("set_reflective", i, f)

    def set_checkerboard(self, i, light, dark, w, h):
        self._line("checker", int(i), light, dark, float(w), float(h))
        self._both("set_checkerboard", i, light, dark, w, h)

    def set_light(self, i):
        self._line("light", int(i))
        self._both("set_light", i)

    def set_intensity(self, i, f):
        self._line("intensity", int(i), float(f))
        self._both("set_intensity", i, f)

    def set_object_indices(self, rank, size):
        self._line("indices", int(rank), int(size))
        self._both("set_object_indices", rank, size)

    def camera_two_mirrors(self):
        self._line("cam2")
        self._both("camera_two_mirrors")

    @property
    def object_count(self):
        return self.oracle.object_count

    def text(self, expanded=False):
        """the scene file: the recorded verbs, or the scene's one-line form if it has one and expanded is false"""
        return "\n".join(self.lines if expanded or self.short is None else [self.short]) + "\n"

    def write(self, path, expanded=False):
        with open(path, "w") as f:
            f.write(self.text(expanded))
        return path


def load_scene(path, host=False):
    """The scene of a scene file as an OracleScene, or as a HostScene (host=True)"""
    if host:
        named, empty = _host_scene().named, _host_scene().empty
    else:
        named, empty = oracle_lib.OracleScene.named, oracle_lib.OracleScene
    scene = None
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            verb, a = w[0], w[1:]
            if verb in ("builtin", "twomirrors"):
                assert scene is None, "a whole scene must come first"
                scene = named(verb)
                continue
            if scene is None:
                scene = empty()
            if verb == "grid":
                build_grid(scene, int(a[0]), bool(int(a[1])))
                continue
            fl = lambda k: unhex(a[k])
            v = lambda k: (unhex(a[k]), unhex(a[k + 1]), unhex(a[k + 2]))
            if verb == "S":
                scene.add_sphere(v(0), fl(3))
            elif verb == "I":
                scene.add_infinite_plane(v(0), v(3), v(6))
            elif verb == "C":
                scene.add_finite_plane_corners(v(0), v(3), v(6))
            elif verb == "A":
                scene.add_finite_plane_axes(v(0), v(3), v(6), fl(9), fl(10))
            elif verb == "color":
                scene.set_color(int(a[0]), v(1))
            elif verb == "diffuse":
                scene.set_diffuse(int(a[0]), fl(1))
            elif verb == "specular":
                scene.set_specular(int(a[0]), fl(1))
            elif verb == "reflective":
                scene.set_reflective(int(a[0]), fl(1))
            elif verb == "checker":
                scene.set_checkerboard(int(a[0]), v(1), v(4), fl(7), fl(8))
            elif verb == "light":
                scene.set_light(int(a[0]))
            elif verb == "intensity":
                scene.set_intensity(int(a[0]), fl(1))
            elif verb == "indices":
                scene.set_object_indices(int(a[0]), int(a[1]))
            elif verb == "cam2":
                scene.camera_two_mirrors()
            else:
                raise ValueError(f"{path}: unknown verb {verb!r}")
    return empty() if scene is None else scene


# ---- the reference binary -------------------------------------------------------------------------------------------------------

class ReferenceFailed(RuntimeError):
    pass


def run_reference(scene_file, W=1, H=1, depth=0, mode=None, rays=None, timeout=300):
    """oracle/_ref/ref_harness as a child process -> (what it wrote, the number of "FAILURE" diagnostics the reference printed).
    No mode: the W x H frame, float32 (W, H, 3).  mode 'trace' | 'hits' | 'occluded' with rays float32 (n, 6): float32 (n, 3) |
    HIT_DTYPE (n,) | bool (n,).  Raises ReferenceFailed on a crash, a non-zero exit or a timeout."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.bin")
        text = open(scene_file).read()
        if text.startswith("grid "):           # the harness knows primitive verbs only
            n, shadows = text.split()[1:3]
            scene_file = build_grid(Recorder(), int(n), bool(int(shadows))).write(os.path.join(tmp, "grid.scene"), expanded=True)
        cmd = [REF_BINARY, scene_file, str(W), str(H), str(depth), out]
        if mode is not None:
            rays_file = os.path.join(tmp, "rays.f32")
            np.ascontiguousarray(rays, dtype=F).reshape(-1, 6).tofile(rays_file)
            cmd += [mode, rays_file]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
        except subprocess.TimeoutExpired:
            raise ReferenceFailed(f"timeout after {timeout} s: {' '.join(cmd)}")
        if r.returncode != 0:
            raise ReferenceFailed(f"exit {r.returncode}: {' '.join(cmd)}: {r.stderr.decode(errors='replace')[-300:]}")
        last = r.stdout.decode().split()
        failures = int(last[-1]) if len(last) >= 2 and last[-2] == "failures" else -1
        raw = open(out, "rb").read()
    if mode is None:
        return np.frombuffer(raw, dtype=F).reshape(W, H, 3).copy(), failures
    if mode == "trace":
        return np.frombuffer(raw, dtype=F).reshape(-1, 3).copy(), failures
    if mode == "hits":
        return np.frombuffer(raw, dtype=HIT_DTYPE).copy(), failures
    return np.frombuffer(raw, dtype=np.uint8).astype(bool), failures


def run_reference_text(text, *args, **kw):
    """run_reference on a scene given as text"""
    with tempfile.NamedTemporaryFile("w", suffix=".scene", delete=False) as f:
        f.write(text)
    try:
        return run_reference(f.name, *args, **kw)
    finally:
        os.unlink(f.name)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

GRID_PALETTE = [(1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 1, 1)]


def build_grid(scene, n, shadows):
    """The synthetic grid-n scene of SURVEY.md Appendix E through the shared verbs (orc_scene_grid and HostScene.grid build it
    natively; test_reference_pins_cpu.py asserts the three equal), so that it can go to the reference through its public API,
    shadow range included."""
    half, step = F(0.5), F(2.5)
    i = scene.add_sphere((-20.0, 10.0, 10.0), float(F(.15)))
    scene.set_light(i)
    scene.set_intensity(i, float(F(.75)))
    i = scene.add_sphere((0.0, 40.0, 11.0), float(F(.15)))
    scene.set_light(i)
    scene.set_intensity(i, 1.0)
    for a in range(n):
        for b in range(n):
            cx = (F(a) - F(n - 1) * half) * step
            cy = F(6.0) + F(b) * step
            i = scene.add_sphere((float(cx), float(cy), 1.0), 1.0)
            scene.set_color(i, GRID_PALETTE[(a * n + b) % 6])
            if (a + b) % 2 == 0:
                scene.set_reflective(i, 1.0)
                scene.set_diffuse(i, 0.0)
            else:
                scene.set_specular(i, 0.5)
    i = scene.add_infinite_plane((0, 0, 0), (0, 0, 1), (1, 0, 0))
    scene.set_color(i, (0, 1, 0))
    scene.set_reflective(i, 0.5)
    scene.set_diffuse(i, 0.5)
    scene.set_checkerboard(i, (1, 1, 1), (0, 0, 0), 3.0, 3.0)
    i = scene.add_infinite_plane((0, 0, 12), (0, 0, -1), (1, 0, 0))
    light_grey = float(F(2) / F(3))
    scene.set_color(i, (light_grey, light_grey, light_grey))
    scene.set_reflective(i, 0.5)
    scene.set_specular(i, 0.5)
    if shadows:
        scene.set_object_indices(0, 1)
    scene.camera_two_mirrors()
    if isinstance(scene, Recorder):
        scene.short = f"grid {n} {int(bool(shadows))}"        # 1 028 objects as verbs would be a 110 KB file
    return scene


def build_degenerate(s):
    """test_parity_gpu.test_degenerate_geometry's scene"""
    i = s.add_sphere((3.0, 5.0, 8.0), 0.15)
    s.set_light(i)
    s.add_sphere((0.0, 6.0, 1.0), 0.0)
    s.add_sphere((1.0, 6.0, 1.0), -1.0)
    s.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    s.add_finite_plane_axes((0.0, 8.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 0.0, 3.0)
    i = s.add_infinite_plane((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    s.set_reflective(i, 0.5)
    i = s.add_sphere((0.0, -1.0, 2.5), 3.0)
    s.set_reflective(i, 1.0)
    s.set_object_indices(0, 1)
    s.camera_two_mirrors()
    return s


CHECKER_SIZES = [(3.0, 3.0), (0.3, 7.7), (1.0e-3, 2.5), (1.0e5, 0.75), (2.0 ** -110, 1.0), (1.0, 2.0 ** 101), (0.0, 1.0), (-2.0, 3.0)]


def build_checkerboard(s, width, height):
    """test_parity_gpu.test_checkerboard_coordinates' scene (the built-in camera)"""
    i = s.add_sphere((2.0, -3.0, 9.0), 0.15)
    s.set_light(i)
    g = s.add_infinite_plane((0.3, 0.1, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    s.set_checkerboard(g, (1.0, 1.0, 1.0), (0.0, 0.0, 0.25), width, height)
    s.set_reflective(g, 0.25)
    k = s.add_sphere((0.5, 6.0, 0.5), 1.5)
    s.set_reflective(k, 1.0)
    s.set_object_indices(0, 1)
    return s


def build_facing_mirrors(s):
    """test_parity_gpu.test_facing_mirrors_depth_400's scene"""
    i = s.add_sphere((3.0, 5.0, 8.0), 0.15)
    s.set_light(i)
    a = s.add_finite_plane_axes((-4.0, 9.0, -1.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 8.0, 8.0)
    b = s.add_finite_plane_axes((4.0, -3.0, -1.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), 8.0, 8.0)
    for m in (a, b):
        s.set_reflective(m, 1.0)
        s.set_diffuse(m, 0.0)
    k = s.add_sphere((0.5, 3.0, 2.0), 0.7)
    s.set_color(k, (1, 0, 0))
    s.set_object_indices(0, 1)
    s.camera_two_mirrors()
    return s


def build_edges(s):
    """A level rectangle z = 0 over [-2, 2]^2 whose hit parameter for a ray straight down from (x, y, z) is z itself, bit for
    bit (normal (0, 0, 1), distance_to_origin -0.0, direction (0, 0, -1)): edge_rays() walks z through the floats around
    the finite plane's threshold 1E-5, which the reference compares in double.  Below it a sphere and a floor that such a ray
    reaches when the rectangle lets it through; the built-in camera."""
    i = s.add_sphere((2.0, 3.0, 6.0), 0.15)
    s.set_light(i)
    i = s.add_finite_plane_axes((-2.0, -2.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 4.0, 4.0)
    s.set_color(i, (1, 0, 0))
    s.set_reflective(i, 0.5)
    i = s.add_sphere((0.0, 0.0, -1.0), 0.5)
    s.set_color(i, (0, 0, 1))
    i = s.add_infinite_plane((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    s.set_color(i, (0, 1, 0))
    s.set_checkerboard(i, (1, 1, 1), (0, 0, 0), 1.0, 1.0)
    s.set_object_indices(0, 1)
    return s


def edge_rays(seed, down):
    """136 rays from heights z = the float 1E-5 and its 8 neighbours either way, at 8 places over build_edges' rectangle,
    straight down by `down`: the rectangle's t is z, and |T - E| is `down`"""
    rng = np.random.RandomState(seed)
    z = F(1e-5)
    below = [z]
    for _ in range(8):
        below.append(np.nextafter(below[-1], F(0)))
    above = [z]
    for _ in range(8):
        above.append(np.nextafter(above[-1], F(1)))
    heights = np.array(below[:0:-1] + above, dtype=F)
    assert len(heights) == 17 and heights[8] == z
    rows = []
    for x, y in rng.uniform(-1.9, 1.9, (8, 2)).astype(F):
        for h in heights:
            rows.append([x, y, h, x, y, F(h) - F(down)])
    return np.array(rows, dtype=F)


def _adversarial(s, seed):
    from test_parity_gpu import _adversarial as build
    return build(s, seed)


def _nested(s):
    from test_parity_gpu import _nested_spheres as build
    return build(s)


def _named(name):
    return lambda host=False: Recorder.named(name, host)


def _built(build, *args):
    def make(host=False):
        rec = Recorder(host=_host_scene().empty() if host else None)
        build(rec, *args)
        return rec
    return make


# the committed frames: key -> (recorder factory, W, H, depth, where the frame lives).  The first three are the survey's
# fixtures, which the reference binary must reproduce byte for byte where they lie.
FRAMES = {
    "b64d4": (_named("builtin"), 64, 64, 4, GOLDEN),
    "g32_64d4": (_built(build_grid, 32, False), 64, 64, 4, GOLDEN),
    "g16_64d8": (_built(build_grid, 16, False), 64, 64, 8, GOLDEN),
    "grid32_64d4": (_built(build_grid, 32, True), 64, 64, 4, GOLDEN_REF),
    "grid16_64d8": (_built(build_grid, 16, True), 64, 64, 8, GOLDEN_REF),
    "twomirrors_64d6": (_named("twomirrors"), 64, 64, 6, GOLDEN_REF),
    "adversarial21_64d5": (_built(_adversarial, 21), 64, 64, 5, GOLDEN_REF),
    "adversarial22_64d5": (_built(_adversarial, 22), 64, 64, 5, GOLDEN_REF),          # SetObjectIndices(1, 3): a partial shadow range
    "room206_64d5": (_built(scene_gen.build_room, 206), 64, 64, 5, GOLDEN_REF),
    "grazing7001_64d3": (_built(scene_gen.build_far_grazing, 7001), 64, 64, 3, GOLDEN_REF),
    "field7_64d3": (_built(scene_gen.build_sphere_field, 7), 64, 64, 3, GOLDEN_REF),
    "degenerate_48x40d4": (_built(build_degenerate), 48, 40, 4, GOLDEN_REF),
    "nested_64d5": (_built(_nested), 64, 64, 5, GOLDEN_REF),
    "edges_32d3": (_built(build_edges), 32, 32, 3, GOLDEN_REF),
}
# the scenes that also carry ray and segment batches: key -> the frame whose scene file they use
BATCHES = {"builtin": "b64d4", "field7": "field7_64d3", "room206": "room206_64d5", "adversarial21": "adversarial21_64d5",
           "edges": "edges_32d3"}
BATCH_RAYS = 1024
BATCH_DEPTH = 3
GRID = (24, 20)          # the first GRID[0] * GRID[1] rays of a batch are this frame's camera rays in pixels[x][z] order


def scene_path(key):
    return os.path.join(GOLDEN_REF, key + ".scene")


def frame_path(key):
    return os.path.join(FRAMES[key][4], key + ".f32")


def batch_path(name, what):
    """what: rays.f32 | hits.bin | colours.f32 | segs.f32 | verdicts.u8"""
    return os.path.join(GOLDEN_REF, f"{name}.{what}")


def load_batch(name):
    """-> (rays (n, 6), the reference's records, its depth-BATCH_DEPTH colours, segments (n, 6), its verdicts)"""
    rays = np.fromfile(batch_path(name, "rays.f32"), dtype=F).reshape(-1, 6)
    hits = np.fromfile(batch_path(name, "hits.bin"), dtype=HIT_DTYPE)
    colours = np.fromfile(batch_path(name, "colours.f32"), dtype=F).reshape(-1, 3)
    segs = np.fromfile(batch_path(name, "segs.f32"), dtype=F).reshape(-1, 6)
    verdicts = np.fromfile(batch_path(name, "verdicts.u8"), dtype=np.uint8).astype(bool)
    assert len(rays) == len(hits) == len(colours) == len(segs) == len(verdicts) == BATCH_RAYS
    return rays, hits, colours, segs, verdicts


# ---- ray and segment batches ----------------------------------------------------------------------------------------------------

def _spheres_and_planes(oscene):
    objs = [oscene.get_object(i) for i in range(oscene.object_count)]
    return [o for o in objs if o.kind == 0], [o for o in objs if o.kind != 0], [o for o in objs if o.is_light]


def ray_batch(oscene, seed, n=BATCH_RAYS, grid=GRID):
    """n rays {E, T} for a scene: the camera rays of a grid[0] x grid[1] frame in pixels[x][z] order (a G-buffer frame of that
    size has their records), 16 rays from around the eye at the lights' centres, camera rays of a 40 x 36 frame in a shuffled order, rays that start inside spheres (anywhere in
    the ball, any direction) and rays that start on planes (at the plane, both ways, some grazing).  No -0.0 among the targets
    (rays_ref.positive_zeros: the oracle's camera route adds +0.0 to them)."""
    from rays_ref import camera_rays, positive_zeros
    rng = np.random.RandomState(seed)
    spheres, planes, lights = _spheres_and_planes(oscene)
    parts = [camera_rays(oscene.cam, grid[0], grid[1]).reshape(-1, 6)]
    cam = camera_rays(oscene.cam, 40, 36).reshape(-1, 6)
    if lights:                                  # from around the eye straight at the lights: records with hitALightSource set
        L = np.array([o.origin.tuple() for o in lights], dtype=F)[rng.randint(len(lights), size=16)]
        E = (cam[0, :3] + rng.uniform(-0.5, 0.5, (16, 3)).astype(F)).astype(F)
        parts.append(np.concatenate([E, L], axis=1))
    rest = n - sum(len(p) for p in parts)
    n_inside = rest // 4 if spheres else 0
    n_plane = rest // 4 if planes else 0
    parts.append(cam[rng.permutation(len(cam))[:rest - n_inside - n_plane]])
    if n_inside:
        pick = rng.randint(len(spheres), size=n_inside)
        c = np.array([spheres[k].origin.tuple() for k in pick], dtype=F)
        r = np.array([spheres[k].radius for k in pick], dtype=F)[:, None]
        E = (c + rng.uniform(-0.55, 0.55, (n_inside, 3)).astype(F) * r).astype(F)
        parts.append(np.concatenate([E, (E + rng.normal(size=(n_inside, 3)).astype(F)).astype(F)], axis=1))
    if n_plane:
        pick = rng.randint(len(planes), size=n_plane)
        rows = []
        for k in pick:
            o = planes[k]
            po = np.array((o.plane_origin if o.kind == 2 else o.origin).tuple(), dtype=F)
            hz, vt, nm = (np.array(v.tuple(), dtype=F) for v in (o.horizontal, o.vertical, o.normal))
            hd, vd = (F(o.h_distance), F(o.v_distance)) if o.kind == 2 else (F(8), F(8))
            E = po + hz * F(rng.uniform(-0.1, 1.1) * hd) + vt * F(rng.uniform(-0.1, 1.1) * vd)
            T = E + nm * F(rng.choice([-1.0, 1.0, 0.01, -0.01])) + rng.uniform(-0.7, 0.7, 3).astype(F)
            rows.append(np.concatenate([E, T]).astype(F))
        parts.append(np.nan_to_num(np.array(rows, dtype=F), nan=0.5, posinf=1e4, neginf=-1e4))
    rays = np.ascontiguousarray(np.concatenate(parts).astype(F))
    assert rays.shape == (n, 6)
    return positive_zeros(rays)


def segment_batch(oscene, hits, seed, n=BATCH_RAYS):
    """n segments {E, T} from the reference's records `hits` of a ray batch: hit point -> a light's centre, hit point -> a point
    near it, and points inside spheres -> a light's centre."""
    rng = np.random.RandomState(seed)
    spheres, _, lights = _spheres_and_planes(oscene)
    L = np.array([o.origin.tuple() for o in lights], dtype=F)
    P = hits["point"][hits["object"] >= 0]
    P = P[np.isfinite(P).all(axis=1)]
    assert len(P) and len(L)
    n_inside = n // 8 if spheres else 0
    k = n - n_inside
    E = P[rng.randint(len(P), size=k)]
    T = L[rng.randint(len(L), size=k)].copy()
    near = rng.rand(k) < 0.5
    T[near] = (T[near] + rng.uniform(-1.5, 1.5, (int(near.sum()), 3)).astype(F)).astype(F)
    parts = [np.concatenate([E, T], axis=1)]
    if n_inside:
        pick = rng.randint(len(spheres), size=n_inside)
        c = np.array([spheres[j].origin.tuple() for j in pick], dtype=F)
        r = np.array([spheres[j].radius for j in pick], dtype=F)[:, None]
        E = (c + rng.uniform(-0.55, 0.55, (n_inside, 3)).astype(F) * r).astype(F)
        parts.append(np.concatenate([E, L[rng.randint(len(L), size=n_inside)]], axis=1))
    segs = np.ascontiguousarray(np.concatenate(parts).astype(F))
    assert segs.shape == (n, 6)
    return segs


def batch_rays(name, oscene, seed):
    """the rays of batch `name`; the edges scene's end with edge_rays()"""
    rays = ray_batch(oscene, seed)
    if name == "edges":
        edge = edge_rays(seed, 1.0)
        rays[-len(edge):] = edge
    return rays


def batch_segments(name, oscene, hits, seed):
    """the segments of batch `name` from the reference's records of its rays; the edges scene's end with edge_rays() that stop
    above the sphere"""
    segs = segment_batch(oscene, hits, seed)
    if name == "edges":
        edge = edge_rays(seed + 1, 0.25)
        segs[-len(edge):] = edge
    return segs


# ---- the digest sweep -----------------------------------------------------------------------------------------------------------

GENERATORS = {"random": scene_gen.build_random, "field": scene_gen.build_sphere_field, "room": scene_gen.build_room,
              "grazing": scene_gen.build_far_grazing}
SWEEP_DEPTHS = (0, 1, 3, 6, 12)
SWEEP_SEEDS = range(1000, 1060)          # committed in digests.json
LIVE_SEEDS = range(2000, 2040)           # fresh: run against the binary where it exists
SWEEP_SIZE = (40, 36)


def sweep_cases():
    """every case of golden/ref/digests.json: [(id, recorder factory, W, H, depth, is a fuzz seed)]"""
    out = []
    for g, build in GENERATORS.items():
        for k, seed in enumerate(SWEEP_SEEDS):
            out.append((f"{g}_{seed}", _built(build, seed), *SWEEP_SIZE, SWEEP_DEPTHS[k % len(SWEEP_DEPTHS)], True))
    for seed in list(range(20, 32)) + [77]:
        W, H, depth = (80, 48, 4) if seed == 77 else (96, 64, 5)
        out.append((f"adversarial_{seed}", _built(_adversarial, seed), W, H, depth, False))
    for k, (w, h) in enumerate(CHECKER_SIZES):
        out.append((f"checkerboard_{k}", _built(build_checkerboard, w, h), 96, 64, 3, False))
    out.append(("facing_mirrors_d400", _built(build_facing_mirrors), 24, 20, 400, False))
    out.append(("builtin_500x504_d50", _named("builtin"), 500, 504, 50, False))
    for name, n, W, depth in (("grid32", 32, 64, 4), ("grid32", 32, 256, 4), ("grid16", 16, 64, 8), ("grid16", 16, 256, 8)):
        out.append((f"{name}_{W}x{W}_d{depth}", _built(build_grid, n, True), W, W, depth, False))
    out.append(("twomirrors_48x48_d6", _named("twomirrors"), 48, 48, 6, False))
    return out


SWEEP_MIN_CASES = 4 * 60 + 13 + 8 + 1 + 1 + 4 + 1
MAX_EXCLUDED_SEEDS = int(0.02 * 4 * 60)          # 2 % of the sweep's seeds; named scenes: none


def load_digests():
    with open(os.path.join(GOLDEN_REF, "digests.json")) as f:
        return json.load(f)


def count_nans(a):
    return int(np.isnan(a).sum())


def same_bits(a, b):
    """elementwise: equal bit patterns, or both NaN (payload bits are not portable)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def records_same(got, want):
    """per record: every field equal by bits, float fields NaN-aware"""
    g = np.ascontiguousarray(got, dtype=HIT_DTYPE).reshape(-1).view(np.uint32).reshape(-1, 12)
    w = np.ascontiguousarray(want, dtype=HIT_DTYPE).reshape(-1).view(np.uint32).reshape(-1, 12)
    nan = np.isnan(g.view(F)) & np.isnan(w.view(F))
    nan[:, 0] = nan[:, 11] = False
    return ((g == w) | nan).all(axis=1)
