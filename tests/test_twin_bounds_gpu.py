"""The bundle boxes of the twin tiles (csrc/rt_kernel.hip, wave_bounds3_twin()): the packed reduction must deliver every lane's
value of every ray to all six bounds.

One twin, 16 x 8 pixels (two tiles of 16 columns by 4 rows: option "tile_z" 4) at depth 1, over a mirror floor tilted 45
degrees to the view, with enough idle objects behind the eye that both scans cull by their bundle (RT_NEAR_CULL_MIN_ITEMS,
RT_SHADOW_CULL_MIN_ITEMS).  For each of the 128 (lane, ray)
positions of the twin, placed with the oracle's eye_ray:
  "direction": a small sphere on that pixel's reflected ray -- the level-1 nearest scan culls by the box of the directions;
  "point":     a small blocker between that pixel's shading point and the light -- the shadow scan culls by the box of the points.
Each over two floors: "full", where all 128 rays reach the floor and the boxes are the hulls of 128 values, and "patch", a
mirror no larger than that pixel's footprint, where the pixel's ray is the only one in use and each of the six bounds IS its
value: a reduction that loses the value of one lane position in one chain leaves an empty or a wrong box, culls the object and
changes the pixel.  Every frame is compared bit for bit with the CPU oracle's; the objects are checked (in float64) to be
missed by every camera ray, so that the pixel changes through the level-1 scan or the shadow scan alone."""
import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu

W, H = 16, 8
TWIN = b"rt_render_kernel"


def _unit(v):
    return v / np.linalg.norm(v)


class Layout:
    """the geometry every frame shares, from the default camera's rays"""

    def __init__(self, eye_ray):
        self.o = np.array(eye_ray(0.5, 0.5)[0], dtype=np.float64)
        dc = _unit(np.array(eye_ray(0.5, 0.5)[1], dtype=np.float64))
        up = np.array(eye_ray(0.5, 1.0)[1], dtype=np.float64) - np.array(eye_ray(0.5, 0.0)[1], dtype=np.float64)
        up = _unit(up - up.dot(dc) * dc)
        self.dc, self.n, self.a = dc, (up - dc) / np.sqrt(2.0), (up + dc) / np.sqrt(2.0)
        self.b = np.cross(self.n, self.a)
        self.F = self.o + 5.0 * dc                                   # the floor passes through here
        self.light = self.F + 4.0 * self.n + 2.0 * self.a
        self.d = np.array([[_unit(np.array(eye_ray(x / W, z / H)[1], dtype=np.float64)) for z in range(H)] for x in range(W)])
        t = (self.F - self.o).dot(self.n) / self.d.dot(self.n)
        self.P = self.o + t[..., None] * self.d                      # where each pixel's ray meets the floor
        self.r = self.d - 2.0 * self.d.dot(self.n)[..., None] * self.n
        flat = self.P.reshape(-1, 3)
        gaps = np.linalg.norm(flat[:, None] - flat[None], axis=-1) + np.eye(W * H) * 1e9
        self.gap = gaps.min(axis=1).reshape(W, H)                    # to the nearest other pixel's point

    def missed_by_camera_rays(self, centre, radius):
        v = centre - self.o
        along = self.d.dot(v)
        return (np.linalg.norm(v - along[..., None] * self.d, axis=-1) > 1.5 * radius).all()

    def build(self, s, floor, case, x, z):
        light = s.add_sphere(tuple(self.light), 0.1)
        s.set_light(light)
        for k in range(10):                                          # idle objects behind the eye: the culls have work
            i = s.add_sphere(tuple(self.o - 10.0 * self.dc + (k - 4.5) * self.b), 0.2)
            s.set_color(i, (0.2, 0.9, 0.3))
        if floor == "full":
            half_a = half_b = 20.0
            centre = self.F
        else:
            half_a = half_b = 0.3 * self.gap[x, z]
            centre = self.P[x, z]
        corner = centre - half_a * self.a - half_b * self.b
        i = s.add_finite_plane_corners(tuple(corner), tuple(corner + 2 * half_a * self.a), tuple(corner + 2 * half_b * self.b))
        s.set_reflective(i, 1.0)
        s.set_diffuse(i, 0.5)
        s.set_specular(i, 0.0)
        s.set_color(i, (0.9, 0.8, 0.7))
        if case == "direction":
            centre, radius = self.P[x, z] + 3.0 * self.r[x, z], 0.05
        elif case == "point":
            gap = self.gap[x, z]
            centre, radius = self.P[x, z] + 0.5 * gap * _unit(self.light - self.P[x, z]), 0.12 * gap
        if case != "base":
            assert self.missed_by_camera_rays(centre, radius), (case, x, z)
            i = s.add_sphere(tuple(centre), radius)
            s.set_color(i, (1.0, 0.1, 0.1))
        s.set_object_indices(0, 1)
        return s


@pytest.fixture(scope="module")
def layout(oracle):
    return Layout(oracle.OracleScene().eye_ray)


@pytest.fixture(scope="module")
def bases(oracle, layout):
    """the frames without the object: the full floor's, and each pixel's patch's"""
    full = layout.build(oracle.OracleScene(), "full", "base", 0, 0).render(W, H, 1)
    return {"full": lambda x, z: full, "patch": lambda x, z: layout.build(oracle.OracleScene(), "patch", "base", x, z).render(W, H, 1)}


@pytest.mark.parametrize("ray", [0, 1])
@pytest.mark.parametrize("case", ["direction", "point"])
@pytest.mark.parametrize("floor", ["full", "patch"])
def test_every_lane_reaches_the_box(oracle, layout, bases, floor, case, ray):
    """ray: the tile of the twin -- rows 0-3 are the lanes' first rays, rows 4-7 their second"""
    for x in range(W):
        for z in range(4 * ray, 4 * ray + 4):
            want = layout.build(oracle.OracleScene(), floor, case, x, z).render(W, H, 1)
            assert (want[x, z] != bases[floor](x, z)[x, z]).any(), f"{floor} {case} ({x}, {z}): the object changes nothing"
            r = Renderer(layout.build(HostScene.empty(), floor, case, x, z))
            r.set_option("tile_z", 4)
            got = r.render(W, H, 1)
            li = r.launch_info()
            assert li.kernel == TWIN and (li.tile_x, li.tile_z) == (16, 4)
            same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=-1)
            assert same.all(), f"{floor} {case} ({x}, {z}): pixels {np.argwhere(~same).tolist()} differ"
            r.close()
