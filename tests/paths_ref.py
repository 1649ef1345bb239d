"""The reference of include/rt_paths.h, for the tests: the header's definition restated in numpy fp32, one rounding per
operation, over the flat list of paths q = i S + s.  Nothing is derived a second time: bounce 0's rays are indirect_ref.rays of
the records, ray_{b+1} is indirect_ref.rays(g_b, 1, seed_b, key0 S) over the flat path list -- record q of that list samples with
key0 S + q = (key0 + i) S + s -- the colours are rays_ref.oracle_trace's and the records query_ref.intersect's (or the handle's
own ray batches and queries, for scenes the oracle does not cover), and the resolve is indirect_ref.resolve of the paths' sums.

RULES names the wrong rules of the mutation study (tests/test_paths_cpu.py); walk(..., rule=name) follows one of them."""
import functools

import numpy as np

import adaptive_frames
import ao_ref
import indirect_ref
import query_ref
import rays_ref

F = np.float32
GOLDEN = 0x9E3779B9
HIT_LIGHT, HIT_INSIDE = ao_ref.HIT_LIGHT, ao_ref.HIT_INSIDE
MAX_BOUNCES = 8
RULES = ("same_seed", "flat_key", "no_late_mask", "backward", "late_T", "no_flip", "dead_only")


def bounce_seed(seed, b):
    return (int(seed) + b * GOLDEN) & 0xFFFFFFFF


def oracle_tracer(orc, gather_depth):
    """-> f(rays (k, 6)) = (colours (k, 3), records (k,)) from the CPU oracle"""
    scene = query_ref.Scene(orc)

    def trace(rays):
        return rays_ref.oracle_trace(orc, rays, gather_depth), query_ref.intersect(scene, rays)
    return trace


def renderer_tracer(r, gather_depth):
    """-> the same from a Renderer's own rt_trace_rays and rt_intersect_rays (pinned by their own tests)"""
    def trace(rays):
        rays = np.ascontiguousarray(rays, dtype=F)
        if not len(rays):
            return np.zeros((0, 3), F), np.zeros(0, query_ref.HIT_DTYPE)
        return r.trace_rays(rays, gather_depth), r.intersect_rays(rays)
    return trace


def object_kd(g, kd):
    """kd(g.object): 0.0f for a miss and for an object the scene does not have"""
    obj = g["object"]
    k = np.zeros(len(g), dtype=F)
    known = (obj >= 0) & (obj < len(kd))
    k[known] = np.asarray(kd, dtype=F)[obj[known]]
    return k


class Walk:
    """the paths of a batch of records, bounce by bounce, as far as asked: per bounce b the colours (Q, 3) -- unmasked, zeros
    where the path is not alive --, whether the ray's first hit is a light (Q,), the throughput T_b (Q, 3) and alive_b (Q,).
    The walk depends on gain (a throughput of zero ends a path) and not on emitters or the base."""

    def __init__(self, trace, hits, n, kd, gain=1.0, seed=0, key0=0, rule=None, raygen=None):
        """raygen: None for indirect_ref.rays, or f(records (k,), n, seed, key0) -> rays (k, n n, 6): the library's
        rt_indirect_rays, where a test composes the public calls"""
        assert rule is None or rule in RULES, rule
        self.raygen = raygen or (lambda records, n, seed, key0: indirect_ref.rays(records, n, seed, key0)[0])
        self.trace, self.n, self.S, self.kd, self.gain, self.seed, self.key0, self.rule = trace, n, n * n, kd, F(gain), seed, key0, rule
        self.hits = np.ascontiguousarray(hits)
        flat = self.hits.reshape(-1)
        self.Q = len(flat) * self.S
        self.rays = np.array(self.raygen(flat, n, seed, key0), dtype=F).reshape(self.Q, 6)
        self.alive = [np.repeat(ao_ref.live_records(flat), self.S)]
        self.T = [np.ones((self.Q, 3), dtype=F)]
        self.colours, self.light, self.w = [], [], []
        self.g = None

    def extend(self, B):
        """trace bounces until B of them are known"""
        while len(self.colours) < B:
            b = len(self.colours)
            if b > 0:
                self._step(b - 1)
            alive = self.alive[b]
            colours = np.zeros((self.Q, 3), dtype=F)
            g = np.zeros(self.Q, dtype=query_ref.HIT_DTYPE)
            g["object"] = -1
            colours[alive], g[alive] = self.trace(self.rays[alive])
            self.colours.append(colours)
            self.light.append(alive & ((g["flags"] & HIT_LIGHT) != 0))
            self.g = g
        return self

    def _step(self, b):
        """from bounce b's records: T_{b+1}, alive_{b+1} and ray_{b+1}"""
        g, alive, rule = self.g, self.alive[b], self.rule
        with np.errstate(all="ignore"):
            w = (g["color"].astype(F) * object_kd(g, self.kd)[:, None]) * self.gain
            T = (self.T[b] * w).astype(F)
        self.w.append(w)
        ends = (g["object"] < 0) | ((g["flags"] & HIT_LIGHT) != 0) | (T == 0).all(axis=1)
        if rule == "late_T":                      # the decision sees the throughput before its multiplication
            ends = (g["object"] < 0) | ((g["flags"] & HIT_LIGHT) != 0) | (self.T[b] == 0).all(axis=1)
        if rule == "dead_only":                   # the records' own rule alone (a miss, a light): no throughput ends a path
            ends = (g["object"] < 0) | ((g["flags"] & HIT_LIGHT) != 0)
        nxt = alive & ~ends
        source = g
        if rule == "no_flip":
            source = g.copy()
            source["flags"] &= ~HIT_INSIDE
        seed = self.seed if rule == "same_seed" else bounce_seed(self.seed, b + 1)
        if rule == "flat_key":                    # key0 + q in place of (key0 + i) S + s
            key = int(self.key0)
        else:
            key = (int(self.key0) * self.S) & 0xFFFFFFFF
        rays = np.array(self.raygen(np.ascontiguousarray(source), 1, seed, key), dtype=F).reshape(self.Q, 6)
        rays[~nxt] = F(0)
        self.rays = rays
        self.T.append(np.where(nxt[:, None], T, F(0)).astype(F))
        self.alive.append(nxt)

    def counts(self, B):
        """alive[0 .. B-1]"""
        self.extend(B)
        return [int(a.sum()) for a in self.alive[:B]]

    def sums(self, B, emitters=False):
        """acc of every path after B bounces -> float32 (Q, 3)"""
        self.extend(B)
        rule = self.rule

        def colour(b):
            c = self.colours[b].copy()
            if not emitters and not (rule == "no_late_mask" and b >= 1):
                c[self.light[b]] = F(0)
            return c
        with np.errstate(all="ignore"):
            if rule == "backward":                # colour_b + w_b * rest, from the last bounce inwards
                rest = colour(B - 1)
                for b in range(B - 2, -1, -1):
                    rest = (colour(b) + np.where(self.alive[b + 1][:, None], self.w[b] * rest, F(0))).astype(F)
                return rest
            acc = colour(0)
            for b in range(1, B):
                acc = np.where(self.alive[b][:, None], acc + self.T[b] * colour(b), acc).astype(F)
        return acc

    def term(self, B, emitters=False, base=None):
        """rt_indirect_paths' output -> float32 hits.shape + (3,)"""
        acc = self.sums(B, emitters).reshape(self.hits.shape + (self.S, 3))
        return indirect_ref.resolve(acc, None, self.kd, self.hits, self.gain, base, emitters=True)


def paths(orc, hits, n, bounces, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False, base=None, kd=None, rule=None):
    """rt_indirect_paths of the records hits on the oracle scene orc -> (float32 hits.shape + (3,), alive[0 .. bounces-1])"""
    kd = indirect_ref.object_diffuse(orc) if kd is None else kd
    w = Walk(oracle_tracer(orc, gather_depth), hits, n, kd, gain, seed, key0, rule)
    return w.term(bounces, emitters, base), w.counts(bounces)


# ---- the frames compared with the CPU oracle: indirect_ref.FRAMES and EMITTER_FRAME, gain 1, each walked once ---------------------

@functools.lru_cache(maxsize=None)
def oracle_walk(frame, gain=1.0):
    """the Walk of a frame of indirect_ref.FRAMES on the CPU oracle; extend it as far as a test needs"""
    key, W, H, depth, n, seed, gather_depth = frame
    orc = adaptive_frames.oracle_scene(key)
    hits = indirect_ref.oracle_gather(*frame)[1]
    w = Walk(oracle_tracer(orc, gather_depth), hits, n, indirect_ref.object_diffuse(orc), gain, seed, 0)
    w.orc = orc                                   # (the tracer's scene lives as long as the walk)
    return w


def oracle_term(frame, bounces, emitters, with_base):
    rgb = indirect_ref.oracle_gather(*frame)[0]
    return oracle_walk(frame).term(bounces, emitters, rgb if with_base else None)


# The conditions (a test must not pass on a bounce that adds nothing): the share of the live records whose term differs between B
# and B + 1 bounces, emitters 0, no base, gain 1.  Measured on the CPU oracle:
#     builtin 0.834 0.834 0.832    random3 0.891 0.890 0.890    grid16 0.681 0.561 0.453
#     random2 0.432 0.215 0.051    twomirrors 0.215 0.036 0.023   (their paths leave the scene: compared bit for bit, no condition)
CONDITIONS = {"builtin": 3, "random3": 3, "grid16": 2}          # frame -> the steps B -> B + 1, from B = 1, that must hold 0.5
# alive[0..3] of every frame, and what it is without the zero-throughput stop
ALIVE = {"builtin": [20286, 17020, 14157, 12078], "grid16": [8252, 5299, 3563, 2363], "random2": [2488, 539, 178, 40],
         "twomirrors": [4388, 798, 90, 42], "random3": [4032, 3943, 3716, 3630]}


def differing_share(a, b, hits):
    """the share of the live records on which two terms differ in some word"""
    live = ao_ref.live_records(hits).reshape(np.shape(hits))
    differ = (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)
    return float(differ[live].mean())


def check_conditions(frame):
    key = frame[0]
    hits = indirect_ref.oracle_gather(*frame)[1]
    terms = [oracle_term(frame, B, False, False) for B in range(1, CONDITIONS[key] + 2)]
    for B in range(1, CONDITIONS[key] + 1):
        share = differing_share(terms[B - 1], terms[B], hits)
        assert share >= 0.5, (key, B, share)
