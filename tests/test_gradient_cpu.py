"""Temporal-gradient weights for an accumulated history (include/rt_gradient.h) without a GPU: the header, the exported symbols,
every argument check in the header's order (none touches a device), gradient_ref -- the tests' restatement of the definition --
against a per-pixel restatement in np.float32 scalars, each line of the header's WHAT FOLLOWS on the reference, the conditions
on the ghost pixels of two pose pairs of the motion scene, counted with the reference on the oracle's colours and records, and
gradient_edges.py's edge inputs: the reference against the scalar restatement on each, and the restatement with one line changed
against the reference -- the condition that those inputs can tell a kernel with that line from the header's."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cameras
import clamp_ref
import gradient_edges
import gradient_ref
import motion_scenes
from clamp_scenes import GHOST_KW, GHOST_PAIRS, ghost_error, ghost_setting
from denoise_ref import same_bits
from gradient_edges import made_up_inputs
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_gradient.h")
FUNCTIONS = ["rt_capi_gradient_version", "rt_gradient_reweight", "rt_gradient_reweight_device"]
F = np.float32
NAMES = gradient_ref.NAMES


def same_words(got, want, what):
    """bit for bit"""
    for g, w, name in zip(got, want, NAMES):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {name}"


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t)\s+(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["rt_capi_query.h"]
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    lines = [line.split() for line in r.stdout.splitlines() if line.split()]
    exported = sorted(p[-1] for p in lines if p[-2] == "T" and re.fullmatch(r"rt_\w*gradient\w*", p[-1]))
    assert exported == FUNCTIONS                              # and nothing else of this unit: the library has one kernel form
    assert int(re.search(r"#define RT_CAPI_GRADIENT_VERSION (\d+)", text).group(1)) == lib.rt_capi_gradient_version() == 1
    assert C.sizeof(capi.RtGradientParams) == 32
    assert "rt_gradient.h" in open(os.path.join(INCLUDE, "rt_clamp.h")).read()       # the clamp's "Not provided" points here


def test_header_is_plain_c99_with_every_other_header_and_the_struct_is_32_bytes(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert "rt_gradient.h" in others and len(others) >= 25
    for first in ('#include "rt_gradient.h"\n', ""):             # on its own before every other header, and among them
        src = tmp_path / "gradient.c"
        src.write_text(first + "".join(f'#include "{h}"\n' for h in others) +
                       "#include <stddef.h>\n"
                       "int main(void) { rt_gradient_params p = {3, 2, 1, 1, 0.9f, 2.0f, 0.0f, 1e-6f};\n"
                       "  return (RT_CAPI_GRADIENT_VERSION == 1 && sizeof p == 32 && offsetof(rt_gradient_params, match_color) == 12\n"
                       "          && offsetof(rt_gradient_params, normal_cos) == 16 && offsetof(rt_gradient_params, den_floor) == 28\n"
                       "          && p.gain == 2.0f) ? 0 : 1; }\n")
        exe = tmp_path / "gradient"
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

P = capi.RtGradientParams
GOOD = (3, 2, 1, 1, 0.9, 2.0, 0.0, 1e-6)
NAN, INF = float("nan"), float("inf")
UP = float(np.nextafter(F(1), F(2)))                            # the first float above 1
DOWN = float(np.nextafter(F(-1), F(-2)))
TINY = float(np.nextafter(F(0), F(-1)))                         # the first float below 0
# each bad value -- the first refused one on either side of its range -- with every later field bad too, and the word of the
# message that names the first
BAD_PARAMS = [((c, 1, 3, 2, NAN, -1.0, 2.0, -1.0), "channels") for c in (0, 2, 4)]
BAD_PARAMS += [((3, s, 3, 2, NAN, -1.0, 2.0, -1.0), "scale") for s in (1, 9, 0, -2)]
BAD_PARAMS += [((1, 2, r, 2, NAN, -1.0, 2.0, -1.0), "radius") for r in (-1, 3)]
BAD_PARAMS += [((3, 8, 0, m, NAN, -1.0, 2.0, -1.0), "match_color") for m in (-1, 2)]
BAD_PARAMS += [((3, 8, 2, 0, v, -1.0, 2.0, -1.0), "normal_cos") for v in (NAN, UP, DOWN, INF)]
BAD_PARAMS += [((3, 2, 2, 1, 1.0, v, 2.0, -1.0), "gain") for v in (TINY, NAN, INF)]
BAD_PARAMS += [((3, 2, 2, 1, -1.0, 0.0, v, -1.0), "lambda_min") for v in (TINY, NAN, UP, INF)]
BAD_PARAMS += [((3, 2, 2, 1, -1.0, 0.0, 1.0, v), "den_floor") for v in (TINY, NAN, INF)]
# the last admitted values of every range
EDGE_PARAMS = [(1, 2, 0, 0, -1.0, 0.0, 0.0, 0.0), (3, 8, 2, 1, 1.0, 3e38, 1.0, 3e38), (3, 3, 1, 1, -0.0, 1e-45, 1e-45, 1e-45)]

# fake addresses: no check dereferences one.  cur, hits, value, moments, len, now_lo, then_lo, lo_hits, then_hits, then the six
# outputs, the flags on a byte
INPUTS = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000)
OUTPUTS = (0xA00000, 0xB00000, 0xC00000, 0xD00000, 0xE00000, 0xF00001)
ALL = INPUTS + OUTPUTS
WORDS = ALL[:14] + (0xF00000,)                                  # the flags on a word, so that a float output may stand there
NONE = (None,) * 15
REQUIRED = (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11)


def _call(params, Wn, H, pointers, device_call, device=0):
    lib = capi.load_library()
    p = C.byref(params) if params is not None else None
    fn = lib.rt_gradient_reweight_device if device_call else lib.rt_gradient_reweight
    rc = fn(device, p, Wn, H, *pointers, None)
    return rc, lib.rt_last_error().decode()


def test_every_argument_check_comes_before_the_device_in_the_headers_order(have_gpu):
    INV = capi.RT_ERR_INVALID
    for device_call in (False, True):
        rc, msg = _call(None, 0, 0, NONE, device_call)
        assert rc == INV and "params" in msg
        for bad, word in BAD_PARAMS:
            rc, msg = _call(P(*bad), 0, 0, NONE, device_call)
            assert rc == INV and word in msg, (bad, msg)
        for Wn, H in ((0, 3), (4, 0), (-1, 3), (4, -2)):
            rc, msg = _call(P(*GOOD), Wn, H, NONE, device_call)
            assert rc == INV and "Wn, H" in msg, (Wn, H, msg)
        for Wn, H in ((1 << 15, 1 << 15), (533333334, 1), (23095, 23094)):
            assert "too large" in _call(P(*GOOD), Wn, H, NONE, device_call)[1]
        for Wn, H in ((1 << 26, 1), (1 << 26, 7), (67108861, 7)):       # 2^24 tiles of 4 x 64 pixels or more
            assert "too thin" in _call(P(*GOOD), Wn, H, NONE, device_call)[1], (Wn, H)
        for Wn, H in ((23094, 23094), (67108860, 1), (1, 533333333), (66666666, 8)):
            rc, msg = _call(P(*GOOD), Wn, H, NONE, device_call)        # allowed: the next check speaks
            assert rc == INV and "NULL" in msg, (Wn, H, msg)
        for edge in EDGE_PARAMS:
            assert "is NULL" in _call(P(*edge), 8, 6, NONE, device_call)[1]
        for missing in REQUIRED:                                     # every required buffer, the records misaligned as well
            args = list(ALL)
            args[1] = INPUTS[1] + 8
            args[missing] = None
            rc, msg = _call(P(*GOOD), 8, 6, args, device_call)
            assert rc == INV and "is NULL" in msg, (missing, msg)
    # the device variant: the records' alignment, then the floats', then the overlaps
    for slot in (1, 7, 8):
        for off in (4, 8, 12):
            args = list(ALL)
            args[slot] += off
            args[0] += 2                                             # (a misaligned float too)
            rc, msg = _call(P(*GOOD), 8, 6, args, True)
            assert rc == INV and "16-byte" in msg, (slot, off)
    for slot in (0, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13):
        args = list(ALL)
        args[slot] += 2
        args[14] = INPUTS[1]                                         # (an overlapping output too)
        rc, msg = _call(P(*GOOD), 8, 6, args, True)
        assert rc == INV and "4-byte" in msg, slot
    # a 4 x 6 rectangle of three channels at scale 2 -- 2 x 3 cells: cur and value 288 bytes, records 1152, moments 192, length,
    # variance and lambda 96, flags 24; the cell frames 72 and their records 288
    size = {0: 288, 1: 1152, 2: 288, 3: 192, 4: 96, 5: 72, 6: 72, 7: 288, 8: 288, 9: 288, 10: 192, 11: 96, 12: 96, 13: 96, 14: 24}
    cases = []
    for o in range(9, 15):
        step = 1 if o == 14 else 4
        for q in list(range(9)) + [k for k in range(9, 15) if k != o]:
            own = q == o - 7 and o < 12
            word = "d_cur or d_hits" if q < 2 else "another output" if q >= 9 else "a cell buffer" if q >= 5 else "an input"
            cases += [(o, WORDS[q], not own, word), (o, WORDS[q] + size[q] - step, True, word), (o, WORDS[q] - size[o] + step, True, word),
                      (o, WORDS[q] + size[q], False, word), (o, WORDS[q] - size[o], False, word)]
            if own:
                cases += [(o, WORDS[q] + 4, True, "partially"), (o, WORDS[q] - 4, True, "partially")]
    for o, address, refused, word in cases:
        args = list(WORDS)
        args[o] = address
        rc, msg = _call(P(*GOOD), 4, 6, args, True, device=-1)
        # (in place and adjacent are not overlapping: the call goes on to the device, whose index is bad or which there is none of)
        assert rc != capi.RT_OK and ("overlaps" in msg) == refused and (not refused or (rc == INV and word in msg)), (o, hex(address), msg)
    args = list(WORDS)
    args[9:12] = args[2:5]                                           # the whole history in place
    rc, msg = _call(P(*GOOD), 4, 6, args, True, device=-1)
    assert rc != capi.RT_OK and "overlaps" not in msg
    # a NULL then_hits overlaps nothing, wherever an output stands
    rc, msg = _call(P(*GOOD), 4, 6, args[:8] + [None] + args[9:], True, device=-1)
    assert rc != capi.RT_OK and "overlaps" not in msg and "NULL" not in msg
    if have_gpu:
        return
    NODEV = capi.RT_ERR_NO_DEVICE                                    # every admitted edge reaches the device check
    for edge in EDGE_PARAMS:
        assert _call(P(*edge), 4, 6, args, True)[0] == NODEV
        assert _call(P(*edge), 4, 6, list(ALL[:8]) + [None] + list(ALL[9:12]) + [None, None, None], True)[0] == NODEV
    host = [np.zeros(size[k] * 16, dtype=np.uint8) for k in range(15)]       # (room for any admitted scale's cells)
    assert _call(P(*GOOD), 4, 6, [a.ctypes.data for a in host], False)[0] == NODEV
    assert _call(P(*GOOD), 4, 6, [a.ctypes.data for a in host[:8]] + [None] + [a.ctypes.data for a in host[9:12]] + [None] * 3, False)[0] == NODEV


def test_python_wrappers_refuse_without_a_device(have_gpu):
    from tilecoderaytracer_amd import gradient_params, gradient_reweight
    pr = gradient_params()
    assert [getattr(pr, n) for n, _ in pr._fields_][:4] == [3, 2, 1, 1]
    assert (pr.normal_cos, pr.gain, pr.lambda_min, pr.den_floor) == (float(F(0.9)), 2.0, 0.0, float(F(1e-6)))
    pr = gradient_params(1, 8, 0, False, 0.5, 4.0, 0.25, 0.5)
    assert [getattr(pr, n) for n, _ in pr._fields_] == [1, 8, 0, 0, 0.5, 4.0, 0.25, 0.5]
    hits, lo_hits = np.zeros((8, 6), dtype=HIT_DTYPE), np.zeros((4, 3), dtype=HIT_DTYPE)
    cur, moments, length = np.zeros((8, 6, 3), dtype=F), np.zeros((8, 6, 2), dtype=F), np.zeros((8, 6), dtype=F)
    lo = np.zeros((4, 3, 3), dtype=F)
    with pytest.raises(ValueError):
        gradient_reweight(cur, hits, cur[..., 0], moments, length, lo, lo, lo_hits)
    with pytest.raises(ValueError):
        gradient_reweight(cur, hits, cur, moments[:7], length, lo, lo, lo_hits)
    with pytest.raises(ValueError):
        gradient_reweight(cur, hits, cur, moments, length, lo, lo, lo_hits, scale=3)       # 3 x 2 cells, not 4 x 3
    with pytest.raises(ValueError):
        gradient_reweight(cur, hits, cur, moments, length, lo, lo[..., 0], lo_hits)
    with pytest.raises(ValueError):
        gradient_reweight(cur, hits, cur, moments, length, lo, lo, lo_hits, lo_hits[:3])
    with pytest.raises(TypeError):
        gradient_reweight(cur, hits, cur, moments, length, lo, lo, lo_hits, channels=3)
    if have_gpu:
        return                                                   # (what follows is the refusal for want of a device)
    from tilecoderaytracer_amd import RtError
    with pytest.raises(RtError) as e:
        gradient_reweight(cur, hits, cur, moments, length, lo, lo, lo_hits, lo_hits)
    assert e.value.code == capi.RT_ERR_NO_DEVICE
    with pytest.raises(RtError) as e:
        gradient_reweight(cur[..., 0], hits, cur[..., 0], moments, length, lo[..., 0], lo[..., 0], lo_hits, scale=9)
    assert e.value.code == capi.RT_ERR_INVALID and "scale" in e.value.message


# ---- 3. gradient_ref: the definition ----------------------------------------------------------------------------------------------

def by_hand(cur, hits, value, moments, length, now_lo, then_lo, lo_hits, then_hits, x, z, scale, radius, match_color, normal_cos,
            gain, lambda_min, den_floor, wrong=None):
    """pixel (x, z) by the header's definition, every operation on np.float32 scalars -> (value list, m1, m2, len, variance,
    lambda, flag); wrong: one of gradient_edges.WRONG_RULES, the one line of the definition stated that way instead"""
    Wl, Hl = lo_hits.shape
    zero, one = F(0.0), F(1.0)
    h = hits[x, z]
    c, v = [F(t) for t in np.atleast_1d(cur[x, z])], [F(t) for t in np.atleast_1d(value[x, z])]
    n = len(c)
    m1, m2, L = F(moments[x, z, 0]), F(moments[x, z, 1]), F(length[x, z])
    lum = lambda w: (F(0.25) * w[0] + F(0.5) * w[1]) + F(0.25) * w[2] if n == 3 else w[0]
    dead = lambda g: g["object"] < 0 or (g["flags"] & 2) != 0
    side = 0 if wrong == "side_bit_unread" else 3

    def result(vo, m1o, m2o, Lo, lam, flag, m1i=m1, m2i=m2):
        t = m2i - m1i * m1i if wrong == "variance_of_the_input" else m2o - m1o * m1o
        return vo, m1o, m2o, Lo, (t if t > 0 else zero), (lam if lam > 0 else zero), flag

    if dead(h) or not (L >= one if wrong == "length_at_least_one" else L > one):
        return result(v, m1, m2, L, zero, 0)
    cnt, num, den = 0, zero, zero
    last = radius if wrong == "window_to_r" else radius + 1
    i0, j0 = x // scale, z // scale
    for a in range(-radius, last + 1):
        for b in range(-radius, last + 1):
            i, j = i0 + a, j0 + b
            if not (0 <= i < Wl and 0 <= j < Hl):
                continue
            g = lo_hits[i, j]
            if dead(g) or g["object"] != h["object"] or (g["flags"] & side) != (h["flags"] & side):
                continue
            if match_color and wrong != "colours_unread" and g["color"].tobytes() != h["color"].tobytes():
                continue
            n_p, n_q = [F(t) for t in h["normal"]], [F(t) for t in g["normal"]]
            t = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
            if not (t > F(normal_cos) if wrong == "greater" else t >= F(normal_cos)):
                continue
            ln, lt = lum([F(t) for t in np.atleast_1d(now_lo[i, j])]), lum([F(t) for t in np.atleast_1d(then_lo[i, j])])
            d = ln - lt
            if d < 0:
                d = -d
            m = ln
            if lt > m:
                m = lt
            if wrong == "m_is_the_sum":
                m = ln + lt
            if then_hits is not None and wrong != "changed_cell_keeps_d":
                k = then_hits[i, j]
                if k["object"] != g["object"] or (k["flags"] & 3) != (g["flags"] & 3):
                    d = m
            cnt, num, den = cnt + 1, num + d, den + m
    if cnt == 0:
        return result(v, m1, m2, L, zero, 2)
    floor = F(den_floor)
    t = num / den if (den >= floor if wrong == "den_at_least_floor" else den > floor) else zero
    lam = F(gain) * t
    if lam > one:
        lam = one
    if not (lam >= F(lambda_min) if wrong == "at_least_lambda_min" else lam > F(lambda_min)):
        return result(v, m1, m2, L, lam, 0)
    l = lum(c)
    if lam == one and wrong != "restart_is_a_reblend":
        return result(list(c), l, l * l, one, lam, 3)
    vo = [v[k] + lam * (c[k] - v[k]) for k in range(n)]
    m1o = m1 + lam * (l - m1)
    m2o = m2 + lam * (l * l - m2)
    al = one / L
    a2 = al + lam * (one - al)
    Lo = one / a2
    if not Lo >= one:
        Lo = one
    if not Lo <= L and wrong != "length_not_capped":
        Lo = L
    return result(vo, m1o, m2o, Lo, lam, 3 if lam == one else 1)


def compare_by_hand(inputs, kw, wrong=None):
    """-> (the reference's outputs, the pixels at which the scalar restatement differs from them)"""
    out = gradient_ref.reweight(*inputs, **kw)
    Wn, H = inputs[1].shape
    differ = []
    with np.errstate(all="ignore"):
        for x in range(Wn):
            for z in range(H):
                vo, m1, m2, Lo, var, lam, flag = by_hand(*inputs, x, z, wrong=wrong, **kw)
                got = [np.atleast_1d(out[0][x, z]), out[1][x, z], out[2][x, z], out[3][x, z], out[4][x, z]]
                want = [np.array(vo, dtype=F), np.array([m1, m2], dtype=F), F(Lo), F(var), F(lam)]
                if flag != int(out[5][x, z]) or not all(same_bits(g, w) for g, w in zip(got, want)):
                    differ.append((x, z))
    return out, differ


def assert_ref_is_by_hand(inputs, what, **kw):
    out, differ = compare_by_hand(inputs, kw)
    assert not differ, (what, kw, differ[:5])
    return out


@pytest.mark.parametrize("channels", [3, 1])
def test_ref_equals_the_definition_in_float32_scalars_on_made_up_records(channels):
    seen = np.zeros(4, dtype=np.int64)
    for k, (Wn, H, scale, radius) in enumerate(((7, 5, 2, 2), (23, 70, 2, 1), (23, 70, 3, 0), (13, 37, 5, 2), (17, 20, 8, 1))):
        inputs = made_up_inputs(Wn * 100 + H + channels, Wn, H, channels, scale)
        if k % 2:
            inputs[8] = None
        kw = dict(scale=scale, radius=radius, match_color=bool((radius + channels) % 2), normal_cos=(0.3, -1.0, 0.7)[radius],
                  gain=(1.0, 2.0, 8.0)[radius], lambda_min=(0.0, 0.1, 0.0)[radius], den_floor=(1e-6, 0.0, 0.5)[radius])
        out = assert_ref_is_by_hand(inputs, f"{Wn}x{H}", **kw)
        seen += np.bincount(out[5].reshape(-1), minlength=4)[:4]
    assert (seen >= 40).all(), seen                               # untouched, re-blended, left for no cell and restarted


# ---- 4. WHAT FOLLOWS, line by line -------------------------------------------------------------------------------------------------

KWS = [dict(scale=2, radius=1, match_color=True, normal_cos=0.3, gain=2.0, lambda_min=0.0, den_floor=1e-6),
       dict(scale=3, radius=2, match_color=False, normal_cos=-1.0, gain=1.0, lambda_min=0.1, den_floor=0.0),
       dict(scale=4, radius=0, match_color=True, normal_cos=0.5, gain=8.0, lambda_min=0.0, den_floor=0.25),
       dict(scale=8, radius=2, match_color=False, normal_cos=0.9, gain=0.5, lambda_min=1.0, den_floor=1e-6)]


@pytest.mark.parametrize("channels", [3, 1])
def test_equal_cell_frames_change_nothing_and_neither_does_gain_zero(channels):
    Wn, H = 23, 70
    for kw in KWS:
        inputs = made_up_inputs(40 + channels, Wn, H, channels, kw["scale"])
        cur, hits, value, moments, length, now_lo, then_lo, lo_hits, then_hits = inputs
        for then in (None, lo_hits.copy()):
            for lo in (now_lo, then_lo):                          # (NaN and infinities among the cells' words)
                out = gradient_ref.reweight(cur, hits, value, moments, length, lo, lo.copy(), lo_hits, then, **kw)
                same_words(out[:3], (value, moments, length), f"equal cell frames {kw}")
                assert not out[4].view(np.uint32).any() and not (out[5] & 1).any()
        out = gradient_ref.reweight(*inputs, **dict(kw, gain=0.0))
        same_words(out[:3], (value, moments, length), f"gain 0 {kw}")
        assert not out[4].view(np.uint32).any() and not (out[5] & 1).any()
        # and the cell frames do matter: with the case's own gain pixels are touched, unless lambda_min is 1
        out = gradient_ref.reweight(*inputs, **kw)
        assert ((out[5] & 1) != 0).sum() >= (0 if kw["lambda_min"] == 1.0 else 100), kw


@pytest.mark.parametrize("channels", [3, 1])
def test_a_pixel_at_or_below_lambda_min_keeps_every_word_and_its_variance(channels):
    Wn, H = 23, 70
    for kw in KWS:
        inputs = made_up_inputs(50 + channels, Wn, H, channels, kw["scale"])
        value, moments, length = inputs[2:5]
        out = gradient_ref.reweight(*inputs, **kw)
        lam, flags = out[4], out[5]
        keep = ~(lam > F(kw["lambda_min"]))
        assert keep.sum() >= 200 and ((flags[keep] & 1) == 0).all() and ((flags[~keep] & 1) == 1).all()
        same_words([o[keep] for o in out[:3]], [a[keep] for a in (value, moments, length)], f"left alone {kw}")
        with np.errstate(all="ignore"):
            t = moments[..., 1] - moments[..., 0] * moments[..., 0]
            variance = np.where(t > 0, t, F(0)).astype(F)
        assert out[3][keep].tobytes() == variance[keep].tobytes()
        restarted = flags == 3
        assert (out[2][restarted] == 1).all() and (lam[restarted] == 1).all()
        assert same_bits(out[0][restarted], inputs[0][restarted])


def test_the_call_is_not_idempotent():
    inputs = made_up_inputs(61, 23, 70, 3, 2, special=False)
    kw = KWS[0]
    once = gradient_ref.reweight(*inputs, **kw)
    twice = gradient_ref.reweight(inputs[0], inputs[1], once[0], once[1], once[2], *inputs[5:], **kw)
    blended = once[5] == 1
    assert blended.sum() >= 100
    assert (np.ascontiguousarray(twice[0]).view(np.uint32) != np.ascontiguousarray(once[0]).view(np.uint32)).any(axis=-1)[blended].mean() > 0.5
    again = twice[2] > 1                                         # (a restarted pixel has no history the second time)
    assert again.sum() >= 1000 and twice[4][once[2] > 1].tobytes() == once[4][once[2] > 1].tobytes()      # lambda depends on the cell frames alone


def test_a_strip_equals_the_frames_columns_but_those_whose_window_reaches_beyond_it():
    Wn, H = 24, 70
    for channels in (3, 1):
        for kw in KWS[:3]:
            s, r = kw["scale"], kw["radius"]
            inputs = made_up_inputs(90 + channels, Wn, H, channels, s)
            full = gradient_ref.reweight(*inputs, **kw)
            x0, x1 = 2 * s, Wn - 3
            i0, i1 = x0 // s, -(-x1 // s)
            part = [np.ascontiguousarray(a[x0:x1]) for a in inputs[:5]] + [np.ascontiguousarray(a[i0:i1]) for a in inputs[5:]]
            strip = gradient_ref.reweight(*part, **kw)
            # column x's window is cell columns x/s - r .. x/s + r + 1: inside the strip's cells [i0, i1) or beyond the frame's
            Wl = -(-Wn // s)
            cols = [x for x in range(x0, x1) if x // s - r >= i0 and (x // s + r + 1 < i1 or i1 == Wl)]
            assert len(cols) >= 2 or r == 2, (kw, cols)
            for x in cols:
                same_words([o[x - x0] for o in strip], [f[x] for f in full], f"strip column {x} {kw}")
            assert any(o[0].tobytes() != f[x0].tobytes() for o, f in zip(strip, full)) or r == 0, kw


# ---- 5. the conditions on the ghost pixels ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gradient_setting(name, W, H):
    """clamp_scenes.ghost_setting(name, W, H) and what a gradient needs beside it: the oracle's colours of the previous pose and
    its records (the cameras are equal, so they are this frame's points in the previous frame's scene) -> (the setting, before,
    prev_hits)"""
    setting = ghost_setting(name, W, H)
    cam_prev, _, prev_hits, hits = motion_scenes.records(name, W, H)
    assert hits.tobytes() == setting[1].tobytes()
    scene = motion_scenes.oracle(motion_scenes.PAIRS[name][0])
    cameras.put(cam_prev, orc=scene)
    before = scene.render(W, H, 4)
    before.setflags(write=False)
    return setting, before, prev_hits


def ghost_reweight(name, scale, radius=1, gain=2.0, noise=None, **kw):
    (cur, hits, value, moments, length, ghost, unchanged), before, prev_hits = gradient_setting(name, 192, 128)
    now_lo, then_lo = np.ascontiguousarray(cur[::scale, ::scale]), np.ascontiguousarray(before[::scale, ::scale])
    if noise is not None:
        now_lo, then_lo = (now_lo + noise[::scale, ::scale, None]).astype(F), (then_lo + noise[::scale, ::scale, None]).astype(F)
    lo_hits, then_hits = np.ascontiguousarray(hits[::scale, ::scale]), np.ascontiguousarray(prev_hits[::scale, ::scale])
    return gradient_ref.reweight(cur, hits, value, moments, length, now_lo, then_lo, lo_hits, then_hits, scale=scale,
                                 radius=radius, gain=gain, details=True, **kw), (now_lo, then_lo, lo_hits, then_hits)


@pytest.mark.parametrize("name", GHOST_PAIRS)
def test_the_gradient_halves_the_ghost_beats_the_clamp_and_spares_the_unchanged_pixels(name):
    """Measured with the reference at 192 x 128, r = 1, gain 2, the other parameters at their defaults; the figures are printed
    (pytest -s) and recorded in the README."""
    cur, hits, value, moments, length, ghost, unchanged = gradient_setting(name, 192, 128)[0]
    without = ghost_error(value, cur, ghost)
    clamped = ghost_error(clamp_ref.clamp(cur, hits, value, moments, length, **GHOST_KW)[0], cur, ghost)
    assert ghost.sum() >= 200 and unchanged.sum() >= 10000
    for scale in (2, 3, 4):
        out, _ = ghost_reweight(name, scale)
        error = ghost_error(out[0], cur, ghost)
        touched = unchanged & (out[4] > 0)
        print(name, "scale", scale, "ghost pixels", int(ghost.sum()), "error without", without, "clamp r=1", clamped, "gradient", error,
              "ratio", error / without, "unchanged", int(unchanged.sum()), "of them with lambda > 0", int(touched.sum()),
              "flags 1 / 2 / 3", [int((out[5] == k).sum()) for k in (1, 2, 3)])
        assert error <= 0.5 * without, (scale, error, without)                                # (i)
        assert scale != 2 or error < clamped, (error, clamped)                                # (ii)
        assert touched.sum() <= 0.10 * unchanged.sum(), (scale, int(touched.sum()))           # (iii)
        assert np.ascontiguousarray(out[0]).view(np.uint32)[touched].tobytes() == np.ascontiguousarray(value).view(np.uint32)[touched].tobytes()


@pytest.mark.parametrize("name", GHOST_PAIRS)
def test_noise_common_to_both_cell_frames_touches_no_pixel_whose_cells_are_unchanged(name):
    """(iv): a seeded noise plane of sigma 0.2 added to both cell planes alike"""
    noise = (np.random.default_rng(7).normal(size=(192, 128)) * 0.2).astype(F)
    for scale in (2, 4):
        quiet, (now_lo, then_lo, lo_hits, then_hits) = ghost_reweight(name, scale)
        noisy, _ = ghost_reweight(name, scale, noise=noise)
        same = (now_lo.view(np.uint32) == then_lo.view(np.uint32)).all(axis=-1) & (lo_hits["object"] == then_hits["object"]) & \
            ((lo_hits["flags"] & 3) == (then_hits["flags"] & 3))
        # a pixel's window holds only unchanged cells: every cell of it that exists, counted or not
        Wl, Hl = same.shape
        padded = np.ones((Wl + 4, Hl + 4), dtype=bool)
        padded[1:1 + Wl, 1:1 + Hl] = same
        whole = np.ones((Wl, Hl), dtype=bool)
        for a in range(-1, 3):
            for b in range(-1, 3):
                whole &= padded[1 + a:1 + a + Wl, 1 + b:1 + b + Hl]
        pixels = np.repeat(np.repeat(whole, scale, axis=0), scale, axis=1)[:192, :128]
        print(name, "scale", scale, "pixels whose cells are all unchanged", int(pixels.sum()), "noisy flags there",
              np.bincount(noisy[5][pixels], minlength=4).tolist())
        assert pixels.sum() >= 10000
        assert (noisy[5][pixels] == quiet[5][pixels]).all() and noisy[4][pixels].tobytes() == quiet[4][pixels].tobytes()
        # namely 0 -- but for the pixels none of whose cells lies on their surface, whose flag the definition sets to 2 with
        # or without noise
        counted = noisy[6]["cells"] > 0
        assert not noisy[4][pixels].view(np.uint32).any() and (noisy[5][pixels & counted] == 0).all()
        assert (noisy[5][pixels & ~counted & noisy[6]["walked"]] == 2).all() and (pixels & ~counted).sum() <= 0.01 * pixels.sum()
        same_words([o[pixels] for o in noisy[:3]], [o[pixels] for o in quiet[:3]], "noise")


# ---- 6. the edge inputs of gradient_edges.py ---------------------------------------------------------------------------------------

def edge_case(name):
    """a case of gradient_edges.CASES with three channels or one, in turn by its place in the list -> (inputs, kw)"""
    channels = 3 if list(gradient_edges.CASES).index(name) % 2 == 0 else 1
    case = gradient_edges.CASES[name](channels)
    return case[:9], case[9]


@pytest.mark.parametrize("name", list(gradient_edges.CASES))
def test_ref_equals_the_definition_in_float32_scalars_on_the_edge_inputs(name):
    inputs, kw = edge_case(name)
    hits, length = inputs[1], inputs[4]
    assert hits.shape[0] <= 13 and hits.shape[1] <= 130
    out = assert_ref_is_by_hand(inputs, name, **kw)
    lam, flags = out[4], out[5]
    walked = ~clamp_ref.dead_records(hits) & (length > F(1.0))
    if name == "G1_lambda_at_min":
        assert walked.all() and (lam == F(0.5)).all() and (flags == 0).all()
        same_words(out[:3], inputs[2:5], name)
    if name == "G1_lambda_above_min":
        assert (lam == F(0.5)).all() and (flags == 1).all()
    if name == "G2_gain_t_is_one":
        assert (lam == 1).all() and (flags == 3).all() and (out[2] == 1).all() and same_bits(out[0], inputs[0])
    if name == "G2_gain_t_below_one":
        assert (lam == np.nextafter(F(1), F(0))).all() and (flags == 1).all()
    if name.startswith("G3"):
        inner = np.zeros(flags.shape, dtype=bool)
        inner[2:-4, 2:-4] = True                                 # r = 1 at scale 2: the window is whole from cell 1 to the last but two
        assert (flags[~inner] == 0).all() and (flags[inner] == (1 if name.endswith("above_floor") else 0)).all()
    if name == "G4_dot_at_cos":
        assert (flags == 1).all() and (lam > 0).all()
    if name in ("G4_dot_under_cos", "G5_side_in_lo", "G6_colour_matched", "G13_then_null"):
        assert (flags == 0).all() and not lam.view(np.uint32).any()
    if name in ("G5_side_in_then", "G6_colour_unmatched"):
        assert (flags == 1).sum() >= 500
    if name == "G7_lengths":
        assert (walked == (length > 1)).all() and not walked[length == 1].any() and walked[length == np.nextafter(F(1), F(2))].all()
        assert (flags[walked] == 1).all() and (flags[~walked] == 0).all()
        assert (out[2][walked] >= 1).all() and (out[2][walked] <= length[walked]).all()
    if name == "G8_cap":
        assert (flags == 1).all() and (out[2] <= length).all() and (out[2] == length).sum() >= 100
    if name == "G11_nan_counted":
        nan = np.isnan(inputs[5].reshape(inputs[7].shape + (-1,))[..., 0])
        has = np.repeat(np.repeat(nan | np.roll(nan, -1, 0) | np.roll(nan, -1, 1) | np.roll(np.roll(nan, -1, 0), -1, 1), 2, 0), 2, 1)
        inner = np.zeros(flags.shape, dtype=bool)
        inner[:-2, :-2] = True                                   # (where np.roll does not wrap)
        inner &= has[:flags.shape[0], :flags.shape[1]]
        assert inner.sum() >= 100 and (flags[inner] == 0).all() and not lam[inner].view(np.uint32).any()
        assert (flags == 1).sum() >= 100
    if name == "G11_nan_uncounted":
        assert (flags == 1).sum() >= 500 and not np.isnan(out[0]).any() and (lam[flags == 1] == F(0.5)).all()
    if name.startswith("G12"):
        assert (flags == 1).sum() >= 20 and (flags == 0).sum() >= 20


WRONG = [(rule, name) for rule, names in gradient_edges.WRONG_RULES.items() for name in names]


@pytest.mark.parametrize("rule, name", WRONG, ids=[f"{r}-{n}" for r, n in WRONG])
def test_the_edge_inputs_tell_each_wrong_rule_from_the_headers(rule, name):
    """the condition that the inputs can discriminate: the per-pixel restatement with one line changed differs from the
    reference in at least 20 pixels of the case"""
    inputs, kw = edge_case(name)
    _, differ = compare_by_hand(inputs, kw, wrong=rule)
    print(rule, name, "pixels that differ:", len(differ), "of", inputs[1].size)
    assert len(differ) >= 20, (rule, name, len(differ))


def test_every_wrong_rule_of_the_issue_is_told_apart_by_a_named_input():
    for rule in ("window_to_r", "m_is_the_sum", "changed_cell_keeps_d", "at_least_lambda_min", "restart_is_a_reblend",
                 "length_not_capped", "variance_of_the_input"):
        assert gradient_edges.WRONG_RULES[rule] and all(n in gradient_edges.CASES for n in gradient_edges.WRONG_RULES[rule]), rule
