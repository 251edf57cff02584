"""What tests/test_gpu_frame_kernels.py and tests/test_frame_kernels_host.py share, numpy and the oracle alone: the encode matrix and the
k_encode instantiations it launches, the configurations of the other sections, the frames, the oracle's planes of a launch, and the
comparison of a call's plane buffers with them.

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import numpy as np

from tests.golden.make_golden import special_frame
from tests.support.host import GAP, gaps_intact, layout, plane_rows, plane_samples, same_rows, widen_halves

NF = 3
SIZES = [(64, 32), (258, 6), (6, 4)]        # four pixels per thread where the mode has such a kernel / a ragged last tile / one tile
LUV, RGB, YCC, XYZ = 0, 1, 2, 3             # include/lumahip.h lumahip_colorspace
PQ, LINEAR = 1, 4                           # lumahip_ptf
# colour space -> (name, bitdepthC, maxLum, minLum, the preScalings its rows run with)
SPACES = {LUV: ("luv", 8, 1e4, 0.005, (1.0,)), RGB: ("rgb", 8, 1e4, 0.005, (1.0,)), YCC: ("ycbcr", 10, 1000.0, 0.01, (1.0, 20.0)),
          XYZ: ("xyz", 8, 1e4, 0.005, (1.0,))}
# search mode (lut_index.hpp LutMode) -> (ptf, bits, tunes) that put a context into it (lumahip_core.hip ensure_search_index)
MODES = {3: (PQ, 11, ()), 4: (PQ, 11, (("lds_table_max_kb", 0),)), 7: (LINEAR, 12, ()), 0: (PQ, 11, (("force_literal", 1),)),
         2: (PQ, 13, (("force_literal", 1),))}
FORMS = ("planar", "f16", "planar_f16")     # the call forms that go round the matrix beside the packed float call
MIN_DISTINCT = 64                           # sample values an expected plane of 64x32 or 258x6 holds at least


def config(cs, ptf, bits):
    _, bits_c, max_lum, min_lum, _ = SPACES[cs]
    return (ptf, bits, cs, bits_c, max_lum, min_lum)


def pq8(cs):
    return config(cs, PQ, 8)


def pq13(cs):
    """the 13-bit sibling whose table (32 KiB) leaves LDS under "lds_table_max_kb" 0: evenly spaced for XYZ, PQ elsewhere"""
    return config(cs, LINEAR if cs == XYZ else PQ, 13)


def encode_matrix():
    """rows of (id, cs, mode, configuration, tunes, profile, w, h, preScaling, stats, second form, lm5): every search mode by every
    colour space, both 16-bit profiles and the three sizes; `stats` on every other row; the second call form going round, so that
    each form meets every (colour space, mode).  YCbCr rows of mode 3 come twice: with statistics (LM 3) and, `lm5`, without and
    under "half_table" 0 (float frames then take the composite records, LM 5; halves keep LM 3 -- lumahip_encode.hip
    encode_frames_device_impl).  The 8-bit profiles run on one records-in-LDS row per colour space (`pq8`)."""
    out = []
    for ci, cs in enumerate((LUV, RGB, YCC, XYZ)):
        name, _, _, _, scs = SPACES[cs]
        for mi, mode in enumerate((3, 4, 7, 0, 2)):
            ptf, bits, tunes = MODES[mode]
            for sc in scs:
                j = 0
                for profile in (2, 3):
                    for (w, h) in SIZES:
                        form = FORMS[(ci + mi + j) % 3]
                        ident = "%s-m%d-sc%g-p%d-%dx%d" % (name, mode, sc, profile, w, h)
                        if cs == YCC and mode == 3:
                            tn = (("half_table", 0),)
                            out.append((ident + "-stats", cs, mode, config(cs, ptf, bits), tn, profile, w, h, sc, True, form, False))
                            out.append((ident + "-lm5", cs, mode, config(cs, ptf, bits), tn, profile, w, h, sc, False, form, True))
                        else:
                            out.append((ident, cs, mode, config(cs, ptf, bits), tunes, profile, w, h, sc, (ci + mi + j) % 2 == 0, form, False))
                        j += 1
        for j, profile in enumerate((0, 1)):
            for k, (w, h) in enumerate(SIZES):
                out.append(("%s-pq8-p%d-%dx%d" % (name, profile, w, h), cs, 3, pq8(cs), (("half_table", 0),) if cs == YCC else (), profile, w, h,
                            scs[-1], cs == YCC or (j + k) % 2 == 0, FORMS[(ci + j + k) % 3], False))
    return out


def kernel_of(cs, mode, profile, w, lm5):
    """(CS, SUB, VW, LM) of the k_encode a float launch of this row takes (frames 16-byte aligned, frame stride % 4 == 0):
    lumahip_encode.hip -- four pixels per thread for the record searches at w % 4 == 0, two otherwise"""
    return (cs, profile in (0, 2), 4 if (mode in (3, 4, 7) and w % 4 == 0) else 2, 5 if lm5 else mode)


# ---- the frames of a launch and the oracle's planes of them
def frames(w, h, nf=NF, halves=False):
    """nf distinct (3, h, w) frames as tests/test_gpu_parity.py frames() makes its first: log-uniform over 1e-4 .. 3e4, special_frame
    (NaN, infinities, negatives, zeros) in the corner of the sizes that hold it; frame f is seeded w * 131 + h + 7919 f.
    halves: the same narrowed to binary16 (1e9 and 3e38 become inf, 1e-30 zero)"""
    out = []
    for f in range(nf):
        rng = np.random.default_rng(w * 131 + h + 7919 * f)
        a = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(3, h, w))).astype(np.float32)
        if h >= 8 and w >= 16:
            a[:, :8, :16] = special_frame(8, 16)
        out.append(a)
    out = np.stack(out)
    with np.errstate(over="ignore"):
        return out.astype(np.float16) if halves else out


_orc, _exp = {}, {}


def oracle(o, cfg):
    if cfg not in _orc:
        _orc[cfg] = o.Oracle(*cfg)
    return _orc[cfg]


def expected(o, cfg, profile, w, h, sc, halves=False, nf=NF):
    """(frames, their oracle planes, the oracle's strides) of a launch, computed once per key and never written to: for halves the oracle
    runs on the widened halves"""
    key = (cfg, profile, w, h, sc, halves, nf)
    if key not in _exp:
        fr = frames(w, h, nf, halves)
        wide = widen_halves(fr) if halves else fr
        planes, st = [], None
        for f in range(nf):
            pl, st, _ = oracle(o, cfg).encode(wide[f].copy(), sc, profile)
            planes.append(pl)
        for x in [fr] + [p for pl in planes for p in pl]:
            x.setflags(write=False)
        _exp[key] = (fr, planes, tuple(st))
    return _exp[key]


def expected_stats(o, cfg, frame, sc):
    """{float64 sum, min, max} of the oracle's transformed channel 0 as the kernels fold them: fminf / fmaxf pass over a NaN, the sum
    does not"""
    t = np.array(frame, dtype=np.float32, copy=True)
    oracle(o, cfg).transform(t, True, sc)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(t[0].astype(np.float64).sum()), np.float32(np.nanmin(t[0])), np.float32(np.nanmax(t[0]))


def stats_problem(got, want, rel=1e-4):
    """None, or how a frame's {sum, min, max} misses expected_stats: min and max bit for bit, the sum to `rel`"""
    s, mn, mx = (np.float32(x) for x in got)
    if mn.view(np.uint32) != want[1].view(np.uint32) or mx.view(np.uint32) != want[2].view(np.uint32):
        return "min / max %r %r, expected %r %r" % (mn, mx, want[1], want[2])
    if np.isnan(want[0]) or np.isinf(want[0]):
        ok = (np.isnan(s) and np.isnan(want[0])) or float(s) == want[0]
    else:
        ok = abs(float(s) - want[0]) <= rel * abs(want[0])
    return None if ok else "sum %r, expected %r" % (s, want[0])


def informative(planes, w, h, profile, tag):
    """asserted on the reference alone: each expected plane of each frame holds at least MIN_DISTINCT sample values, U and V differ"""
    for f, pl in enumerate(planes):
        s = [plane_samples(pl[p], w, h, profile, p) for p in range(3)]
        for p in range(3):
            n = np.unique(s[p]).size
            assert n >= MIN_DISTINCT, tag + (f, p, "%d distinct sample values" % n)
        assert not np.array_equal(s[1], s[2]), tag + (f, "U and V are the same")
    return min(np.unique(plane_samples(pl[p], w, h, profile, p)).size for pl in planes for p in range(3))


# ---- layouts
def wide_layout(w, h, profile):
    """row strides wider than the rows that every vector access still takes: row bytes + 16"""
    return tuple(plane_rows(w, h, profile, p)[1] + 16 for p in range(3))


def odd_layout(w, h, profile):
    """(row strides, gaps) that make every row stride and every frame stride odd"""
    st = tuple(rb + 3 if rb % 2 == 0 else rb + 2 for rb in (plane_rows(w, h, profile, p)[1] for p in range(3)))
    size = layout(w, h, profile, st, 0)[1]
    return st, tuple(GAP + (1 if (size[p] + GAP) % 2 == 0 else 0) for p in range(3))


def planes_problem(bufs, exp, w, h, profile, st, gap=GAP, base=0):
    """None, or what is wrong with the three byte buffers of a call that wrote len(exp) frames: plane p of frame f at
    base + f * frame stride, rows st[p] apart.  Every frame's samples are the expected frame's (same_rows), and every byte that is no
    sample -- behind a row, behind a frame (the last one too), in front of the base -- holds the sentinel"""
    nf = len(exp)
    hs, size, pfs = layout(w, h, profile, st, gap)
    for p in range(3):
        if bufs[p].size != base + nf * pfs[p]:
            return "plane %d: %d bytes, the layout has %d" % (p, bufs[p].size, base + nf * pfs[p])
    for f in range(nf):
        got = [bufs[p][base + f * pfs[p]: base + f * pfs[p] + size[p]].reshape(hs[p], st[p]) for p in range(3)]
        if not same_rows(got, exp[f], w, h, profile):
            rb = [plane_rows(w, h, profile, p)[1] for p in range(3)]
            bad = [p for p in range(3) if not np.array_equal(got[p][:, :rb[p]], exp[f][p][:, :rb[p]])]
            return "frame %d: the samples of plane(s) %s differ" % (f, bad)
    if not gaps_intact(bufs, w, h, profile, nf, st, gap, base):
        return "a byte outside the samples changed (row padding, gap, in front of the base or behind the last frame)"
    return None
