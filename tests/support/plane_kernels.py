"""What tests/test_gpu_plane_kernels.py and tests/test_plane_kernels_host.py share, numpy and the oracle alone: the matrix of the
plane-fed calls and the k_transcode / k_transcode_distortion / k_transcode_distortion_map / k_transcode_moments_map instantiations it
launches, the source planes of a launch, the ORACLE's decode -> encode of them, the given planes of the measuring families -- a
perturbed copy of that expectation (tests/support/measuring.py given_from) -- numpy's words for the pair, and wrong kernels modelled
with the oracle and numpy, which every row's inputs must tell from a right one.

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support import measuring as ms
from tests.support.host import SENTINEL, plane_rows
from tests.support.transcode_moments import own_planes_moments

NF = fk.NF
FAMILIES = ("transcode", "distortion", "distortion_map", "moments_map")
SIZES = ms.SIZES
PROFILES = ms.PROFILES
PQ10_YCC = fk.config(fk.YCC, fk.PQ, 10)
PQ8_YCC = (fk.PQ, 8, fk.YCC, 8, 1000.0, 0.01)
SOURCES = (fk.LUV, fk.YCC)                                   # PQ-11 Lu'v' / PQ-10 YCbCr 10
TARGETS = ((fk.LUV, 3), (fk.LUV, 7), (fk.YCC, 5))             # PQ-11 Lu'v' / LINEAR-12 Lu'v' / PQ-10 YCbCr 10, and the LM they come to
PAIRS = tuple((csd, cse) for csd in SOURCES for cse in (fk.LUV, fk.YCC))
EIGHT_BIT = (((0, 1), SIZES[0]), ((3, 1), SIZES[0]), ((1, 0), SIZES[1]), ((0, 2), SIZES[1]))
SC_FAR = 3e5                                                  # outside [2^-16, 2^16]: XformConst::sc_mode 2
FAR_SIZE, FAR_PROFILES = SIZES[1], (2, 2)

Row = collections.namedtuple("Row", "id family csd cse lm scfg dcfg sp dp w h src_sc dst_sc block stats")


def side_cfg(cs, lm, profile):
    """the configuration of one side: PQ-11 (LM 7: LINEAR-12) Lu'v' or PQ-10 YCbCr 10, and in an 8-bit profile the 8-bit table of
    the colour space -- an 11-bit table stored into 8 bits saturates the oracle's luma plane to one value"""
    if profile < 2:
        return fk.pq8(fk.LUV) if cs == fk.LUV else PQ8_YCC
    return PQ10_YCC if cs == fk.YCC else fk.config(fk.LUV, *fk.MODES[lm][:2])


def scalings(csd, cse, lm):
    """[(src_sc, dst_sc)] of a pair's rows: Lu'v' sides take 1; a YCbCr source 1 and 20 (sc_mode 0 and 1); a YCbCr target 20.  The
    evenly spaced LINEAR-12 table spends 410 of its 4096 codes on the 1000 cd/m2 of the YCbCr source, so that target takes ten times
    the source's preScaling: (1, 10) and (20, 200) decode to the same luminances, and both leave the luma plane informative"""
    if csd != fk.YCC:
        return [(1.0, 20.0 if cse == fk.YCC else 1.0)]
    if lm == 7:
        return [(1.0, 10.0), (20.0, 200.0)]
    return [(sc, 20.0 if cse == fk.YCC else 1.0) for sc in (1.0, 20.0)]


def far_scalings(cse, lm):
    return (SC_FAR, 10 * SC_FAR if lm == 7 else SC_FAR)


def sc_mode(sc):
    """luma_device.hpp XformConst::sc_mode of a YCbCr source"""
    return 0 if sc == 1.0 else 1 if 2.0 ** -16 <= sc <= 2.0 ** 16 else 2


def _block(family, n):
    return None if family == "transcode" else ms.block_of(family, n)


def _ident(family, csd, cse, lm, sp, dp, w, h, src_sc, eight=False):
    return "%s-%s-%s-%s-p%d-p%d-%dx%d-sc%g" % (family, fk.SPACES[csd][0], fk.SPACES[cse][0], "pq8" if eight else "lm%d" % lm, sp, dp, w, h, src_sc)


def plane_matrix():
    """Rows of (id, family, CSD, CSE, LM, source configuration, target configuration, sp, dp, w, h, src_sc, dst_sc, block, stats): every
    family by both sources, the three targets, (sp, dp) over {2, 3}^2 and the three sizes, a YCbCr source with both preScalings of
    `scalings`; the blocks going round {16, 32, 64} (moments: {8, 16, 32, 64}), `stats` on every other k_transcode row.  Behind them,
    per (family, colour-space pair), the four 8-bit rows of EIGHT_BIT (LM 3 or 5) and, per (family, YCbCr source, target), one row
    with src_sc 3e5 at 258x6"""
    out = []
    for family in FAMILIES:
        for csd in SOURCES:
            for (cse, lm) in TARGETS:
                n = 0
                for sp in PROFILES:
                    for dp in PROFILES:
                        for (w, h) in SIZES:
                            for (src_sc, dst_sc) in scalings(csd, cse, lm):
                                out.append(Row(_ident(family, csd, cse, lm, sp, dp, w, h, src_sc), family, csd, cse, lm, side_cfg(csd, 3, sp),
                                               side_cfg(cse, lm, dp), sp, dp, w, h, src_sc, dst_sc, _block(family, n), family == "transcode" and n % 2 == 0))
                            n += 1
                if csd == fk.YCC:
                    (w, h), (sp, dp) = FAR_SIZE, FAR_PROFILES
                    src_sc, dst_sc = far_scalings(cse, lm)
                    out.append(Row(_ident(family, csd, cse, lm, sp, dp, w, h, src_sc), family, csd, cse, lm, side_cfg(csd, 3, sp), side_cfg(cse, lm, dp),
                                   sp, dp, w, h, src_sc, dst_sc, _block(family, n), False))
        for (csd, cse) in PAIRS:
            lm = 5 if cse == fk.YCC else 3
            for n, ((sp, dp), (w, h)) in enumerate(EIGHT_BIT):
                src_sc, dst_sc = scalings(csd, cse, lm)[-1]
                out.append(Row(_ident(family, csd, cse, lm, sp, dp, w, h, src_sc, True), family, csd, cse, lm, side_cfg(csd, 3, sp), side_cfg(cse, lm, dp),
                               sp, dp, w, h, src_sc, dst_sc, _block(family, 3 * n), family == "transcode" and n % 2 == 0))
    return out


def kernel_of(row):
    """(family, CSD, SUBD, CSE, SUBE, VW, LM) of the kernel this row's call launches (lumahip_pick.hpp pick_planes), both plane sets
    aligned for units of four samples: transcode_plan takes four pixels per thread at w % 4 == 0, two otherwise"""
    return (row.family, row.csd, row.sp in (0, 2), row.cse, row.dp in (0, 2), 4 if row.w % 4 == 0 else 2, row.lm)


# ---- the planes of a launch
PLANTED = (8, 16)       # luma rows and columns of the corner of 264x70 that holds the boundary and out-of-range codes


def planted_codes(cfg, profile, p):
    """the codes of the corner: 0, 1, the largest code of the plane, the code behind it and all ones, where the sample holds them"""
    top = (1 << (cfg[1] if p == 0 else cfg[3])) - 1
    ones = 0xFFFF if profile > 1 else 0xFF
    return sorted({v for v in (0, 1, top, top + 1, ones) if v <= ones})


def plane_values(plane, profile):
    """the integers of a (rows, row bytes) plane without padding"""
    a = np.ascontiguousarray(plane)
    return (a.view("<u2") if profile > 1 else a).astype(np.int64)


_src = {}


def source_planes(cfg, profile, w, h):
    """NF distinct frames of code planes, each three (rows, row bytes) arrays: seeded random in-range codes -- luma 0 .. 2^bitdepth - 1,
    chroma 0 .. 2^bitdepthC - 1 -- and at 264x70 planted_codes going round the 8x16 corner: a chroma code beyond the largest is what
    sets bad_code and sends its unit to the complete functions.  Made once per key, read-only"""
    key = (cfg, profile, w, h)
    if key not in _src:
        bps, frames = 2 if profile > 1 else 1, []
        for f in range(NF):
            rng = np.random.default_rng([cfg[0], cfg[1], cfg[2], cfg[3], profile, w, h, f])
            fr = []
            for p in range(3):
                rows, rb = plane_rows(w, h, profile, p)
                v = rng.integers(0, 1 << (cfg[1] if p == 0 else cfg[3]), size=(rows, rb // bps))
                if (w, h) == SIZES[0]:
                    sub = 2 if (p and profile in (0, 2)) else 1
                    cr, cc = PLANTED[0] // sub, PLANTED[1] // sub
                    codes = planted_codes(cfg, profile, p)
                    v[:cr, :cc] = np.resize(np.roll(codes, f), cr * cc).reshape(cr, cc)
                a = np.ascontiguousarray(v.astype("<u2" if bps == 2 else np.uint8)).view(np.uint8).reshape(rows, rb)
                a.setflags(write=False)
                fr.append(a)
            frames.append(fr)
        _src[key] = frames
    return _src[key]


Expect = collections.namedtuple("Expect", "s d e")
_exp = {}


def expected(o, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc, nf=NF):
    """The inputs of a launch and what the oracle makes of them, computed once per key and not written to afterwards:
    s   source_planes(scfg, sp, w, h)
    d   the ORACLE's decode of them under the source configuration: (nf, 3, h, w) floats
    e   the ORACLE's encode of d under the target configuration, per frame three (rows, stride) arrays"""
    key = (scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
    if key not in _exp:
        s = source_planes(scfg, sp, w, h)
        st = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        d = np.stack([fk.oracle(o, scfg).decode(s[f], st, w, h, src_sc, sp) for f in range(nf)])
        e = [fk.oracle(o, dcfg).encode(d[f].copy(), dst_sc, dp)[0] for f in range(nf)]
        for a in [d] + [p for fr in e for p in fr]:
            a.setflags(write=False)
        _exp[key] = Expect(s, d, e)
    return _exp[key]


def expected_of(o, row):
    return expected(o, row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc)


Given = collections.namedtuple("Given", "g words dist dmap")
_given = {}


def given_for(o, family, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc, block):
    """the given planes of a measuring launch and numpy's words of (e, g), as measuring.given_for's: g is `expected`'s e perturbed, the
    distortion family sparsely, the map families densely with frame 1 keeping its last block column and row wherever a map has more
    than one.  Once per key, read-only"""
    key = (family, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc, block)
    if key not in _given:
        e = expected(o, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc).e
        rng = np.random.default_rng([FAMILIES.index(family), scfg[1], scfg[2], dcfg[0], dcfg[1], dcfg[2], sp, dp, w, h, int(src_sc), block or 0])
        _given[key] = Given(*ms.given_from(rng, family, e, w, h, dp, block))
    return _given[key]


def given_of(o, row):
    return given_for(o, row.family, row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc, row.block)


def own_planes_measure_nothing(family, own, tag):
    """the call on the planes the kernel is held to: no difference (moments: both signals have the same sums)"""
    if family == "moments_map":
        assert own_planes_moments(own), tag + ("the oracle's own planes", own)
    else:
        assert not own.any(), tag + ("the oracle's own planes", own)


# ---- wrong kernels, modelled with the oracle and numpy alone
def _with_samples(plane, w, h, profile, p, v):
    """a copy of a (rows, stride) plane with the (rows, columns) integers v as its samples"""
    a = np.array(plane, copy=True)
    rows, rb = plane_rows(w, h, profile, p)
    a[:rows, :rb] = np.ascontiguousarray(v.astype("<u2" if profile > 1 else np.uint8)).view(np.uint8).reshape(rows, rb)
    return a


def _samples(plane, w, h, profile, p):
    rows, rb = plane_rows(w, h, profile, p)
    a = np.ascontiguousarray(np.asarray(plane)[:rows, :rb])
    return (a.view("<u2") if profile > 1 else a).astype(np.int64)


def wrong_kernels(o, row):
    """{name: planes}: what kernels with one fault each would make of this row's source planes, as lists of frames of three
    (rows, stride) planes like `expected`'s e.  Only the faults that apply to the row are modelled:
    uv_swapped         U and V change places
    frames_swapped_f   frames f and f + 1 change places
    sc_dropped         a YCbCr source decoded without its `/ sc`
    top_left_chroma    4:4:4 -> 4:2:0: the chroma of a 2x2 cell taken from its top-left pixel instead of the cell's average
    first_of_four      4:2:0 -> 4:4:4: of the four codes a source chroma sample becomes, only the first stored (the others keep
                       what the destination held: the sentinel)
    last_column        one sample of the last column of every plane of frame 1 off by one"""
    ex = expected_of(o, row)
    w, h, sp, dp, e = row.w, row.h, row.sp, row.dp, ex.e
    enc = fk.oracle(o, row.dcfg)
    out = {"uv_swapped": [[fr[0], fr[2], fr[1]] for fr in e]}
    for f in range(NF - 1):
        out["frames_swapped_%d" % f] = [e[f + 1] if k == f else e[f] if k == f + 1 else e[k] for k in range(NF)]
    if row.csd == fk.YCC and row.src_sc != 1.0:
        st = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        out["sc_dropped"] = [enc.encode(fk.oracle(o, row.scfg).decode(ex.s[f], st, w, h, 1.0, sp), row.dst_sc, dp)[0] for f in range(NF)]
    if sp in (1, 3) and dp in (0, 2):
        frames = []
        for f in range(NF):
            d = np.array(ex.d[f], copy=True)
            d[:, 1::2, :] = d[:, 0::2, :]
            d[:, :, 1::2] = d[:, :, 0::2]
            frames.append([e[f][0]] + enc.encode(d, row.dst_sc, dp)[0][1:])
        out["top_left_chroma"] = frames
    if sp in (0, 2) and dp in (1, 3):
        fill = SENTINEL * 0x101 if dp > 1 else SENTINEL
        frames = []
        for f in range(NF):
            fr = [e[f][0]]
            for p in (1, 2):
                v = np.full((h, w), fill, dtype=np.int64)
                v[0::2, 0::2] = _samples(e[f][p], w, h, dp, p)[0::2, 0::2]
                fr.append(_with_samples(e[f][p], w, h, dp, p, v))
            frames.append(fr)
        out["first_of_four"] = frames
    top = 0xFFFF if dp > 1 else 0xFF
    frames = [list(fr) for fr in e]
    for p in range(3):
        v = _samples(e[1][p], w, h, dp, p)
        y = v.shape[0] // 2
        v[y, -1] += 1 if v[y, -1] < top else -1
        frames[1][p] = _with_samples(e[1][p], w, h, dp, p, v)
    out["last_column"] = frames
    return out


def tells(o, row, planes):
    """whether the row's comparison fails for a kernel that makes `planes` of its source: a k_transcode row compares the written
    planes (fk.planes_problem), a measuring row the words of (planes, g) with numpy's of (e, g)"""
    ex = expected_of(o, row)
    if row.family == "transcode":
        hp = ms.HostPlanes(planes, row.w, row.h, row.dp)
        return fk.planes_problem(hp.bufs, ex.e, row.w, row.h, row.dp, hp.st, hp.gap, hp.base) is not None
    gv = given_of(o, row)
    return not np.array_equal(ms.words_of(row.family, planes, gv.g, row.w, row.h, row.dp, row.block), gv.words)


__all__ = ["EIGHT_BIT", "FAMILIES", "NF", "PAIRS", "PROFILES", "SC_FAR", "SIZES", "SOURCES", "TARGETS", "Expect", "Given", "Row", "expected",
           "expected_of", "given_for", "given_of", "kernel_of", "own_planes_measure_nothing", "plane_matrix", "plane_values", "planted_codes",
           "sc_mode", "scalings", "side_cfg", "source_planes", "tells", "wrong_kernels"]
