"""What tests/test_gpu_config_edges.py and tests/test_config_edges_host.py share, numpy and the oracle alone: quantizer configurations at
the edges of what the LDS-staging kernels take, the LDS arithmetic of the host code restated (each function names the line it restates),
the rows of both tests, their inputs -- which reach both ends of every staged table --, the ORACLE's expectation of a row, and wrong
kernels modelled with the oracle and numpy, which every row they apply to must tell from a right one.

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only.

Each configuration is (ptf, luminance bits, colour space, colour bits, maxLum, minLum).  Single quantizers:
  S1  PQ-13 Lu'v' 12            the largest records: 139792 B, 1024 threads; decode 32784 + 16384 B; moments map 139792 + 3840 B
  S2  PQ-12 YCbCr 12 (1000)     composite records + powf 104560 B; decode powf + table + y table + two chroma-term tables 104736 B
  S3  LINEAR-14 Lu'v' 9         value-keyed records, 131344 B; odd colour depth
  S4  PQ-9 YCbCr 9 (1000)       odd depths, small tables
  S5  PQ-6 Lu'v' 5, profiles 0 and 1   tables far smaller than a workgroup (the oracle's luma plane holds all 64 codes at this depth)
  S6  PQ-11 Lu'v' 16            the table leaves LDS on the decode side (colour depth above 12)
  S7  PQ-11 YCbCr 10 (1000)     the half-input table beside 32720 B of composite records: 160224 B; with the moments map's 3840 B it
                                crosses the budget, and binary16 frames fall back to the search of the mode there and nowhere else
  S8  PQ-13 YCbCr 12 (1000)     not in the issue's table: the largest decode-side layout upload_decode_tables accepts is this one's, powf +
                                table + y table + two chroma-term tables = 137504 B (S2's is the largest the plane-fed calls take).  Its
                                140088 B of records do not fit beside the powf tables: search mode 4, which the measuring calls refuse
S1 .. S7 come to a search mode the frame-fed measuring calls take (3 or 7); measuring_lm derives the refusal of S8.
Source -> target pairs (bytes of both sides' tables, k_transcode; the measuring families add 128 / 1536 / 3840 B):
  P1   PQ-12 Lu'v' 8  -> PQ-13 Lu'v' 8       157216   all five families run; the moments map 2784 B below the budget
  P2   PQ-12 Lu'v' 10 -> PQ-13 Lu'v' 8       160288   3552 B below; distortion 160416, map 161824 run; moments 164128: refused, 288 B above
  P3   PQ-12 Lu'v' 12 -> PQ-13 Lu'v' 8       172576   refused by all five
  P3b  PQ-12 Lu'v' 11 -> PQ-13 Lu'v' 8       164384   refused by all five, 544 (distortion 672, map 2080) B above the budget
  P4   S2 -> LOG-12 Lu'v' 8                  147632   all run
  P5   S2 -> PQ-12 Lu'v' 8                   170864   refused by all
  P6   PQ-12 Lu'v' 8 -> S2                   121984   all run (composite records)
  P7a  PQ-12 Lu'v' 8 -> LINEAR-14 Lu'v' 8    148768   all run (value-keyed records)
  P7b  PQ-10 YCbCr 10 -> LINEAR-13 Lu'v' 8   121264   all run
  P8   S4 -> PQ-9 Lu'v' 9 (1000)             small    all run
  P9   S6 -> PQ-11 Lu'v' 8                            S6's colour depth as a source: refused by all five
P3b is not in the issue's table: 12 bits of source colour put P3 8736 B above the budget, 11 bits come within 4 KiB of it.
The preScalings are pk.scalings' for a Lu'v' source; a YCbCr source of maxLum 1000 takes (1, r) and (20, 20 r) with r = 1.25 target
maxLum / source maxLum -- pk.scalings gives the LINEAR-12 target 10 for the same reason --, so that the grey pixels of the source's
largest luma codes come to the target's largest code whatever the colour codes' rounding takes off them.
What the expectation of an accepted row must hold is the lowest code an encode can produce, not code 0: the reference clamps Y at 1e-4
(black_code), and a Lu'v' source cannot reach a YCbCr target's black at all (plane_row_informative)."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support import light_level as ll
from tests.support import measuring as ms
from tests.support import plane_kernels as pk
from tests.support.host import float_to_half_np, plane_rows, plane_samples, widen_halves
from tests.support.transcode_half import box

NF = fk.NF
PQ, LOG, LINEAR = 1, 2, 4
LUV, YCC = fk.LUV, fk.YCC
S1 = (PQ, 13, LUV, 12, 1e4, 0.005)
S2 = (PQ, 12, YCC, 12, 1000.0, 0.01)
S3 = (LINEAR, 14, LUV, 9, 1e4, 0.005)
S4 = (PQ, 9, YCC, 9, 1000.0, 0.01)
S5 = (PQ, 6, LUV, 5, 1e4, 0.005)
S6 = (PQ, 11, LUV, 16, 1e4, 0.005)
S7 = (PQ, 11, YCC, 10, 1000.0, 0.01)
S8 = (PQ, 13, YCC, 12, 1000.0, 0.01)
SINGLES = collections.OrderedDict([("S1", S1), ("S2", S2), ("S3", S3), ("S4", S4), ("S5", S5), ("S6", S6), ("S7", S7), ("S8", S8)])
PQ12_8, PQ12_10, PQ12_11, PQ12_12 = ((PQ, 12, LUV, cb, 1e4, 0.005) for cb in (8, 10, 11, 12))
PQ13_8 = (PQ, 13, LUV, 8, 1e4, 0.005)
PAIRS = collections.OrderedDict([
    ("P1", (PQ12_8, PQ13_8)), ("P2", (PQ12_10, PQ13_8)), ("P3", (PQ12_12, PQ13_8)), ("P3b", (PQ12_11, PQ13_8)),
    ("P4", (S2, (LOG, 12, LUV, 8, 1e4, 0.005))), ("P5", (S2, PQ12_8)), ("P6", (PQ12_8, S2)), ("P7a", (PQ12_8, (LINEAR, 14, LUV, 8, 1e4, 0.005))),
    ("P7b", (pk.PQ10_YCC, (LINEAR, 13, LUV, 8, 1e4, 0.005))), ("P8", (S4, (PQ, 9, LUV, 9, 1000.0, 0.01))),
    ("P9", (S6, (PQ, 11, LUV, 8, 1e4, 0.005)))])
FRAME_SIZES = ((64, 32), (258, 6))
PLANE_SIZES = ((264, 70), (258, 6))
HALF_SIZES = ((264, 72), (268, 76))
PROFILE_PAIRS = ((2, 2), (3, 2), (2, 3))
FRAME_CALLS = ("encode", "decode", "distortion", "distortion_map", "moments_map", "light")
PLANE_FAMILIES = pk.FAMILIES + ("half",)
BLOCKS = {"distortion": (None,), "distortion_map": (16, 64), "moments_map": (8, 64)}
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_enc", 2), ("block", 64))}

# ---- the LDS arithmetic of the host code, restated
BUDGET = 160 * 1024                 # lumahip_internal.hpp LUMAHIP_LDS_PER_WORKGROUP
TABLE_MAX = 144 * 1024              # lumahip_internal.hpp LUMAHIP_LDS_TABLE_MAX_DEFAULT
POWF_SMALL = 16 * 2 * 8 + 32 * 8    # pow_glibc.hpp PowfTables
POWF_WIDE = POWF_SMALL + 2048 * 16 + 22 * 16 * 16 + 16 * 16   # pow_glibc.hpp PowfTablesWide: + wide, foldA (FOLD_A_LEN = 22 * 16), foldC
HALF_BYTES = ((0x7C00 + 1) * 4 + 15) & ~15                    # luma_kernels.hpp lds_half_bytes
MEET = {"distortion": 16 * 8, "distortion_map": 16 * 12 * 8, "moments_map": 32 * 15 * 8, "light": 8 * 8, "transcode": 0, "half": 0}
#                                     lumahip_internal.hpp MeasureOut::lds_bytes: the static LDS of the measuring kernels
BIG = 53 * 1024                     # lumahip_launch.hip block_threads_for: beyond it 1024 threads
# Record counts of the tables, computed on the CPU (tests/test_config_edges_host.py recomputes every one with lumahip_build_lut and
# lumahip_thresh_index_host / lumahip_lin_index_host / lumahip_ycbcr_luma_index_host).  Key: (kind, ptf, bits, maxLum)
RECORDS = {("thresh", PQ, 13, 1e4): 34946, ("thresh", PQ, 13, 1000.0): 35022,("thresh", PQ, 12, 1e4): 16531, ("thresh", PQ, 12, 1000.0): 16592, ("thresh", LOG, 12, 1e4): 10722,
           ("thresh", PQ, 11, 1e4): 7834, ("thresh", PQ, 11, 1000.0): 7848, ("thresh", PQ, 10, 1000.0): 3700, ("thresh", PQ, 9, 1000.0): 1744,
           ("thresh", PQ, 6, 1e4): 177, ("thresh", LINEAR, 13, 1e4): 114689, ("thresh", LINEAR, 14, 1e4): 245761,
           ("lin", LINEAR, 13, 1e4): 8209, ("lin", LINEAR, 14, 1e4): 16418,
           ("composite", PQ, 12, 1000.0): 16346, ("composite", PQ, 11, 1000.0): 8177, ("composite", PQ, 10, 1000.0): 4085,
           ("composite", PQ, 9, 1000.0): 2039}


def round16(b):
    return (b + 15) & ~15


def _records(kind, cfg):
    return RECORDS[(kind, cfg[0], cfg[1], cfg[4])]


def lut_bytes(cfg):
    """lumahip_internal.hpp lut_lds_bytes / luma_kernels.hpp lds_lut_bytes: the table and its NaN padding up to a multiple of four
    floats (lumahip_core.hip upload_decode_tables lut_floats)"""
    return round16((((1 << cfg[1]) + 1 + 3) & ~3) * 4)


def col_bytes(cfg):
    """maxC + 1 floats: the u'v' table, or one chroma-term table (lumahip_launch.hip:28-30, luma_kernels.hpp lds_quant_bytes `col`)"""
    return round16((1 << cfg[3]) * 4)


def _fits(words, powf):
    """lumahip_core.hip records_fit_lds"""
    return words * 4 <= TABLE_MAX and words * 4 + 16 + powf <= BUDGET


def search(cfg):
    """(search mode, records' bytes in LDS or 0, composite records' bytes or 0): lumahip_core.hip ensure_search_index -- float-bit
    records in LDS when they fit (3), else value-keyed pairs for an evenly spaced table (7), else the records in global memory (4);
    YCbCr in mode 3: the composite records when they fit"""
    powf = POWF_WIDE if cfg[2] == YCC else 0
    n = _records("thresh", cfg)
    if _fits(n, powf):
        comp = _records("composite", cfg) if cfg[2] == YCC else 0
        return 3, round16(n * 4), (round16(comp * 4) if comp and _fits(comp, powf) else 0)
    if cfg[0] == LINEAR and _fits(2 * _records("lin", cfg), powf):
        return 7, round16(_records("lin", cfg) * 8), 0
    return 4, 0, 0


def encode_lds(cfg, ycode=False, half=False):
    """lumahip_launch.hip lds_bytes(c, true, cs, ycode, half): the records, or the composite records; the wide powf tables for YCbCr,
    or, with the half-input table, that table and the small ones"""
    mode, rec, comp = search(cfg)
    b = comp if ycode else rec
    if ycode and half:
        return b + HALF_BYTES + POWF_SMALL
    return b + (POWF_WIDE if cfg[2] == YCC else 0)


def half_table_fits(cfg):
    """lumahip_core.hip lumahip_half_table_info / lumahip_encode.hip:146"""
    return cfg[2] == YCC and search(cfg)[2] > 0 and encode_lds(cfg, True, True) <= BUDGET


def lut_in_lds(cfg):
    """lumahip_core.hip upload_decode_tables (:400)"""
    b, powf = ((1 << cfg[1]) + 4) * 4, POWF_WIDE if cfg[2] == YCC else 0
    return cfg[3] <= 12 and b <= max(TABLE_MAX, 16 * 1024 + 16) and b + (4 << cfg[3]) + 64 + powf <= BUDGET


def has_ytab(cfg):
    """lumahip_core.hip upload_decode_tables (:404-412), for a table of finite non-negative values"""
    return cfg[2] == YCC and lut_in_lds(cfg) and 2 * round16(((1 << cfg[1]) + 4) * 4) + (8 << cfg[3]) + 64 + POWF_WIDE <= BUDGET


def decode_lds(cfg):
    """lumahip_launch.hip lds_bytes(c, false, cs): [powf][table][u'v' table | y table, two chroma-term tables]"""
    b = 0
    if lut_in_lds(cfg):
        b += lut_bytes(cfg)
        if cfg[2] == LUV:
            b += col_bytes(cfg)
        if has_ytab(cfg):
            b += lut_bytes(cfg) + 2 * col_bytes(cfg)
    return b + (POWF_WIDE if cfg[2] == YCC else 0)


def source_taken(scfg):
    """lumahip_transcode.hip:57-62 / lumahip_light_level.hip:106-110: the table staged in LDS, luminance depth up to 12, a y table"""
    return scfg[1] <= 12 and lut_in_lds(scfg) and (scfg[2] != YCC or has_ytab(scfg))


def pair_lds(scfg, dcfg):
    """lumahip_transcode.hip:72-75 transcode_plan: [powf once][source: table + u'v' table | + y table + two chroma-term tables][target:
    records]; None where the target has no records in LDS (:67)"""
    mode, rec, comp = search(dcfg)
    tgt = comp if dcfg[2] == YCC else (rec if mode in (3, 7) else 0)
    if not tgt:
        return None
    src = lut_bytes(scfg) + (lut_bytes(scfg) + 2 * col_bytes(scfg) if scfg[2] == YCC else col_bytes(scfg))
    return (POWF_WIDE if YCC in (scfg[2], dcfg[2]) else 0) + src + tgt


def pair_accepted(family, scfg, dcfg):
    """lumahip_transcode.hip:57-80"""
    lds = pair_lds(scfg, dcfg)
    return source_taken(scfg) and lds is not None and lds + MEET[family] <= BUDGET


def target_lm(dcfg):
    return 5 if dcfg[2] == YCC else search(dcfg)[0]


def light_accepted(cfg):
    """lumahip_light_level.hip:106-113"""
    return source_taken(cfg) and cfg[3] <= 12 and decode_lds(cfg) + MEET["light"] <= BUDGET


def measuring_lm(cfg, in16, family):
    """(LM, LDS bytes of the tables) of a frame-fed measuring launch, or None for a refusal: lumahip_distortion.hip:40-56"""
    mode, rec, comp = search(cfg)
    if mode not in (3, 7):
        return None
    meet = MEET[family]
    if in16 and comp and encode_lds(cfg, True, True) + meet <= BUDGET:
        lm, lds = 6, encode_lds(cfg, True, True)
    elif not in16 and comp:
        lm, lds = 5, encode_lds(cfg, True)
    else:
        lm, lds = mode, encode_lds(cfg)
    return (lm, lds) if lds + meet <= BUDGET else None


# ---- rows
FrameRow = collections.namedtuple("FrameRow", "id sid cfg call profile w h sc")
PlaneRow = collections.namedtuple("PlaneRow", "id pid family scfg dcfg sp dp w h src_sc dst_sc")


def frame_sc(cfg, w):
    """the preScaling of a frame-fed row: 1 for Lu'v'; YCbCr 20 at 64x32 and 1 at 258x6"""
    return 1.0 if cfg[2] != YCC else 20.0 if w == 64 else 1.0


def frame_rows():
    out = []
    for sid, cfg in SINGLES.items():
        for call in FRAME_CALLS:
            for profile in ((0, 1) if sid == "S5" else (2, 3)):
                for (w, h) in FRAME_SIZES:
                    out.append(FrameRow("%s-%s-p%d-%dx%d" % (sid, call, profile, w, h), sid, cfg, call, profile, w, h, frame_sc(cfg, w)))
    return out


def scalings(scfg, dcfg):
    if scfg[2] != YCC:
        return pk.scalings(scfg[2], dcfg[2], target_lm(dcfg))
    if dcfg[2] == YCC:
        return [(1.0, 20.0), (20.0, 20.0)]
    r = 1.25 * dcfg[4] / scfg[4]
    return [(1.0, r), (20.0, 20.0 * r)]


def plane_rows_all():
    out = []
    for pid, (scfg, dcfg) in PAIRS.items():
        for family in PLANE_FAMILIES:
            for (sp, dp) in PROFILE_PAIRS:
                for (w, h) in (HALF_SIZES if family == "half" else PLANE_SIZES):
                    for (src_sc, dst_sc) in scalings(scfg, dcfg):
                        out.append(PlaneRow("%s-%s-p%d-p%d-%dx%d-sc%g" % (pid, family, sp, dp, w, h, src_sc), pid, family, scfg, dcfg, sp, dp, w, h,
                                            src_sc, dst_sc))
    return out


def row_accepted(row):
    """derived from the sums and the budget, never listed"""
    if isinstance(row, PlaneRow):
        return pair_accepted(row.family, row.scfg, row.dcfg)
    if row.call in ("encode", "decode"):
        return True
    if row.call == "light":
        return light_accepted(row.cfg)
    return measuring_lm(row.cfg, False, row.call) is not None or measuring_lm(row.cfg, True, row.call) is not None


def row_lds(row):
    """the bytes of tables the row's (float) launch stages, for the rows that run again under other launch shapes"""
    if isinstance(row, PlaneRow):
        return pair_lds(row.scfg, row.dcfg)
    if row.call == "encode":
        return max(encode_lds(row.cfg), encode_lds(row.cfg, search(row.cfg)[2] > 0))
    if row.call in ("decode", "light"):
        return decode_lds(row.cfg)
    return measuring_lm(row.cfg, False, row.call)[1]


def big(row):
    return row_accepted(row) and row_lds(row) > BIG


# ---- inputs
EDGE_ROWS, EDGE_COLS, EDGE_AT = 8, 16, 16        # the corner of every frame that goes round both ends of every table: luma columns 16 .. 31


def edge_codes(cfg, p):
    top = (1 << (cfg[1] if p == 0 else cfg[3])) - 1
    return [0, 1, 2, 3, top - 3, top - 2, top - 1, top]


def grey_code(cfg):
    """the colour code nearest (224 * 0 + 128) / 255"""
    return int(round(((1 << cfg[3]) - 1) * 128.0 / 255.0))


_src = {}


def source_planes(cfg, profile, w, h):
    """NF distinct frames of code planes, each three (rows, row bytes) arrays: pk.source_planes' seeded random in-range codes (and, at
    264x70, its planted out-of-range codes in luma columns 0 .. 15), and in luma rows 0 .. 7, columns 16 .. 31 of every frame the
    codes 0 .. 3 and top - 3 .. top of the plane going round, frame f starting at the f-th.  Made once per key, read-only"""
    key = (cfg, profile, w, h)
    if key not in _src:
        frames, bps = [], 2 if profile > 1 else 1
        for f in range(NF):
            rng = np.random.default_rng([7, cfg[0], cfg[1], cfg[2], cfg[3], profile, w, h, f])
            fr = []
            for p in range(3):
                rows, rb = plane_rows(w, h, profile, p)
                bits = cfg[1] if p == 0 else cfg[3]
                assert bits <= 8 * bps, (cfg, profile, "the samples do not hold the codes")
                v = rng.integers(0, 1 << bits, size=(rows, rb // bps))
                sub = 2 if (p and profile in (0, 2)) else 1
                if (w, h) == pk.SIZES[0]:
                    cr, cc = pk.PLANTED[0] // sub, pk.PLANTED[1] // sub
                    v[:cr, :cc] = np.resize(np.roll(pk.planted_codes(cfg, profile, p), f), cr * cc).reshape(cr, cc)
                er, c0, ec = min(EDGE_ROWS // sub, rows), EDGE_AT // sub, EDGE_COLS // sub
                which = (np.arange(ec)[None, :] // 2 + 4 * (np.arange(er)[:, None] // 2) + f) % 8      # 2x2 cells of one code: the half-size box keeps them
                v[:er, c0:c0 + ec] = np.asarray(edge_codes(cfg, p))[which]
                if cfg[2] == YCC:       # a YCbCr pixel is as bright as its luma code says only when it is grey
                    v[:er, c0 + ec:c0 + 2 * ec] = np.asarray(edge_codes(cfg, p))[which] if p == 0 else grey_code(cfg)
                a = np.ascontiguousarray(v.astype("<u2" if bps == 2 else np.uint8)).view(np.uint8).reshape(rows, rb)
                a.setflags(write=False)
                fr.append(a)
            frames.append(fr)
        _src[key] = frames
    return _src[key]


def lut_of(o, cfg):
    return fk.oracle(o, cfg).mapping


_frames = {}


def frames(o, cfg, w, h, sc, halves=False):
    """fk.frames' log-uniform frames (special_frame in the corner of 64x32) and, in the last row of every frame, four grey pixels above
    the table's largest value and four below its smallest positive one (two of them zero), as the quantizer sees them after the
    preScaling.  halves: the same narrowed to binary16"""
    key = (cfg, w, h, sc, halves)
    if key not in _frames:
        lut = lut_of(o, cfg)
        a = np.array(fk.frames(w, h), copy=True)
        above = np.float32(min(4.0 * float(lut[-1]) / sc, 6.0e4))
        below = np.float32(float(lut[lut > 0][0]) / (4.0 * sc))
        for f in range(NF):
            a[f, :, h - 1, 8 * f:8 * f + 4] = above
            a[f, :, h - 1, 8 * f + 4:8 * f + 8] = (below, below, 0, 0)      # (YCbCr tells the smallest positive values from black)
        with np.errstate(over="ignore"):
            a = a.astype(np.float16) if halves else a
        a.setflags(write=False)
        _frames[key] = a
    return _frames[key]


# ---- expectations
def _decode(orc, planes, w, h, sc, profile):
    st = [plane_rows(w, h, profile, p)[1] for p in range(3)]
    with np.errstate(all="ignore"):
        return np.stack([orc.decode(fr, st, w, h, sc, profile) for fr in planes])


def _encode(orc, d, sc, profile):
    return [orc.encode(np.array(d[f], dtype=np.float32, copy=True), sc, profile)[0] for f in range(len(d))]


def _frozen(*arrays):
    for a in arrays:
        for x in (a if isinstance(a, list) else [a]):
            for y in (x if isinstance(x, list) else [x]):
                y.setflags(write=False)


FrameExpect = collections.namedtuple("FrameExpect", "frames e s d")
_fexp = {}


def frame_expected(o, cfg, profile, w, h, sc, halves=False):
    """The inputs of a frame-fed launch and what the oracle makes of them, once per key and read-only:
    frames  `frames` (halves: binary16)           e  the ORACLE's planes of them (halves: of the widened halves)
    s       source_planes(cfg, profile, w, h)     d  the ORACLE's decode of s: (NF, 3, h, w) float32"""
    key = (cfg, profile, w, h, sc, halves)
    if key not in _fexp:
        fr = frames(o, cfg, w, h, sc, halves)
        e = _encode(fk.oracle(o, cfg), widen_halves(fr) if halves else fr, sc, profile)
        s = source_planes(cfg, profile, w, h)
        d = _decode(fk.oracle(o, cfg), s, w, h, sc, profile)
        _frozen(e, d)
        _fexp[key] = FrameExpect(fr, e, s, d)
    return _fexp[key]


PlaneExpect = collections.namedtuple("PlaneExpect", "s d e")
_pexp = {}


def plane_expected(o, row):
    """as pk.expected (half: as tests/support/transcode_half.py expected, the 2x2 box in between) on this module's source planes"""
    key = (row.family == "half", row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc)
    if key not in _pexp:
        s = source_planes(row.scfg, row.sp, row.w, row.h)
        d = _decode(fk.oracle(o, row.scfg), s, row.w, row.h, row.src_sc, row.sp)
        e = _encode(fk.oracle(o, row.dcfg), box(d) if row.family == "half" else d, row.dst_sc, row.dp)
        _frozen(e, d)
        _pexp[key] = PlaneExpect(s, d, e)
    return _pexp[key]


def target_size(row):
    return (row.w // 2, row.h // 2) if row.family == "half" else (row.w, row.h)


_given = {}


def given(o, row, block, halves=False):
    """ms.given_from on the row's expected planes: (g, words, dist, dmap), once per key"""
    key = (row, block, halves)
    if key not in _given:
        if isinstance(row, PlaneRow):
            e, (w, h), profile, family = plane_expected(o, row).e, target_size(row), row.dp, row.family
        else:
            e, (w, h), profile, family = frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc, halves).e, (row.w, row.h), row.profile, row.call
        rng = np.random.default_rng([11, len(row.id), sum(row.id.encode()), block or 0, int(halves)])
        _given[key] = ms.given_from(rng, family, e, w, h, profile, block)
    return _given[key]


def plane_row_informative(o, row):
    """luma_informative on the expectation of an accepted plane-fed row.  A Lu'v' source decodes no pixel below X = Y = Z = 1e-4, which a
    YCbCr target tells from black (and how dark its luma gets depends on the chroma): that pair is not asked for the lowest code"""
    tw, th = target_size(row)
    luma_informative(o, plane_expected(o, row).e, tw, th, row.dp, row.dcfg, row.dst_sc, (row.id,), not (row.scfg[2] == LUV and row.dcfg[2] == YCC))


def narrowed(d):
    return float_to_half_np(d).reshape(np.shape(d))


_black = {}


def black_code(o, cfg, sc):
    """the lowest luminance code an encode under cfg produces: the reference's transform clamps Y at 1e-4 (Lu'v') and starts its luma at
    16 / 255 (YCbCr), so no input comes below the code of a black pixel, whatever lies under it in the table"""
    if (cfg, sc) not in _black:
        pl = fk.oracle(o, cfg).encode(np.zeros((3, 8, 16), dtype=np.float32), sc, 3 if cfg[1] > 8 else 1)[0]
        _black[(cfg, sc)] = int(plane_samples(pl[0], 16, 8, 3 if cfg[1] > 8 else 1, 0)[0, 0])
    return _black[(cfg, sc)]


def luma_informative(o, e, w, h, profile, cfg, sc, tag, black=True):
    """asserted on the oracle's planes alone: every frame's luma plane holds the lowest code an encode produces (black_code) and the
    table's largest code and at least 64 distinct values (a table of fewer: every code from black_code up), U differs from V, the frames
    differ pairwise.  black=False: the lowest code is out of the row's reach and not asked for"""
    top, low = (1 << cfg[1]) - 1, black_code(o, cfg, sc)
    for f, pl in enumerate(e):
        y = plane_samples(pl[0], w, h, profile, 0)
        assert (y.min() == low or not black) and y.max() == top, tag + (f, "luma codes %d .. %d, an encode produces %d .. %d" % (y.min(), y.max(), low, top))
        n = np.unique(y).size
        assert n >= min(fk.MIN_DISTINCT, top + 1 - low), tag + (f, "%d distinct luma codes" % n)
        assert not np.array_equal(plane_samples(pl[1], w, h, profile, 1), plane_samples(pl[2], w, h, profile, 2)), tag + (f, "U and V are the same")
        for g in range(f + 1, len(e)):
            assert any(not np.array_equal(pl[p], e[g][p]) for p in range(3)), tag + (f, g, "two frames with the same planes")


# ---- wrong kernels, modelled with the oracle and numpy alone
DECODE_SIDE = ("lut_end_zero", "colour_end_zero", "colour_shifted", "y_table_exchanged")
WRONG = DECODE_SIDE + ("records_top_lost",)


def _pq(v, lmax, encode):
    """the reference's PQ pair in float32 (a model's table needs no more than that)"""
    m, n, c1, c2, c3 = (np.float32(x) for x in (78.8438, 0.1593, 0.8359, 18.8516, 18.6875))
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        if encode:
            lp = np.power(v / np.float32(lmax), n)
            return np.power((c1 + c2 * lp) / (1 + c3 * lp), m)
        vp = np.power(v, np.float32(1.0) / m)
        return np.float32(lmax) * np.power(np.maximum(np.float32(0), vp - c1) / (c2 - c3 * vp), np.float32(1.0) / n)


def _colour_mapped(planes, cfg, profile, fn):
    """source planes with fn applied to the in-range codes of both colour planes"""
    top, out = (1 << cfg[3]) - 1, []
    for fr in planes:
        new = [fr[0]]
        for p in (1, 2):
            v = pk.plane_values(fr[p], profile)
            inr = v <= top
            v = np.where(inr, fn(v, top), v)
            new.append(np.ascontiguousarray(v.astype("<u2" if profile > 1 else np.uint8)).view(np.uint8).reshape(fr[p].shape))
        out.append(new)
    return out


def _with_table(o, cfg, table):
    """an oracle of its own for cfg whose table is `table`"""
    orc = o.Oracle(*cfg)
    orc.overwrite_mapping(table)
    return orc


def wrong_decodes(o, cfg, planes, profile, w, h, sc):
    """{name: (NF, 3, h, w) frames}: what decode sides with one fault each make of these source planes
    lut_end_zero       the last 16 bytes of the luminance table (YCbCr: and of the y table made of it) read as zero: the oracle on a
                       copy of the table with its last four entries zeroed
    colour_end_zero    the last four entries of the u'v' table, or of both chroma-term tables, read as zero: colour codes maxC - 3 .. maxC
                       decode as the code of a zero entry (Lu'v': 0, which is 1e-10 * 255 / 410; YCbCr: the code nearest maxC * 128 / 255)
    colour_shifted     the colour table read one 16-byte piece too far: colour code c decodes as c + 4 (up to maxC - 4)
    y_table_exchanged  YCbCr: the kernel takes luminance-table entries for y: the oracle on the table whose y table is that table"""
    lut = np.array(lut_of(o, cfg), copy=True)
    zeroed = np.array(lut, copy=True)
    zeroed[-4:] = 0
    out = {"lut_end_zero": _decode(_with_table(o, cfg, zeroed), planes, w, h, sc, profile)}
    orc = fk.oracle(o, cfg)
    zero = 0 if cfg[2] == LUV else int(round(((1 << cfg[3]) - 1) * 128.0 / 255.0))
    out["colour_end_zero"] = _decode(orc, _colour_mapped(planes, cfg, profile, lambda v, top: np.where(v >= top - 3, zero, v)), w, h, sc, profile)
    out["colour_shifted"] = _decode(orc, _colour_mapped(planes, cfg, profile, lambda v, top: np.where(v <= top - 4, v + 4, v)), w, h, sc, profile)
    if cfg[2] == YCC:
        as_y = _pq(np.minimum(np.float32(1), (np.float32(219) * lut + np.float32(16)) / np.float32(255)), cfg[4], False)
        out["y_table_exchanged"] = _decode(_with_table(o, cfg, as_y), planes, w, h, sc, profile)
    return out


def records_top_lost(e, w, h, profile, cfg):
    """the top of the records lost: the target's largest code is never produced -- expected luma codes equal to maxVal become maxVal - 1"""
    top, out = (1 << cfg[1]) - 1, []
    for fr in e:
        y = np.array(fr[0], copy=True)
        rows, rb = plane_rows(w, h, profile, 0)
        v = plane_samples(fr[0], w, h, profile, 0)
        v = np.where(v == top, top - 1, v)
        y[:rows, :rb] = np.ascontiguousarray(v.astype("<u2" if profile > 1 else np.uint8)).view(np.uint8).reshape(rows, rb)
        out.append([y, fr[1], fr[2]])
    return out


def _planes_differ(a, b, w, h, profile):
    return any(not np.array_equal(plane_samples(a[f][p], w, h, profile, p), plane_samples(b[f][p], w, h, profile, p)) for f in range(len(a)) for p in range(3))


def _frames_differ(a, b):
    return not np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def wrong_results(o, row, halves=False):
    """{name: what the row compares} for every modelled wrong kernel that applies to the row -- decoded frames (decode), light-level words
    (light), or planes (every other row): the models of the decode side for rows that decode, records_top_lost for rows that encode"""
    if isinstance(row, PlaneRow):       # (the planes of a pair serve its four full-size families)
        key = ("planes", row.family == "half") + tuple(row[3:])
    else:
        key = ("frames", row.call in ("decode", "light"), row.cfg, halves) + tuple(row[4:])
    if key not in _wrong:
        _wrong[key] = _wrong_planes(o, row, halves)
    if isinstance(row, FrameRow) and row.call == "light":
        return {name: ll.model_frames(d, 1.0) for name, d in _wrong[key].items()}
    return _wrong[key]


_wrong = {}


def _wrong_planes(o, row, halves):
    out = {}
    if isinstance(row, PlaneRow):
        ex, enc = plane_expected(o, row), fk.oracle(o, row.dcfg)
        tw, th = target_size(row)
        for name, d in wrong_decodes(o, row.scfg, ex.s, row.sp, row.w, row.h, row.src_sc).items():
            out[name] = _encode(enc, box(d) if row.family == "half" else d, row.dst_sc, row.dp)
        out["records_top_lost"] = records_top_lost(ex.e, tw, th, row.dp, row.dcfg)
        return out
    ex = frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc, halves)
    if row.call in ("decode", "light"):
        return wrong_decodes(o, row.cfg, ex.s, row.profile, row.w, row.h, row.sc)
    return {"records_top_lost": records_top_lost(ex.e, row.w, row.h, row.profile, row.cfg)}


def expected_names(row):
    if isinstance(row, PlaneRow):
        return set(WRONG) - (set() if row.scfg[2] == YCC else {"y_table_exchanged"})
    if row.call in ("decode", "light"):
        return set(DECODE_SIDE) - (set() if row.cfg[2] == YCC else {"y_table_exchanged"})
    return {"records_top_lost"}


def tells(o, row, result, block=None, halves=False):
    """whether the row's comparison fails for a kernel that comes to `result` (as wrong_results gives it)"""
    if isinstance(row, PlaneRow):
        ex, (w, h), profile, family = plane_expected(o, row), target_size(row), row.dp, row.family
    else:
        ex, (w, h), profile, family = frame_expected(o, row.cfg, row.profile, row.w, row.h, row.sc, halves), (row.w, row.h), row.profile, row.call
    if family == "decode":
        return _frames_differ(narrowed(result), narrowed(ex.d)) if halves else _frames_differ(result, ex.d)
    if family == "light":
        return not np.array_equal(result, ll.model_frames(ex.d, 1.0))
    if family in ("encode", "transcode", "half"):
        return _planes_differ(result, ex.e, w, h, profile)
    gv = given(o, row, block, halves)
    return not np.array_equal(ms.words_of(family, result, gv[0], w, h, profile, block), gv[1])
