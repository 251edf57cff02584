"""What tests/test_gpu_transcode_half.py and tests/test_transcode_half_host.py share, numpy and the oracle alone: the model of
lumahip_transcode_half_frames_device -- the ORACLE's decode of the source planes, numpy's float32 2x2 box in the specified
association, the ORACLE's encode of the result under the target configuration --, the matrix of the call and the k_transcode_half
instantiations it launches, and wrong kernels modelled the same way, which every row's inputs must tell from the right one.  The
source planes, the configurations of both sides and the preScalings are tests/support/plane_kernels.py's.

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support import plane_kernels as pk
from tests.support.host import plane_rows

NF = pk.NF
# source sizes: VW 4, several tile rows / VW 4, target 260 wide: past one tile column / target 134 wide: VW 2, past one tile column /
# one unit
SIZES = [(264, 72), (520, 12), (268, 76), (8, 4)]
ORDER_SIZES = (SIZES[0], SIZES[2])      # where the Lu'v' -> Lu'v' rows must also tell the association from two others
PROFILES = pk.PROFILES
FAR_SIZE, FAR_PROFILES = SIZES[1], (2, 2)
EIGHT_BIT = tuple((pair, SIZES[0] if n < 2 else SIZES[2]) for n, (pair, _) in enumerate(pk.EIGHT_BIT))

Row = collections.namedtuple("Row", "id csd cse lm scfg dcfg sp dp w h src_sc dst_sc stats eight")


def _ident(csd, cse, lm, sp, dp, w, h, src_sc, eight=False):
    return "half-%s-%s-%s-p%d-p%d-%dx%d-sc%g" % (fk.SPACES[csd][0], fk.SPACES[cse][0], "pq8" if eight else "lm%d" % lm, sp, dp, w, h, src_sc)


def half_matrix():
    """Rows of (id, CSD, CSE, LM, source configuration, target configuration, sp, dp, w, h, src_sc, dst_sc, stats, eight): both sources
    by the three targets, (sp, dp) over {2, 3}^2 and the four source sizes, a YCbCr source with both preScalings of pk.scalings;
    `stats` on every other row.  Behind them, per (YCbCr source, target), one row with src_sc 3e5 and, per colour-space pair, the
    four 8-bit rows of EIGHT_BIT (LM 3 or 5)"""
    out, n = [], 0
    for csd in pk.SOURCES:
        for (cse, lm) in pk.TARGETS:
            for sp in PROFILES:
                for dp in PROFILES:
                    for (w, h) in SIZES:
                        for (src_sc, dst_sc) in pk.scalings(csd, cse, lm):
                            out.append(Row(_ident(csd, cse, lm, sp, dp, w, h, src_sc), csd, cse, lm, pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp),
                                           sp, dp, w, h, src_sc, dst_sc, n % 2 == 0, False))
                            n += 1
            if csd == fk.YCC:
                (w, h), (sp, dp) = FAR_SIZE, FAR_PROFILES
                src_sc, dst_sc = pk.far_scalings(cse, lm)
                out.append(Row(_ident(csd, cse, lm, sp, dp, w, h, src_sc), csd, cse, lm, pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp), sp, dp, w, h,
                               src_sc, dst_sc, False, False))
    for (csd, cse) in pk.PAIRS:
        lm = 5 if cse == fk.YCC else 3
        for k, ((sp, dp), (w, h)) in enumerate(EIGHT_BIT):
            src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
            out.append(Row(_ident(csd, cse, lm, sp, dp, w, h, src_sc, True), csd, cse, lm, pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp), sp, dp, w, h,
                           src_sc, dst_sc, k % 2 == 0, True))
    return out


def kernel_of(row):
    """(CSD, SUBD, CSE, SUBE, VW, LM) of the k_transcode_half this row's call launches (lumahip_pick.hpp pick_planes), both plane sets
    aligned for units of four samples: transcode_plan takes four pixels per thread where the TARGET's width is a multiple of 4"""
    return (row.csd, row.sp in (0, 2), row.cse, row.dp in (0, 2), 4 if (row.w // 2) % 4 == 0 else 2, row.lm)


# ---- the model
def box(d, order="spec"):
    """step 2 of the call on (..., h, w) float32: the 2x2 average in fp32 -- `spec` ((a + b) + (c + d)) * 0.25, a b the upper pair, c d
    the lower; the two orders a kernel may not take: `columns` ((a + c) + (b + d)), `sequential` (((a + b) + c) + d)"""
    d = np.asarray(d, dtype=np.float32)
    a, b, c, e = d[..., 0::2, 0::2], d[..., 0::2, 1::2], d[..., 1::2, 0::2], d[..., 1::2, 1::2]
    q = np.float32(0.25)
    with np.errstate(invalid="ignore", over="ignore"):
        if order == "spec":
            m = ((a + b) + (c + e)) * q
        elif order == "columns":
            m = ((a + c) + (b + e)) * q
        elif order == "sequential":
            m = (((a + b) + c) + e) * q
        else:
            raise ValueError(order)
    assert m.dtype == np.float32, "the model's average left fp32"
    return np.ascontiguousarray(m)


Expect = collections.namedtuple("Expect", "s d m e")
_exp = {}


def expected(o, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc):
    """The inputs of a launch and the model's outputs, computed once per key and not written to afterwards:
    s   pk.source_planes(scfg, sp, w, h): NF frames
    d   the ORACLE's decode of them under the source configuration: (NF, 3, h, w) floats
    m   box(d): (NF, 3, h/2, w/2) floats
    e   the ORACLE's encode of m under the target configuration, per frame three (rows, stride) arrays of (w/2) x (h/2)"""
    key = (scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
    if key not in _exp:
        s = pk.source_planes(scfg, sp, w, h)
        st = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        d = np.stack([fk.oracle(o, scfg).decode(s[f], st, w, h, src_sc, sp) for f in range(NF)])
        m = box(d)
        e = [fk.oracle(o, dcfg).encode(m[f].copy(), dst_sc, dp)[0] for f in range(NF)]
        for a in [d, m] + [p for fr in e for p in fr]:
            a.setflags(write=False)
        _exp[key] = Expect(s, d, m, e)
    return _exp[key]


def expected_of(o, row):
    return expected(o, row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc)


# ---- wrong kernels, modelled with the oracle and numpy alone
WRONG_KERNELS = ("top_left", "horizontal_pair", "vertical_pair")
WRONG_ORDERS = ("columns", "sequential")


def wrong_frame(d, name):
    """what a kernel with one fault makes of a decoded (3, h, w) frame in the place of box(d)"""
    a, b, c = d[..., 0::2, 0::2], d[..., 0::2, 1::2], d[..., 1::2, 0::2]
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "top_left":
            return np.ascontiguousarray(a)
        if name == "horizontal_pair":
            return np.ascontiguousarray((a + b) * np.float32(0.5))
        if name == "vertical_pair":
            return np.ascontiguousarray((a + c) * np.float32(0.5))
    return box(d, name)


def luma_differences(o, row, name, f=0):
    """in how many luma samples of frame f the planes of the wrong kernel or wrong order `name` differ from the model's"""
    ex = expected_of(o, row)
    planes = fk.oracle(o, row.dcfg).encode(wrong_frame(ex.d[f], name).copy(), row.dst_sc, row.dp)[0]
    tw, th = row.w // 2, row.h // 2
    rows, rb = plane_rows(tw, th, row.dp, 0)
    return int(np.count_nonzero(pk.plane_values(np.asarray(planes[0])[:rows, :rb], row.dp) != pk.plane_values(np.asarray(ex.e[f][0])[:rows, :rb], row.dp)))


__all__ = ["EIGHT_BIT", "NF", "ORDER_SIZES", "PROFILES", "SIZES", "WRONG_KERNELS", "WRONG_ORDERS", "Expect", "Row", "box", "expected", "expected_of",
           "half_matrix", "kernel_of", "luma_differences", "wrong_frame"]
