"""What tests/test_gpu_transcode_quarter.py and tests/test_transcode_quarter_host.py share, numpy and the oracle alone: the model of
lumahip_transcode_quarter_frames_device (include/lumahip_rungs.h) -- the ORACLE's decode of the source planes, numpy's float32 2x2 box
of tests/support/transcode_half.py applied twice, the ORACLE's encode of the result under the target configuration --, the matrix of
the call and the k_transcode_quarter instantiations it launches, and wrong kernels modelled the same way, which every row's inputs
must tell from the right one.  The matrix is the half-resolution one's with the source sizes doubled: the targets are the same.

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only."""
import numpy as np

from tests.support import frame_kernels as fk
from tests.support import plane_kernels as pk
from tests.support import transcode_half as th
from tests.support.host import plane_rows
from tests.support.transcode_half import Expect, Row, box

NF = th.NF
# source sizes: target 132x36, VW 4, several tile rows / target 260x6, VW 4, past one 256-pixel tile column / target 134x38, VW 2, past
# one 128-pixel tile column / target 4x2, one VW 4 unit / target 2x2, one VW 2 unit: the smallest legal frame
SIZES = [(528, 144), (1040, 24), (536, 152), (16, 8), (8, 8)]
ORDER_SIZES = (SIZES[0], SIZES[2])      # where the Lu'v' -> Lu'v' rows must also tell the association from two others
PROFILES = th.PROFILES


def quarter_matrix():
    """th.half_matrix() with every source size doubled (ids renamed), and behind it, per (source, target), one row of the smallest legal
    frame, 8 x 8, which the half matrix has no counterpart of"""
    out = []
    for r in th.half_matrix():
        w, h = 2 * r.w, 2 * r.h
        out.append(r._replace(id=_ident(r, w, h), w=w, h=h))
    n = 0
    for csd in pk.SOURCES:
        for (cse, lm) in pk.TARGETS:
            sp, dp = ((2, 2), (3, 3), (2, 3), (3, 2))[n % 4]
            src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
            (w, h) = SIZES[4]
            r = Row("", csd, cse, lm, pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp), sp, dp, w, h, src_sc, dst_sc, n % 2 == 0, False)
            out.append(r._replace(id=_ident(r, w, h)))
            n += 1
    return out


def _ident(r, w, h):
    return "quarter-%s-%s-%s-p%d-p%d-%dx%d-sc%g" % (fk.SPACES[r.csd][0], fk.SPACES[r.cse][0], "pq8" if r.eight else "lm%d" % r.lm, r.sp, r.dp, w, h,
                                                    r.src_sc)


def kernel_of(row):
    """(CSD, SUBD, CSE, SUBE, VW, LM) of the k_transcode_quarter this row's call launches (lumahip_pick.hpp pick_planes), both plane sets
    aligned for units of four samples: transcode_plan takes four pixels per thread where the TARGET's width is a multiple of 4"""
    return (row.csd, row.sp in (0, 2), row.cse, row.dp in (0, 2), 4 if (row.w // 4) % 4 == 0 else 2, row.lm)


# ---- the model
_exp = {}


def expected(o, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc):
    """The inputs of a launch and the model's outputs, computed once per key and not written to afterwards:
    s   pk.source_planes(scfg, sp, w, h): NF frames
    d   the ORACLE's decode of them under the source configuration: (NF, 3, h, w) floats
    m   box(box(d)): (NF, 3, h/4, w/4) floats
    e   the ORACLE's encode of m under the target configuration, per frame three (rows, stride) arrays of (w/4) x (h/4)"""
    key = (scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
    if key not in _exp:
        s = pk.source_planes(scfg, sp, w, h)
        st = [plane_rows(w, h, sp, p)[1] for p in range(3)]
        d = np.stack([fk.oracle(o, scfg).decode(s[f], st, w, h, src_sc, sp) for f in range(NF)])
        m = box(box(d))
        e = [fk.oracle(o, dcfg).encode(m[f].copy(), dst_sc, dp)[0] for f in range(NF)]
        for a in [d, m] + [p for fr in e for p in fr]:
            a.setflags(write=False)
        _exp[key] = Expect(s, d, m, e)
    return _exp[key]


def expected_of(o, row):
    return expected(o, row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc)


# ---- wrong kernels, modelled with the oracle and numpy alone
WRONG_KERNELS = ("top_left", "top_left_2x2")
WRONG_ORDERS = ("raster", "rows")


def wrong_frame(d, name):
    """what a kernel with one fault makes of a decoded (3, h, w) frame in the place of box(box(d))"""
    d = np.asarray(d, dtype=np.float32)
    s = [[d[..., y::4, x::4] for x in range(4)] for y in range(4)]      # s[y][x]: source pixel (4X + x, 4Y + y)
    q = np.float32(1.0 / 16.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if name == "top_left":
            m = s[0][0]
        elif name == "top_left_2x2":
            m = box(d)[..., 0::2, 0::2]
        elif name == "raster":
            acc = s[0][0]
            for k in range(1, 16):
                acc = acc + s[k // 4][k % 4]
            m = acc * q
        elif name == "rows":
            r = [(s[y][0] + s[y][1]) + (s[y][2] + s[y][3]) for y in range(4)]
            m = ((r[0] + r[1]) + (r[2] + r[3])) * q
        else:
            raise ValueError(name)
    assert m.dtype == np.float32, "the wrong kernel's average left fp32"
    return np.ascontiguousarray(m)


def luma_differences(o, row, name, f=0):
    """in how many luma samples of frame f the planes of the wrong kernel or wrong order `name` differ from the model's"""
    ex = expected_of(o, row)
    planes = fk.oracle(o, row.dcfg).encode(wrong_frame(ex.d[f], name).copy(), row.dst_sc, row.dp)[0]
    tw, t_h = row.w // 4, row.h // 4
    rows, rb = plane_rows(tw, t_h, row.dp, 0)
    return int(np.count_nonzero(pk.plane_values(np.asarray(planes[0])[:rows, :rb], row.dp) != pk.plane_values(np.asarray(ex.e[f][0])[:rows, :rb], row.dp)))


__all__ = ["NF", "ORDER_SIZES", "PROFILES", "SIZES", "WRONG_KERNELS", "WRONG_ORDERS", "Expect", "Row", "box", "expected", "expected_of",
           "kernel_of", "luma_differences", "quarter_matrix", "wrong_frame"]
