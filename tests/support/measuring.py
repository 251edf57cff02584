"""What tests/test_gpu_measuring_kernels.py and tests/test_measuring_kernels_host.py share, numpy and the oracle alone: the matrix of
the frame-fed measuring calls and the k_distortion / k_distortion_map / k_moments_map instantiations it launches, the given planes of
a launch -- the ORACLE's planes of the frames and a perturbed copy of them -- and numpy's words for the pair
(tests/support/host.py expected_distortion / expected_distortion_map, tests/support/moments.py expected_moments_map).

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support.host import (BLOCKS, GAP, expected_distortion, expected_distortion_map, layout, map_perturbed, perturb, plane_rows,
                                planes_from_frames)
from tests.support.moments import MOM_BLOCKS, expected_moments_map

FAMILIES = ("distortion", "distortion_map", "moments_map")
SIZES = [(264, 70), (258, 6), (6, 4)]       # four pixels per thread, several block columns and rows, ragged both ways, special_frame in
#                                             the corner / two pixels per thread with a ragged last tile / one tile
PROFILES = (2, 3)
FLOAT_FORMS, HALF_FORMS = ("packed", "planar"), ("f16", "planar_f16")
NO_COMPOSITE, NO_HALF_TABLE = (("ycbcr_tables", 0),), (("half_table", 0),)

Row = collections.namedtuple("Row", "id family cs lm cfg tunes in16 profile w h sc block form")


def contexts_of(cs, in16):
    """[(LM, configuration, tunes)]: how a context comes to each front end of a colour space (lumahip_distortion.hip distortion_plan,
    lumahip_core.hip ensure_search_index).  PQ-11 has its records in LDS (LM 3), LINEAR-12 the value-keyed ones (LM 7).  A YCbCr
    context that has the composite records takes them for float frames (LM 5) and, with the half-input table of the preScaling, for
    binary16 frames (LM 6): PQ-10, the configuration tests/test_gpu_half_table.py holds that table to.  Without the composite
    records ("ycbcr_tables" 0) float frames, and without the table ("half_table" 0) binary16 frames, run the search of the mode"""
    pq11, lin12 = fk.config(cs, *fk.MODES[3][:2]), fk.config(cs, *fk.MODES[7][:2])
    if cs != fk.YCC:
        return [(3, pq11, ()), (7, lin12, ())]
    pq10 = fk.config(cs, fk.PQ, 10)
    return [(6, pq10, ()), (3, pq11, NO_HALF_TABLE), (7, lin12, ())] if in16 else [(5, pq10, ()), (3, pq11, NO_COMPOSITE), (7, lin12, ())]


def block_of(family, n):
    """the block of row n of a (family, colour space): sizes go round with n % 3, so the blocks of one size go round too"""
    if family == "distortion":
        return None
    return BLOCKS[(n + n // 3) % 3] if family == "distortion_map" else MOM_BLOCKS[n % 4]


def measuring_matrix():
    """Rows of (id, family, cs, lm, configuration, tunes, in16, profile, w, h, preScaling, block, form): every family by every colour
    space, every front end of it (contexts_of), float and binary16 frames, both 16-bit profiles and the three sizes; YCbCr with
    preScaling 1 and 20; the blocks going round {16, 32, 64} (moments: {8, 16, 32, 64}), the call forms alternating between packed
    and planar.  The 8-bit profiles run on `pq8` rows per colour space, family and frame type: profile 0 and profile 1, one at
    264x70 and one at 258x6 (YCbCr: the search of the mode, LM 3)"""
    out = []
    for family in FAMILIES:
        for cs in (fk.LUV, fk.RGB, fk.YCC, fk.XYZ):
            name, _, _, _, scs = fk.SPACES[cs]
            n = 0
            for in16 in (False, True):
                forms, ft = (HALF_FORMS, "f16") if in16 else (FLOAT_FORMS, "f32")
                for li, (lm, cfg, tunes) in enumerate(contexts_of(cs, in16)):
                    m = li
                    for sc in scs:
                        for profile in PROFILES:
                            for (w, h) in SIZES:
                                ident = "%s-%s-lm%d-%s-sc%g-p%d-%dx%d" % (family, name, lm, ft, sc, profile, w, h)
                                out.append(Row(ident, family, cs, lm, cfg, tunes, in16, profile, w, h, sc, block_of(family, n), forms[m % 2]))
                                n += 1
                                m += 1
                tunes = () if cs != fk.YCC else NO_HALF_TABLE if in16 else NO_COMPOSITE
                for profile, (w, h) in zip((1, 0) if in16 else (0, 1), SIZES[:2]):
                    ident = "%s-%s-pq8-%s-p%d-%dx%d" % (family, name, ft, profile, w, h)
                    out.append(Row(ident, family, cs, 3, fk.pq8(cs), tunes, in16, profile, w, h, scs[-1], block_of(family, n), forms[profile]))
                    n += 1
    return out


def kernel_of(row):
    """(family, CS, SUB, VW, LM, IN16) of the kernel this row's call launches (lumahip_pick.hpp pick_dist), frames 16-byte aligned (8
    for halves) and a frame stride % 4 == 0: distortion_plan takes four pixels per thread at w % 4 == 0, two otherwise"""
    return (row.family, row.cs, row.profile in (0, 2), 4 if row.w % 4 == 0 else 2, row.lm, row.in16)


def half_table_used(row):
    """what half_table_info(sc)["used"] says on this YCbCr row's context: the table exists where the composite records do, unless
    "half_table" is 0"""
    return row.lm in (5, 6) and row.tunes == ()


# ---- the planes of a launch
class HostPlanes:
    """nf frames of code planes in three host byte buffers, laid out as tests/support/device.py Planes lays them out on the device:
    plane p of frame f at base + f * pfs[p], rows st[p] bytes apart, the sentinel in every row padding, gap and in front of the base"""

    def __init__(self, frames, w, h, profile, st=None, gap=GAP, base=0):
        self.w, self.h, self.profile, self.nf, self.gap, self.base = w, h, profile, len(frames), gap, base
        self.st = tuple(st) if st is not None else fk.wide_layout(w, h, profile)
        self.hs, self.size, self.pfs = layout(w, h, profile, self.st, gap)
        self.bufs = planes_from_frames(frames, w, h, profile, self.st, "sentinel", gap, base)

    def frame(self, bufs, f):
        return [bufs[p][self.base + f * self.pfs[p]: self.base + f * self.pfs[p] + self.size[p]].reshape(self.hs[p], self.st[p]) for p in range(3)]


class _Frames:
    """a list of frames, each three (rows, stride) planes, as map_perturbed reads a plane set"""

    def __init__(self, frames):
        self.nf = len(frames)

    def frame(self, bufs, f):
        return bufs[f]


Given = collections.namedtuple("Given", "frames e g words dist dmap")
_given = {}


def given_for(o, family, cfg, profile, w, h, sc, in16, block):
    """The inputs of a launch and numpy's words for them, computed once per key and not written to afterwards:
    frames  fk.frames(w, h), as halves for in16
    e       the ORACLE's planes of them (for halves: of the widened halves), per frame three (rows, stride) arrays
    g       e perturbed: the distortion family on about a tenth of the samples (6x4: half), the map families densely, and with more
            than one block column and row frame 1 keeps its rightmost block column and bottom block row (host.map_perturbed)
    words   the family's expected words of (e, g): (nf, 3, 4), (nf, nby, nbx, 3, 4) or (nf, nby, nbx, 3, 5)
    dist    (nf, 3, 4): expected_distortion of (e, g)
    dmap    map families: expected_distortion_map of (e, g) at `block`"""
    key = (family, cfg, profile, w, h, sc, in16, block)
    if key not in _given:
        frames, e, _ = fk.expected(o, cfg, profile, w, h, sc, in16)
        rng = np.random.default_rng([FAMILIES.index(family), cfg[0], cfg[1], cfg[2], profile, w, h, int(sc), int(in16), block or 0])
        _given[key] = Given(frames, e, *given_from(rng, family, e, w, h, profile, block))
    return _given[key]


def words_of(family, e, g, w, h, profile, block):
    """numpy's words of the family for two lists of frames of three (rows, stride) planes: (nf, 3, 4), (nf, nby, nbx, 3, 4) or
    (nf, nby, nbx, 3, 5)"""
    one = {"distortion": lambda a, b: expected_distortion(a, b, w, h, profile),
           "distortion_map": lambda a, b: expected_distortion_map(a, b, w, h, profile, block),
           "moments_map": lambda a, b: expected_moments_map(a, b, w, h, profile, block)}[family]
    return np.stack([one(e[f], g[f]) for f in range(len(e))])


def given_from(rng, family, e, w, h, profile, block):
    """(g, words, dist, dmap) of given_for for the expected planes e of a launch, whichever front end they are expected of; read-only"""
    nf = len(e)
    if family == "distortion":
        g = [perturb(rng, e[f], w, h, profile, frac=0.5 if w * h < 100 else 0.10) for f in range(nf)]
    elif -(-w // block) > 1 and -(-h // block) > 1:
        g = map_perturbed(rng, _Frames(e), e, w, h, profile, block)
    else:       # (one block column or row: keeping it would leave frame 1 without a difference)
        g = [perturb(rng, e[f], w, h, profile, frac=0.5) for f in range(nf)]
    dist = words_of("distortion", e, g, w, h, profile, None)
    dmap = None if family == "distortion" else words_of("distortion_map", e, g, w, h, profile, block)
    words = dist if family == "distortion" else dmap if family == "distortion_map" else words_of("moments_map", e, g, w, h, profile, block)
    for a in [dist, words] + ([dmap] if dmap is not None else []) + [p for fr in g for p in fr]:
        a.setflags(write=False)
    return g, words, dist, dmap


def given_of(o, row):
    return given_for(o, row.family, row.cfg, row.profile, row.w, row.h, row.sc, row.in16, row.block)


def half_aligned_layout(w, h, profile):
    """(row strides, base): planes half a four-sample unit off its alignment -- 4 bytes off an 8-byte boundary for 16-bit samples, 2 off
    4 for 8-bit -- with row strides and (gap 48) frame strides that are multiples of 8"""
    st = tuple((plane_rows(w, h, profile, p)[1] + 16 + 7) // 8 * 8 for p in range(3))
    return st, (4 if profile > 1 else 2)
