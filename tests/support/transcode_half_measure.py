"""What tests/test_gpu_transcode_half_distortion.py and tests/test_transcode_half_distortion_host.py share, numpy and the oracle alone:
the two matrices of the half-resolution transcode distortion calls (include/lumahip_ladder.h), the k_transcode_half_distortion /
k_transcode_half_distortion_map instantiations their rows launch, and the inputs and expected words of a row -- e from the model of
tests/support/transcode_half.py (`expected`), the given planes and numpy's words from tests/support/measuring.py (`given_from`).

Nothing the library wrote enters an expectation.  Helpers here assert with an explicit message: pytest rewrites `assert` in test
modules only."""
import collections

import numpy as np

from tests.support import frame_kernels as fk
from tests.support import measuring as ms
from tests.support import transcode_half as th
from tests.support.host import BLOCKS

NF = th.NF
FAMILIES = ("distortion", "distortion_map")
# the map's source sizes, position by position in the place of th.SIZES: 264x140 gives a 132x70 target -- VW 4, 9 x 5 blocks of 16, 3 x 2
# of 64, a last block row 6 rows high (the "no tile" sub-tiles) --, the others are th.SIZES'
MAP_SIZES = [(264, 140), (520, 12), (268, 76), (8, 4)]
ORDER_SIZES = {"distortion": th.ORDER_SIZES, "distortion_map": (MAP_SIZES[0], MAP_SIZES[2])}

Row = collections.namedtuple("Row", "id family block " + " ".join(f for f in th.Row._fields if f != "id"))


def _ident(family, r, w, h, block):
    tail = th._ident(r.csd, r.cse, r.lm, r.sp, r.dp, w, h, r.src_sc, r.eight)[len("half-"):]
    return "%s-%s%s" % (family, tail, "" if block is None else "-b%d" % block)


def measure_matrix(family):
    """th.half_matrix() as it stands for the per-frame words; for the map the same rows with the sizes replaced position by position by
    MAP_SIZES and the blocks cycling 16 / 32 / 64 over the rows"""
    out = []
    for n, r in enumerate(th.half_matrix()):
        w, h = (r.w, r.h) if family == "distortion" else MAP_SIZES[th.SIZES.index((r.w, r.h))]
        block = None if family == "distortion" else BLOCKS[n % 3]
        f = r._asdict()
        f.update(id=_ident(family, r, w, h, block), w=w, h=h)
        out.append(Row(family=family, block=block, **f))
    return out


def vw4_exists(csd, subd, cse):
    """lh::transhalfdist_vw4 (luma_kernels.hpp): which kernels of these two families exist at VW 4.  From the compiler's report
    (profiles/transcode_half_distortion_codegen.txt): under the 512-thread bound a 4:4:4 source cannot be had at VW 4 without scratch,
    except Lu'v' -> YCbCr"""
    return subd or (csd == fk.LUV and cse == fk.YCC)


def kernel_of(row, family=None):
    """(family, CSD, SUBD, CSE, SUBE, VW, LM) of the kernel this row's call launches, both plane sets aligned for units of four samples:
    transcode_plan takes four pixels per thread where the TARGET's width is a multiple of 4 and the family exists at VW 4, else two"""
    subd = row.sp in (0, 2)
    vw = 4 if (row.w // 2) % 4 == 0 and vw4_exists(row.csd, subd, row.cse) else 2
    return (family or row.family, row.csd, subd, row.cse, row.dp in (0, 2), vw, row.lm)


def instantiated(family):
    """every kernel lumahip_transcode_half_distortion.hip / lumahip_transcode_half_distortion_map.hip instantiates"""
    return {(family, csd, subd, cse, sube, vw, lm) for csd in (fk.LUV, fk.YCC) for subd in (True, False)
            for (cse, lm) in ((fk.LUV, 3), (fk.LUV, 7), (fk.YCC, 5)) for sube in (True, False) for vw in (4, 2)
            if vw == 2 or vw4_exists(csd, subd, cse)}


Inputs = collections.namedtuple("Inputs", "ex g words dist dmap")
_inputs = {}


def inputs_of(o, row):
    """The inputs of a row's launch and numpy's words for them, computed once and not written to afterwards:
    ex     th.expected of the row: source planes s, decoded floats d, box m, expected planes e of (w/2) x (h/2)
    g      e perturbed (ms.given_from)
    words  the family's expected words: (NF, 3, 4) or (NF, nby, nbx, 3, 4)
    dist   (NF, 3, 4), the per-frame words of (e, g);  dmap: the map's words, or None"""
    if row.id not in _inputs:
        ex = th.expected(o, row.scfg, row.dcfg, row.sp, row.dp, row.w, row.h, row.src_sc, row.dst_sc)
        rng = np.random.default_rng([FAMILIES.index(row.family), row.csd, row.cse, row.lm, row.sp, row.dp, row.w, row.h,
                                     int(row.src_sc), row.block or 0, int(row.eight)])
        _inputs[row.id] = Inputs(ex, *ms.given_from(rng, row.family, ex.e, row.w // 2, row.h // 2, row.dp, row.block))
    return _inputs[row.id]


def wrong_words(o, row, name):
    """the family's words of the planes a wrong kernel or wrong order `name` (th.wrong_frame) would make, against the row's own g"""
    inp = inputs_of(o, row)
    wrong = [fk.oracle(o, row.dcfg).encode(th.wrong_frame(inp.ex.d[f], name).copy(), row.dst_sc, row.dp)[0] for f in range(NF)]
    return ms.words_of(row.family, wrong, inp.g, row.w // 2, row.h // 2, row.dp, row.block)


def own_region(src_frames, w, h, profile):
    """a plane set of (w/2) x (h/2) that is the top-left region of a source set of w x h of the same profile, read with the source's
    own strides: per frame three views"""
    from tests.support.host import plane_rows
    return [[np.asarray(fr[p])[:plane_rows(w // 2, h // 2, profile, p)[0]] for p in range(3)] for fr in src_frames]


__all__ = ["FAMILIES", "MAP_SIZES", "NF", "ORDER_SIZES", "Inputs", "Row", "inputs_of", "instantiated", "kernel_of", "measure_matrix", "own_region",
           "vw4_exists", "wrong_words"]
