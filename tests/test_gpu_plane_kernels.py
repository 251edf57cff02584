"""The plane-fed kernels, every instantiation the picker can return, at their launch bounds and on the layouts their loads and stores
cannot take as vectors -- needs an MI355X.

Every comparison of planes and words is exact equality.  What the kernels are held to is the ORACLE's decode of the source planes
followed by the oracle's encode under the target configuration (tests/support/plane_kernels.py expected), never what
lumahip_transcode_frames_device wrote; the given planes of the measuring families are a perturbed copy of that expectation and the
words numpy's on the pair (tests/support/host.py expected_distortion / expected_distortion_map, tests/support/moments.py
expected_moments_map).  Every launch has three distinct frames of seeded in-range codes; the 264x70 frames carry 0, 1, the largest
code, the code behind it and all ones in an 8x16 corner -- a chroma code beyond the largest sends its unit to the complete
functions.  Before a call the destination planes hold the sentinel in a layout wider than the rows, the words' buffer the 0xC3
pattern, the maps with 16 guard words behind them: every byte that is no sample, and the guard, must survive.
tests/test_plane_kernels_host.py derives the set of kernels and holds the inputs to the conditions that let a row fail: the expectation
is informative, every given plane of every frame differs from it, no map is all zeros or all differences, the frames' words are pairwise
different, and six wrong kernels modelled with the oracle fail every row they apply to.

k_transcode / k_transcode_distortion / k_transcode_distortion_map / k_transcode_moments_map <CSD, SUBD, CSE, SUBE, VW, LM>
(lumahip_pick.hpp pick_planes; the target's search mode is asserted with quantizer_info and, for a YCbCr target, the composite
records with half_table_info's "used", before anything is compared):
  LM 3 records in LDS          test_plane_matrix[*-luv-lm3-*]     target PQ-11 Lu'v'
  LM 7 value-keyed records     test_plane_matrix[*-luv-lm7-*]     target LINEAR-12 Lu'v'
  LM 5 composite records       test_plane_matrix[*-ycbcr-lm5-*]   target PQ-10 YCbCr 10, preScaling 20
for CSD in Lu'v' (PQ-11) and YCbCr (PQ-10, colour depth 10, maxLum 1000; preScaling 1 -- no division -- and 20 -- the short division
-- on every row, and 3e5 -- the complete functions' IEEE division -- on one 258x6 row per target), SUBD and SUBE by profiles 2 (4:2:0)
and 3 (4:4:4), VW 4 at 264x70 (many tiles, 33 block columns at block 8, ragged both ways), VW 2 at 258x6 (a ragged last tile) and 6x4
(one tile): 48 kernels per family, 192 in all.  The blocks go round {16, 32, 64} (moments: {8, 16, 32, 64}).  The sample width is a
run-time value per side: profiles 0 and 1 run on the [*-pq8-*] rows, the side stored in 8 bits under an 8-bit table.  A k_transcode
row also asserts, on every other row, the statistics: min and max bit for bit those of lumahip_encode_frames_device on the oracle's
decoded frames (tests/test_gpu_frame_kernels.py holds those to the oracle), the sum to the oracle's within 1e-4.  A measuring row also
asserts: the oracle's own planes give all zeros (moments: Se == Sg, See == Sgg == Seg); a map folds to
lumahip_transcode_distortion_frames_device's words; See - 2 Seg + Sgg is lumahip_transcode_distortion_map_frames_device's sse (block
8: after folding 2 x 2).  Every row: source and given planes are byte for byte what they were.
  the launch bounds            test_every_plane_kernel_at_its_launch_bounds   all 192 again at 264x70 and 258x6 under "block" 1024 -- the
                               clamps of transcode_plan to TransFamily::bound, TransDistFamily::bound, transmoments_threads_bound and the
                               maps' 32 x block -- and under "grid_enc" 2, "block" 64 -- the persistent loop and the frame change: the
                               planes and words of the default launch

Layouts (one LM per colour-space pair, profile pairs (2,2) (3,3) (0,1) (1,0), all four families):
  every base, row stride and frame stride of the source planes odd          test_plane_sets_off_their_alignment[*-src-odd]
  ... of the written (k_transcode) or given planes: EncArgs / DecArgs::aligned = 0    [*-tgt-odd]
  ... of both                                                                [*-both-odd]
  one plane set good for units of two samples, not of four: VW 2, aligned 1   [*-src-half] [*-tgt-half]

Left unrun: nothing of the above.  pick_planes knows no other source colour space, target search mode or vector width."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support import plane_kernels as pk  # noqa: E402
from tests.support.device import Frames, L, Planes, ctx, encode, measure, on_device, tmap, transcoded  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import GAP, fold_map  # noqa: E402
from tests.support.moments import fold_2x2, sse_of  # noqa: E402
from tests.support.transcode_moments import tmom  # noqa: E402

NF = pk.NF
ROWS = pk.plane_matrix()
_ctx = {}


def context(L, dcfg, scfg, tunes=()):
    """a context on torch's stream per (target configuration, source configuration, tunes), made once"""
    key = (dcfg, scfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, dcfg, scfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def front_end_asserted(c, row):
    """what transcode_plan picks the kernel by: the target's search mode, and for a YCbCr target that the composite records exist"""
    if row.cse == fk.YCC:
        assert c.quantizer_info()["mode"] == 3 and c.half_table_info(row.dst_sc)["used"], (row.id, "no composite records")
    else:
        assert c.quantizer_info()["mode"] == row.lm, row.id


def laid_out(L, frames, w, h, profile, lay=None):
    """the frames on the device in the wide layout, or in (row strides, gap, base)"""
    st, gap, base = lay if lay is not None else (None, GAP, 0)
    return on_device(L, ms.HostPlanes(frames, w, h, profile, st, gap, base))


def call(family, c, src, src_sc, given, dst_sc, block):
    """the words of one plane-fed measuring call: (nf, 3, 4), (nf, nby, nbx, 3, 4) or (nf, nby, nbx, 3, 5)"""
    if family == "distortion":
        return measure(c, src, src_sc, given, dst_sc)
    return (tmap if family == "distortion_map" else tmom)(c, src, src_sc, given, dst_sc, block)


def transcode(L, c, src, src_sc, dp, dst_sc, stats=False, lay=None):
    """one lumahip_transcode_frames_device launch into sentinel-filled planes, in the wide layout or in (row strides, gap, base): (the
    Planes, their host buffers, the per-frame {sum, min, max} or None)"""
    st, gap, base = lay if lay is not None else (fk.wide_layout(src.w, src.h, dp), GAP, 0)
    out = transcoded(c, L, src, src_sc, dp, dst_sc, strides=st, gap=gap, base=base, stats=stats)
    return out if stats else out + (None,)


def written_planes_asserted(dst, bufs, e, tag):
    """every sample the oracle's, every other byte of the destination the sentinel"""
    problem = fk.planes_problem(bufs, e, dst.w, dst.h, dst.profile, dst.st, dst.gap, dst.base)
    assert problem is None, tag + (problem,)


# ---- 1. the matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_plane_matrix(L, oracle_mod, row):
    c = context(L, row.dcfg, row.scfg)
    front_end_asserted(c, row)
    ex = pk.expected_of(oracle_mod, row)
    w, h, sp, dp, family, block = row.w, row.h, row.sp, row.dp, row.family, row.block
    src = laid_out(L, ex.s, w, h, sp)
    if family == "transcode":
        dst, bufs, got = transcode(L, c, src, row.src_sc, dp, row.dst_sc, row.stats)
        written_planes_asserted(dst, bufs, ex.e, (row.id,))
        if row.stats:
            enc = encode(c, L, Frames(ex.d), row.dst_sc, dp, stats=True)[2]
            for f in range(NF):
                want = (fk.expected_stats(oracle_mod, row.dcfg, ex.d[f], row.dst_sc)[0], enc[f][1], enc[f][2])
                print("%s frame %d: {sum, min, max} %r, the encode call's %r, the oracle's sum %r" % (row.id, f, tuple(got[f]), tuple(enc[f]), want[0]))
                problem = fk.stats_problem(got[f], want)
                assert problem is None, (row.id, f, problem)
    else:
        gv = pk.given_of(oracle_mod, row)
        e, g = laid_out(L, ex.e, w, h, dp), laid_out(L, gv.g, w, h, dp)
        got = call(family, c, src, row.src_sc, g, row.dst_sc, block)
        assert np.array_equal(got, gv.words), (row.id, got, gv.words)
        pk.own_planes_measure_nothing(family, call(family, c, src, row.src_sc, e, row.dst_sc, block), (row.id,))
        if family == "distortion_map":
            folded = np.stack([fold_map(got[f]) for f in range(NF)])
            assert np.array_equal(folded, measure(c, src, row.src_sc, g, row.dst_sc)) and np.array_equal(folded, gv.dist), (row.id, "the map's fold")
        if family == "moments_map":
            m, b = (got, block) if block >= 16 else (fold_2x2(got), 16)
            assert np.array_equal(sse_of(m), tmap(c, src, row.src_sc, g, row.dst_sc, b)[..., 0]), (row.id, "See - 2 Seg + Sgg")
        assert e.unchanged() and g.unchanged(), (row.id, "a given plane changed")
    assert src.unchanged(), (row.id, "a source plane changed")


# ---- 2. the launch bounds and the persistent loop
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_enc", 2), ("block", 64))}
SHAPE_BLOCKS = {"transcode": (None,), "distortion": (None,), "distortion_map": (16, 64), "moments_map": (8, 64)}
KERNEL_GROUPS = [pytest.param(family, csd, cse, sp, dp, w, h,
                              id="%s-%s-%s-p%d-p%d-%dx%d" % (family, fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, w, h))
                 for family in pk.FAMILIES for (csd, cse) in pk.PAIRS for sp in pk.PROFILES for dp in pk.PROFILES for (w, h) in pk.SIZES[:2]]


@pytest.mark.parametrize("family,csd,cse,sp,dp,w,h", KERNEL_GROUPS)
def test_every_plane_kernel_at_its_launch_bounds(L, oracle_mod, family, csd, cse, sp, dp, w, h):
    """k_*<CSD, SUBD, CSE, SUBE, VW, every LM of the target> asked to run with 1024 threads: transcode_plan clamps the launch to
    TransFamily::bound (1024, which the HDR10 -> PQ-11 pair's 59 KiB of tables ask for by themselves), TransDistFamily::bound (512 with
    YCbCr on either side), transmoments_threads_bound and, the maps, to 32 x block threads -- a kernel compiled for fewer threads than
    its plan allows fails to launch.  Then two workgroups of one wave: the persistent loop, the frame change inside it, the most
    sub-tiles per map tile.  The planes and words of the default launch and the oracle's, all three"""
    rows = [r for r in ROWS if (r.family, r.csd, r.cse, r.sp, r.dp, r.w, r.h) == (family, csd, cse, sp, dp, w, h) and
            r.src_sc == pk.scalings(csd, cse, r.lm)[-1][0]]
    assert sorted(pk.kernel_of(r)[6] for r in rows) == [lm for (cs, lm) in pk.TARGETS if cs == cse]
    for row in rows:
        ex = pk.expected_of(oracle_mod, row)
        src = laid_out(L, ex.s, w, h, sp)
        for block in SHAPE_BLOCKS[family]:
            if family == "transcode":
                _, default, _ = transcode(L, context(L, row.dcfg, row.scfg), src, row.src_sc, dp, row.dst_sc)
            else:
                gv = pk.given_for(oracle_mod, family, row.scfg, row.dcfg, sp, dp, w, h, row.src_sc, row.dst_sc, block)
                g = laid_out(L, gv.g, w, h, dp)
                default = call(family, context(L, row.dcfg, row.scfg), src, row.src_sc, g, row.dst_sc, block)
                assert np.array_equal(default, gv.words), (row.id, block, "default", default, gv.words)
            for shape, tunes in SHAPES.items():
                c = context(L, row.dcfg, row.scfg, tunes)
                front_end_asserted(c, row)
                if family == "transcode":
                    dst, bufs, _ = transcode(L, c, src, row.src_sc, dp, row.dst_sc)
                    written_planes_asserted(dst, bufs, ex.e, (row.id, shape))
                    assert all(np.array_equal(a, b) for a, b in zip(bufs, default)), (row.id, shape, "the default launch")
                else:
                    got = call(family, c, src, row.src_sc, g, row.dst_sc, block)
                    assert np.array_equal(got, default), (row.id, block, shape, got, default)
            assert family == "transcode" or g.unchanged(), (row.id, block)
        assert src.unchanged(), row.id


# ---- 3. layouts the vector loads and stores cannot take
LAYOUT_PAIRS = {(fk.LUV, fk.LUV): 3, (fk.LUV, fk.YCC): 5, (fk.YCC, fk.LUV): 7, (fk.YCC, fk.YCC): 5}      # one LM per colour-space pair
LAYOUT_PROFILES = [(2, 2), (3, 3), (0, 1), (1, 0)]
LAYOUT_BLOCK = {"transcode": None, "distortion": None, "distortion_map": 16, "moments_map": 8}
KINDS = ["src-odd", "tgt-odd", "both-odd", "src-half", "tgt-half"]


def layout_of(kind, w, h, profile):
    """(row strides, gaps, base) of a plane set of this kind"""
    if kind == "odd":
        return fk.odd_layout(w, h, profile) + (1,)
    st, base = ms.half_aligned_layout(w, h, profile)
    return st, GAP, base


def parities_asserted(kind, pl, tag):
    if kind == "odd":
        assert all(p % 2 == 1 for p in pl.ptrs) and all(s % 2 == 1 for s in pl.st) and all(s % 2 == 1 for s in pl.pfs), tag
    else:       # four samples: 8 bytes, or 4
        unit = 8 if pl.profile > 1 else 4
        assert all(p % unit == unit // 2 for p in pl.ptrs) and all(s % 8 == 0 for s in tuple(pl.st) + tuple(pl.pfs)), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sp,dp", LAYOUT_PROFILES)
@pytest.mark.parametrize("csd,cse", list(LAYOUT_PAIRS), ids=lambda cs: fk.SPACES[cs][0])
def test_plane_sets_off_their_alignment(L, oracle_mod, csd, cse, sp, dp, kind):
    """odd: every plane of the set one byte into its buffer, odd row strides, odd frame strides -- DecArgs::aligned = 0 for planes read,
    EncArgs::aligned = 0 and the byte-wise stores for planes written, with units of four samples (264x70 luma and 4:4:4 chroma), two
    (its 4:2:0 chroma, 258x6) and one (258x6 4:2:0 chroma), by 8- and 16-bit samples.  half: 264x70, the set half a four-sample unit off,
    strides multiples of 8 -- the plan must take two pixels per thread and keep the vector accesses.  The planes and words of the
    aligned call and the oracle's; on an odd destination every byte around the samples shows whether a store ran past a row's end"""
    lm = LAYOUT_PAIRS[(csd, cse)]
    scfg, dcfg = pk.side_cfg(csd, 3, sp), pk.side_cfg(cse, lm, dp)
    src_sc, dst_sc = pk.scalings(csd, cse, lm)[-1]
    c = context(L, dcfg, scfg)
    which, how = kind.split("-")
    for (w, h) in (pk.SIZES[:2] if how == "odd" else pk.SIZES[:1]):
        ex = pk.expected(oracle_mod, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc)
        slay = layout_of(how, w, h, sp) if which in ("src", "both") else None
        tlay = layout_of(how, w, h, dp) if which in ("tgt", "both") else None
        src, plain = laid_out(L, ex.s, w, h, sp, slay), laid_out(L, ex.s, w, h, sp)
        if slay is not None:
            parities_asserted(how, src, (kind, w, h, "source"))
        for family in pk.FAMILIES:
            tag = (fk.SPACES[csd][0], fk.SPACES[cse][0], sp, dp, kind, w, h, family)
            if family == "transcode":
                if tlay is not None:
                    parities_asserted(how, Planes(L, w, h, dp, NF, strides=tlay[0], gap=tlay[1], base=tlay[2]), tag)
                dst, bufs, _ = transcode(L, c, src, src_sc, dp, dst_sc, lay=tlay)
                written_planes_asserted(dst, bufs, ex.e, tag)
                adst, abufs, _ = transcode(L, c, plain, src_sc, dp, dst_sc)
                written_planes_asserted(adst, abufs, ex.e, tag + ("the aligned call",))
                continue
            block = LAYOUT_BLOCK[family]
            gv = pk.given_for(oracle_mod, family, scfg, dcfg, sp, dp, w, h, src_sc, dst_sc, block)
            e, g = laid_out(L, ex.e, w, h, dp, tlay), laid_out(L, gv.g, w, h, dp, tlay)
            if tlay is not None:
                parities_asserted(how, g, tag)
            got = call(family, c, src, src_sc, g, dst_sc, block)
            assert np.array_equal(got, gv.words), tag + (got, gv.words)
            aligned = call(family, c, plain, src_sc, laid_out(L, gv.g, w, h, dp), dst_sc, block)
            assert np.array_equal(got, aligned), tag + ("the aligned call",)
            pk.own_planes_measure_nothing(family, call(family, c, src, src_sc, e, dst_sc, block), tag)
            assert e.unchanged() and g.unchanged(), tag + ("a given plane changed",)
        assert src.unchanged() and plain.unchanged(), (kind, w, h, "a source plane changed")
