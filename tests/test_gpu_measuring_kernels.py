"""The frame-fed measuring kernels, every instantiation the picker can return, and the layouts their loads cannot take as vectors --
needs an MI355X.

Every comparison is exact equality of integers with numpy's words (tests/support/host.py expected_distortion /
expected_distortion_map, tests/support/moments.py expected_moments_map); there is no tolerance anywhere.  The planes the kernels'
front end is held to are the ORACLE's (tests/support/measuring.py given_for: Oracle.encode of every frame of the launch, for
binary16 frames of the widened halves), never what lumahip_encode_frames_device wrote, and the given planes are a perturbed copy of
them with the sentinel in every row padding and gap.  Every launch has three distinct frames (log-uniform 1e-4 .. 3e4, special_frame
in the corner of 264x70: NaN, infinities, negatives and zeros pass through every front end); before a call the output holds the 0xC3
pattern, the maps with 16 guard words behind them, which must survive.  tests/test_measuring_kernels_host.py derives the set of
kernels and holds the inputs to the conditions that let a row fail: every plane of every frame differs, no map is all zeros or all
differences, the frames' words are pairwise different.

k_distortion / k_distortion_map / k_moments_map <CS, SUB, VW, LM, IN16> (lumahip_pick.hpp pick_dist; the search mode is asserted with
quantizer_info, and for YCbCr half_table_info's "used", before anything is compared):
  LM 3 records in LDS          test_measuring_matrix[*-lm3-*]   PQ-11; YCbCr float frames under "ycbcr_tables" 0, binary16 frames under
                                                                "half_table" 0
  LM 7 value-keyed records     test_measuring_matrix[*-lm7-*]   LINEAR-12
  LM 5 composite records       test_measuring_matrix[*-ycbcr-lm5-f32-*]   PQ-10 YCbCr, float frames on a default context
  LM 6 + the half-input table  test_measuring_matrix[*-ycbcr-lm6-f16-*]   the same context, binary16 frames
for CS in Lu'v', RGB, YCbCr (maxLum 1000, colour depth 10, preScaling 1 and 20) and XYZ, SUB by profiles 2 (4:2:0) and 3 (4:4:4), VW 4 at
264x70 (several block columns and rows, ragged both ways), VW 2 at 258x6 (a ragged last tile) and 6x4 (one tile), IN16 by float frames
(the packed and _planar calls alternating) and binary16 frames (_f16 and _planar_f16): 72 kernels per family, 216 in all.  RGB and XYZ
chroma thereby go through quantize_lut<3, N> and <7, N>.  The blocks go round {16, 32, 64} (moments: {8, 16, 32, 64}).  The sample size
is a kernel argument: profiles 0 and 1 run on the [*-pq8-*] rows.  Every row also asserts: the oracle's own planes give all zeros
(moments: Se == Sg, See == Sgg == Seg); frames and planes are byte for byte what they were; a map folds to
lumahip_distortion_frames_device's words; See - 2 Seg + Sgg is lumahip_distortion_map_frames_device's sse (block 8: after folding
2 x 2); a binary16 call equals the float call on the widened frames.
  the launch bounds            test_every_kernel_at_the_largest_workgroup   all 216 again at 264x70 and 258x6 under "block" 1024 -- the
                               clamp of distortion_plan to 32 x block threads and to lh::moments_threads_bound -- and under
                               "grid_enc" 2, "block" 64 -- the persistent loop and the frame change: the words of the default launch

Layouts (one records-in-LDS configuration per colour space, profiles 0-3, all three families, float and binary16 frames):
  every base, row stride and frame stride of the given planes odd    test_given_planes_and_frames_off_their_alignment[*-odd-*]
  given planes good for units of two samples, not of four            [*-half-aligned]   DecArgs::aligned = 0 under VW 4
  float frames 8 bytes off a 16-byte boundary / 3 w h + 2 apart      [*-frames-*]       VW 2 at w % 4 == 0
  halves 4 bytes off an 8-byte boundary / 3 w h + 2 apart / both     [*-frames-*]
  refused before any launch                                          test_refused_layouts_launch_nothing

Left unrun: nothing of the above.  Search modes other than 3 and 7 are refused (tests/test_gpu_distortion.py and its siblings hold the
refusals), so k_distortion<., ., ., 4 | 0 | 2, .> and their map siblings do not exist."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support.device import Frames, L, ctx, dist, dist_map, map_buf, on_device, out_buf  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import ERR_ARG, GAP, OUT_FILL, fold_map, nwords, widen_halves  # noqa: E402
from tests.support.moments import fold_2x2, mom_map, mom_nwords, sse_of  # noqa: E402

NF = fk.NF
ROWS = ms.measuring_matrix()
_ctx = {}


def context(L, cfg, tunes=()):
    """a context on torch's stream per (configuration, tunes), made once; the tunes are set before the first encode-side call"""
    key = (cfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, cfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def call(family, c, fr, sc, given, block, form):
    """the words of one frame-fed measuring call: (nf, 3, 4), (nf, nby, nbx, 3, 4) or (nf, nby, nbx, 3, 5)"""
    if family == "distortion":
        return dist(c, fr, sc, given, form)
    return (dist_map if family == "distortion_map" else mom_map)(c, fr, sc, given, block, form)


def device_frames(frames, in16, pad=4, base=0):
    return Frames(frames, dtype=np.float16 if in16 else np.float32, pad=pad, base=base)


def own_planes_measure_nothing(family, own, tag):
    """the call on the planes the front end is held to: no difference (moments: both signals have the same sums)"""
    if family == "moments_map":
        assert own.any() and np.array_equal(own[..., 0], own[..., 1]) and np.array_equal(own[..., 2], own[..., 3]) and \
            np.array_equal(own[..., 2], own[..., 4]), tag + ("the oracle's own planes", own)
    else:
        assert not own.any(), tag + ("the oracle's own planes", own)


def front_end_asserted(c, row):
    """the search mode and, for YCbCr, whether the half-input table exists: what distortion_plan picks the kernel by"""
    assert c.quantizer_info()["mode"] == (7 if row.lm == 7 else 3), row.id
    if row.cs == fk.YCC:
        assert c.half_table_info(row.sc)["used"] == ms.half_table_used(row), row.id


# ---- 1. the matrix
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_measuring_matrix(L, oracle_mod, row):
    c = context(L, row.cfg, row.tunes)
    front_end_asserted(c, row)
    gv = ms.given_of(oracle_mod, row)
    w, h, profile, sc, block, family = row.w, row.h, row.profile, row.sc, row.block, row.family
    fr = device_frames(gv.frames, row.in16)
    e, g = on_device(L, ms.HostPlanes(gv.e, w, h, profile)), on_device(L, ms.HostPlanes(gv.g, w, h, profile))
    got = call(family, c, fr, sc, g, block, row.form)
    assert np.array_equal(got, gv.words), (row.id, got, gv.words)
    own_planes_measure_nothing(family, call(family, c, fr, sc, e, block, row.form), (row.id,))
    if family == "distortion_map":
        folded = np.stack([fold_map(got[f]) for f in range(NF)])
        assert np.array_equal(folded, dist(c, fr, sc, g, row.form)) and np.array_equal(folded, gv.dist), (row.id, "the map's fold")
    if family == "moments_map":
        m, b = (got, block) if block >= 16 else (fold_2x2(got), 16)
        assert np.array_equal(sse_of(m), dist_map(c, fr, sc, g, b, row.form)[..., 0]), (row.id, "See - 2 Seg + Sgg")
    if row.in16:
        wide = Frames(widen_halves(gv.frames))
        assert np.array_equal(call(family, c, wide, sc, g, block, ms.FLOAT_FORMS[ms.HALF_FORMS.index(row.form)]), got), (row.id, "the float call")
        assert wide.unchanged(), row.id
    assert fr.unchanged() and e.unchanged() and g.unchanged(), (row.id, "an input changed")


# ---- 2. the launch bounds and the persistent loop
SHAPES = {"1024_threads": (("block", 1024),), "two_workgroups_of_64": (("grid_enc", 2), ("block", 64))}
SHAPE_BLOCKS = {"distortion": (None,), "distortion_map": (16, 64), "moments_map": (8, 64)}
KERNEL_GROUPS = [pytest.param(family, cs, profile, w, h, id="%s-%s-p%d-%dx%d" % (family, fk.SPACES[cs][0], profile, w, h))
                 for family in ms.FAMILIES for cs in fk.SPACES for profile in ms.PROFILES for (w, h) in ms.SIZES[:2]]


@pytest.mark.parametrize("family,cs,profile,w,h", KERNEL_GROUPS)
def test_every_kernel_at_the_largest_workgroup(L, oracle_mod, family, cs, profile, w, h):
    """k_*<CS, SUB, VW, every LM, both IN16> asked to run with 1024 threads: distortion_plan clamps a map launch to 32 x block threads (block
    8: 256, block 16: 512) and a moments launch to lh::moments_threads_bound, which block 64 leaves as the only clamp -- a kernel
    compiled for fewer threads than the plan allows fails to launch.  Then two workgroups of one wave: the persistent loop, the frame
    change inside it, the most sub-tiles per map tile.  The words of the default launch and numpy's, all three"""
    rows = [r for r in ROWS if (r.family, r.cs, r.profile, r.w, r.h) == (family, cs, profile, w, h) and r.sc == fk.SPACES[cs][4][-1]]
    assert {ms.kernel_of(r)[4:] for r in rows} == {(lm, in16) for in16 in (False, True) for (lm, _, _) in ms.contexts_of(cs, in16)}
    for row in rows:
        fr = None
        for block in SHAPE_BLOCKS[family]:
            gv = ms.given_for(oracle_mod, family, row.cfg, profile, w, h, row.sc, row.in16, block)
            fr = device_frames(gv.frames, row.in16) if fr is None else fr
            g = on_device(L, ms.HostPlanes(gv.g, w, h, profile))
            default = call(family, context(L, row.cfg, row.tunes), fr, row.sc, g, block, row.form)
            assert np.array_equal(default, gv.words), (row.id, block, "default", default, gv.words)
            for shape, tunes in SHAPES.items():
                c = context(L, row.cfg, row.tunes + tunes)
                front_end_asserted(c, row)
                got = call(family, c, fr, row.sc, g, block, row.form)
                assert np.array_equal(got, default), (row.id, block, shape, got, default)
            assert g.unchanged(), (row.id, block)
        assert fr.unchanged(), row.id


# ---- 3. layouts the vector loads cannot take
def layout_cfg(cs, profile):
    return (fk.config(cs, fk.PQ, 11) if profile > 1 else fk.pq8(cs)), fk.SPACES[cs][4][-1]


LAYOUT_BLOCK = {"distortion": None, "distortion_map": 16, "moments_map": 8}
FRAME_LAYOUTS = [(False, 2, 4), (False, 0, 2), (True, 2, 4), (True, 0, 2), (True, 2, 2)]      # (halves, base, pad) in elements
LAYOUTS = ["odd-264x70", "odd-258x6", "half-aligned"] + ["frames-%s-base%d-pad%d" % ("f16" if i else "f32", b, p) for (i, b, p) in FRAME_LAYOUTS]


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("profile", [0, 1, 2, 3])
@pytest.mark.parametrize("cs", [fk.LUV, fk.RGB, fk.YCC, fk.XYZ], ids=lambda cs: fk.SPACES[cs][0])
def test_given_planes_and_frames_off_their_alignment(L, oracle_mod, cs, profile, kind):
    """odd: every given plane one byte into its buffer, odd row strides, odd frame strides -- DecArgs::aligned = 0, units of four samples
    (264x70 luma and 4:4:4 chroma), two (its 4:2:0 chroma, 258x6) and one (258x6 4:2:0 chroma), by 8- and 16-bit samples.  half-aligned:
    264x70, the planes half a four-sample unit off, strides multiples of 8.  frames-*: 264x70 with the frames 8 bytes off a 16-byte
    boundary (halves: 4 off 8) or 3 w h + 2 elements apart: check_frame_alignment sends the launch to the two-pixel kernels.
    The words of the aligned call and numpy's"""
    cfg, sc = layout_cfg(cs, profile)
    c = context(L, cfg)
    w, h = (258, 6) if kind == "odd-258x6" else (264, 70)
    in16, fbase, fpad = FRAME_LAYOUTS[LAYOUTS.index(kind) - 3] if kind.startswith("frames") else (False, 0, 4)
    for family in ms.FAMILIES:
        block = LAYOUT_BLOCK[family]
        tag = (fk.SPACES[cs][0], profile, kind, family)
        gv = ms.given_for(oracle_mod, family, cfg, profile, w, h, sc, in16, block)
        if kind.startswith("odd"):
            st, gap = fk.odd_layout(w, h, profile)
            hp = [ms.HostPlanes(x, w, h, profile, st, gap, base=1) for x in (gv.e, gv.g)]
        elif kind == "half-aligned":
            st, base = ms.half_aligned_layout(w, h, profile)
            hp = [ms.HostPlanes(x, w, h, profile, st, GAP, base=base) for x in (gv.e, gv.g)]
        else:
            hp = [ms.HostPlanes(x, w, h, profile) for x in (gv.e, gv.g)]
        e, g = on_device(L, hp[0]), on_device(L, hp[1])
        fr = device_frames(gv.frames, in16, fpad, fbase)
        esz = 2 if in16 else 4
        if kind.startswith("odd"):
            assert all(p % 2 == 1 for p in g.ptrs) and all(s % 2 == 1 for s in g.st) and all(s % 2 == 1 for s in g.pfs), tag
        elif kind == "half-aligned":
            unit = 8 if profile > 1 else 4
            assert all(p % unit == unit // 2 for p in g.ptrs) and all(s % 8 == 0 for s in g.st + tuple(g.pfs)), tag
        else:
            assert (fr.ptr % (4 * esz), fr.fs % 4) == (fbase * esz, fpad % 4) and (fbase, fpad) != (0, 4), tag
        form = "f16" if in16 else "packed"
        got = call(family, c, fr, sc, g, block, form)
        assert np.array_equal(got, gv.words), tag + (got, gv.words)
        aligned = call(family, c, device_frames(gv.frames, in16), sc, on_device(L, ms.HostPlanes(gv.g, w, h, profile)), block, form)
        assert np.array_equal(got, aligned), tag + ("the aligned call",)
        own_planes_measure_nothing(family, call(family, c, fr, sc, e, block, form), tag)
        assert fr.unchanged() and e.unchanged() and g.unchanged(), tag + ("an input changed",)


@pytest.mark.parametrize("family", ms.FAMILIES)
def test_refused_layouts_launch_nothing(L, oracle_mod, family):
    """frames 4 bytes off an 8-byte boundary (halves: 2 off 4) and an odd frame stride: LUMAHIP_ERR_ARG from check_frame_alignment, in front
    of the launch; the output keeps its fill, and the same arguments on accepted frames measure what numpy does"""
    import torch
    cfg, sc, profile, w, h, block = fk.config(fk.LUV, fk.PQ, 11), 1.0, 2, 264, 70, LAYOUT_BLOCK[family]
    c = context(L, cfg)
    name = {"distortion": "distortion_frames_device", "distortion_map": "distortion_map_frames_device", "moments_map": "moments_map_frames_device"}[family]
    words = NF * 12 if family == "distortion" else (nwords if family == "distortion_map" else mom_nwords)(NF, w, h, block)
    for in16 in (False, True):
        gv = ms.given_for(oracle_mod, family, cfg, profile, w, h, sc, in16, block)
        g = on_device(L, ms.HostPlanes(gv.g, w, h, profile))
        for what, fbase, fpad in (("one element off", 1, 4), ("an odd frame stride", 0, 3), ("both", 1, 3)):
            fr = device_frames(gv.frames, in16, fpad, fbase)
            assert fr.ptr % (2 * (2 if in16 else 4)) != 0 or fr.fs % 2 == 1
            out = out_buf(NF) if family == "distortion" else map_buf(words)
            tail = (out.data_ptr(),) if family == "distortion" else (block, out.data_ptr())
            with pytest.raises(L.LumaHipError) as ei:
                getattr(c, name + ("_f16" if in16 else ""))(fr.ptr, fr.fs, NF, w, h, sc, profile, g.ptrs, g.st, g.pfs, *tail)
            assert ei.value.code == ERR_ARG, (family, in16, what)
            torch.cuda.synchronize()
            assert np.all(out.cpu().numpy() == OUT_FILL), (family, in16, what, "the output changed")
            assert fr.unchanged() and g.unchanged(), (family, in16, what)
        got = call(family, c, device_frames(gv.frames, in16), sc, g, block, "f16" if in16 else "packed")
        assert np.array_equal(got, gv.words), (family, in16, "after the refused calls")
