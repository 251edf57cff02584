"""Half-resolution transcode distortion and its map (include/lumahip_ladder.h): given code planes of (w/2) x (h/2) against what
lumahip_transcode_half_frames_device would write for source planes of w x h, per frame and per block of the half-size target, one launch
each -- needs an MI355X.

Every comparison of words is exact equality with numpy's integers of (e, g): e the model of tests/support/transcode_half.py (the
ORACLE's decode, numpy's fp32 ((a + b) + (c + d)) * 0.25, the ORACLE's encode), g a perturbed copy of e (tests/support/measuring.py
given_from).  Nothing the library wrote enters an expectation; what the library wrote by the replaced method -- the half-resolution
transcode into scratch planes, then the plane-to-plane call -- is compared on top.  tests/test_transcode_half_distortion_host.py derives
the kernels from the matrices and holds every row's inputs to the conditions that let it fail.

  test_matrix                    every row of both matrices (326): all 38 + 38 kernels, a YCbCr source at preScaling 1, 20 and 3e5, the
                                 8-bit rows; sentinels around the words; both plane sets unchanged; the map folds to the per-frame words;
                                 both agree with the replaced method run on the device
  test_other_launch_shapes       lumahip_tune "block" 256 / 512 / 1024, "grid_enc" 1 and 7, "blocks_per_cu"
  test_layouts_gaps_and_overlap  odd strides and half-aligned sets on either side, frame gaps, a given set inside the source's own buffers
  test_sections_and_host_forms   unordered sections on both lanes; the host forms
  test_far_plane_sets            both sets beyond 2^32 bytes of their pointers
  test_refusals_launch_nothing   every refusal, its code and message, before any launch"""
import collections
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.support import far_layouts as fl  # noqa: E402
from tests.support import frame_kernels as fk  # noqa: E402
from tests.support import measuring as ms  # noqa: E402
from tests.support import plane_kernels as pk  # noqa: E402
from tests.support import transcode_half as th  # noqa: E402
from tests.support import transcode_half_measure as hm  # noqa: E402
from tests.support.device import L, Planes, ctx, dev, on_device  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import GAP, GUARD, OUT_FILL, fold_map, plane_rows  # noqa: E402

NF = hm.NF
ROWS = {family: hm.measure_matrix(family) for family in hm.FAMILIES}
_ctx = {}


def context(L, dcfg, scfg, tunes=()):
    key = (dcfg, scfg, tuple(tunes))
    if key not in _ctx:
        c = ctx(L, dcfg, scfg)
        for name, v in tunes:
            c.tune(name, v)
        _ctx[key] = c
    return _ctx[key]


def laid_out(L, frames, w, h, profile, lay=None):
    """the frames on the device in the wide layout, or in (row strides, gap, base)"""
    st, gap, base = lay if lay is not None else (None, GAP, 0)
    return on_device(L, ms.HostPlanes(frames, w, h, profile, st, gap, base))


def shape_of(nf, tw, t_h, block):
    return (nf, 3, 4) if block is None else (nf, -(-t_h // block), -(-tw // block), 3, 4)


class Words:
    """the output of a call with GUARD sentinel words in front of it and behind it"""

    def __init__(self, shape):
        import torch
        self.shape, self.n = shape, int(np.prod(shape))
        self.t = torch.full((self.n + 2 * GUARD,), OUT_FILL, dtype=torch.int64, device=dev())

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * GUARD

    def untouched(self):
        return bool((self.t == OUT_FILL).all())

    def words(self, tag):
        a = self.t.cpu().numpy()
        assert np.all(a[:GUARD] == OUT_FILL) and np.all(a[-GUARD:] == OUT_FILL), tag + ("sentinel words around the output",)
        return a[GUARD:-GUARD].view(np.uint64).reshape(self.shape)


def measured(c, src, src_sc, given, dst_sc, block, tag, w=None, h=None, sync=True):
    """one launch of the per-frame call (block None) or of the map"""
    import torch
    w, h = w or src.w, h or src.h
    out = Words(shape_of(src.nf, w // 2, h // 2, block))
    args = (src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, w, h, given.ptrs, given.st, given.pfs, given.profile, dst_sc)
    if block is None:
        c.transcode_half_distortion_frames_device(*args, out.ptr)
    else:
        c.transcode_half_distortion_map_frames_device(*args, block, out.ptr)
    if not sync:
        return out
    torch.cuda.synchronize()
    return out.words(tag)


def replaced(L, c, src, src_sc, given, dst_sc, block, tag):
    """the method the calls replace, on the device: the half-resolution transcode into scratch planes, then the plane-to-plane call"""
    import torch
    tw, t_h = src.w // 2, src.h // 2
    scratch = Planes(L, tw, t_h, given.profile, src.nf)
    c.transcode_half_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h, scratch.ptrs, scratch.st, scratch.pfs,
                                   scratch.profile, dst_sc)
    out = Words(shape_of(src.nf, tw, t_h, block))
    args = (scratch.ptrs, scratch.st, scratch.pfs, src.nf, tw, t_h, given.ptrs, given.st, given.pfs, given.profile)
    if block is None:
        c.planes_distortion_frames_device(*args, out.ptr)
    else:
        c.planes_distortion_map_frames_device(*args, block, out.ptr)
    torch.cuda.synchronize()
    return out.words(tag + ("the replaced method",))


def same(got, want, tag):
    assert got.shape == want.shape and np.array_equal(got, want), tag + (int(np.count_nonzero(got != want)), "words differ")


def folded(m):
    return np.stack([fold_map(m[f]) for f in range(m.shape[0])])


# ---- 1. the matrices
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for family in hm.FAMILIES for r in ROWS[family]])
def test_matrix(L, oracle_mod, row):
    c = context(L, row.dcfg, row.scfg)
    inp = hm.inputs_of(oracle_mod, row)
    tw, t_h = row.w // 2, row.h // 2
    src, given = laid_out(L, inp.ex.s, row.w, row.h, row.sp), laid_out(L, inp.g, tw, t_h, row.dp)
    tag = (row.id,)
    got = measured(c, src, row.src_sc, given, row.dst_sc, row.block, tag)
    same(got, inp.words, tag)
    per_frame = got if row.block is None else measured(c, src, row.src_sc, given, row.dst_sc, None, tag + ("per frame",))
    same(per_frame, inp.dist, tag + ("per frame",))
    if row.block is not None:
        same(folded(got), per_frame, tag + ("the map folded",))
    same(replaced(L, c, src, row.src_sc, given, row.dst_sc, row.block, tag), got, tag + ("the replaced method",))
    assert src.unchanged() and given.unchanged(), tag + ("an input plane changed",)


# ---- 2. on one Lu'v' -> Lu'v' row and one -> YCbCr row per family
def picked(family):
    """a 16-bit Lu'v' 4:2:0 -> Lu'v' 4:4:4 row at VW 4 and a YCbCr 4:4:4 -> YCbCr 4:2:0 row (VW 2 by the register decision), both at the
    family's first size, the map at block 16"""
    rows = [r for r in ROWS[family] if (r.w, r.h) == (264, 72 if family == "distortion" else 140) and not r.eight]
    if family == "distortion_map":      # (blocks cycle over the rows: rebuild the picked rows at block 16)
        rows = [r._replace(block=16, id=r.id.rsplit("-b", 1)[0] + "-b16") for r in rows]
    a = next(r for r in rows if (r.csd, r.cse, r.lm, r.sp, r.dp) == (fk.LUV, fk.LUV, 3, 2, 3))
    b = next(r for r in rows if (r.csd, r.cse, r.sp, r.dp, r.src_sc) == (fk.YCC, fk.YCC, 3, 2, 20.0))
    assert hm.kernel_of(a)[5] == 4 and hm.kernel_of(b)[5] == 2, "the picked rows' vector widths"
    return [a, b]


PICKED = [pytest.param(r, id=r.id) for family in hm.FAMILIES for r in picked(family)]
SHAPES = {"block_256": (("block", 256),), "block_512": (("block", 512),), "block_1024": (("block", 1024),), "grid_1": (("grid_enc", 1),),
          "grid_7": (("grid_enc", 7),), "two_per_cu": (("blocks_per_cu", 2),), "grid_7_of_64": (("grid_enc", 7), ("block", 64))}


@pytest.mark.parametrize("row", PICKED)
def test_other_launch_shapes(L, oracle_mod, row):
    """integers throughout: the words of every launch shape are the model's -- 1024 threads asked for (the plan clamps the launch to the
    kernels' bound, and to 32 * block for the map), one workgroup and seven (the persistent loop, the frame change inside it, the
    prefetch running off the end, map tiles handed round)"""
    inp = hm.inputs_of(oracle_mod, row)
    src, given = laid_out(L, inp.ex.s, row.w, row.h, row.sp), laid_out(L, inp.g, row.w // 2, row.h // 2, row.dp)
    for shape, tunes in SHAPES.items():
        c = context(L, row.dcfg, row.scfg, tunes)
        same(measured(c, src, row.src_sc, given, row.dst_sc, row.block, (row.id, shape)), inp.words, (row.id, shape))
    assert src.unchanged() and given.unchanged(), row.id


View = collections.namedtuple("View", "ptrs st pfs profile")


def layout_of(kind, w, h, profile):
    if kind == "odd":
        return fk.odd_layout(w, h, profile) + (1,)
    st, base = ms.half_aligned_layout(w, h, profile)
    return st, GAP, base


@pytest.mark.parametrize("kind", ["src-odd", "given-odd", "both-odd", "src-half", "given-half", "gaps", "own-region"])
@pytest.mark.parametrize("row", PICKED)
def test_layouts_gaps_and_overlap(L, oracle_mod, row, kind):
    """odd: every base, row stride and frame stride of the set odd (DecArgs::aligned = 0: the given rows go byte by byte where they are
    compared); half: the set half a four-sample unit off, strides multiples of 8 (VW 2 with vector loads); gaps: unequal gaps between
    frames on both sides; own-region: the given set is the top-left (w/2) x (h/2) of the source's own buffers, read with the source's
    strides -- two read-only sets that overlap"""
    inp = hm.inputs_of(oracle_mod, row)
    w, h, tw, t_h = row.w, row.h, row.w // 2, row.h // 2
    tag = (row.id, kind)
    if kind == "own-region":
        # (the region is read under the target's profile: the row with the target's profile the source's)
        row = row._replace(dp=row.sp, dcfg=pk.side_cfg(row.cse, row.lm, row.sp), id=row.id + "-own")
        inp = hm.inputs_of(oracle_mod, row)
        src = laid_out(L, inp.ex.s, w, h, row.sp)
        given = View(src.ptrs, src.st, src.pfs, row.sp)      # the source's buffers, strides and frame strides
        own = hm.own_region(inp.ex.s, w, h, row.sp)
        want = ms.words_of(row.family, inp.ex.e, own, tw, t_h, row.dp, row.block)
        assert all(want[f, ..., p, 3].sum() > 0 for f in range(NF) for p in range(3)), tag + ("the region equals e",)
        same(measured(context(L, row.dcfg, row.scfg), src, row.src_sc, given, row.dst_sc, row.block, tag), want, tag)
        assert src.unchanged(), tag
        return
    if kind == "gaps":
        slay, glay = (fk.wide_layout(w, h, row.sp), (208, 16, 80), 0), (fk.wide_layout(tw, t_h, row.dp), (32, 400, 96), 0)
    else:
        which, how = kind.split("-")
        slay = layout_of(how, w, h, row.sp) if which in ("src", "both") else None
        glay = layout_of(how, tw, t_h, row.dp) if which in ("given", "both") else None
    src, given = laid_out(L, inp.ex.s, w, h, row.sp, slay), laid_out(L, inp.g, tw, t_h, row.dp, glay)
    if kind.endswith("odd"):
        for pl in ([src] if slay else []) + ([given] if glay else []):
            assert all(p % 2 == 1 for p in pl.ptrs) and all(s % 2 == 1 for s in tuple(pl.st) + tuple(pl.pfs)), tag
    same(measured(context(L, row.dcfg, row.scfg), src, row.src_sc, given, row.dst_sc, row.block, tag), inp.words, tag)
    assert src.unchanged() and given.unchanged(), tag


@pytest.mark.parametrize("row", PICKED)
def test_sections_and_host_forms(L, oracle_mod, row):
    import torch
    c = context(L, row.dcfg, row.scfg)
    inp = hm.inputs_of(oracle_mod, row)
    w, h, tw, t_h = row.w, row.h, row.w // 2, row.h // 2
    src, given = laid_out(L, inp.ex.s, w, h, row.sp), laid_out(L, inp.g, tw, t_h, row.dp)
    c.begin_unordered(2)
    outs = [measured(c, src, row.src_sc, given, row.dst_sc, row.block, (row.id,), sync=False) for _ in range(2)]
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for lane, o in enumerate(outs):
        same(o.words((row.id, "lane", lane)), inp.words, (row.id, "lane", lane))
    # the host forms: frame by frame, tight strides
    sst, gst = ([plane_rows(*a, p)[1] for p in range(3)] for a in ((w, h, row.sp), (tw, t_h, row.dp)))
    for f in range(NF):
        s = [np.ascontiguousarray(np.asarray(inp.ex.s[f][p])[:, :sst[p]]) for p in range(3)]
        g = [np.ascontiguousarray(np.asarray(inp.g[f][p])[:, :gst[p]]) for p in range(3)]
        if row.block is None:
            got = c.transcode_half_distortion_frame(s, sst, w, h, g, gst, row.src_sc, row.sp, row.dst_sc, row.dp)
        else:
            got = c.transcode_half_distortion_map_frame(s, sst, w, h, g, gst, row.src_sc, row.sp, row.dst_sc, row.dp, row.block)
            assert got.shape[:2] == tuple(reversed(L.distortion_map_dims(tw, t_h, row.block))), row.id
        same(got, inp.words[f], (row.id, "host form", f))
    assert src.unchanged() and given.unchanged(), row.id


# ---- 3. far plane sets
@pytest.mark.parametrize("family", hm.FAMILIES)
def test_far_plane_sets(L, oracle_mod, family):
    """source size 264x72, three frames, kind far16: plane frame strides of 2^31 + 16 (p + 1) bytes behind a lead of 2^31, so frame 2 of
    both sets lies beyond 2^32 bytes of its pointer; two sparse allocations of 6 GiB live.  The words equal the near layout's"""
    row = next(r for r in ROWS["distortion"] if (r.csd, r.cse, r.lm, r.sp, r.dp, r.w, r.h) == (fk.LUV, fk.LUV, 3, 2, 2, 264, 72))
    block = None if family == "distortion" else 32
    row = row._replace(family=family, block=block, id="far-%s-%s" % (family, row.id))
    inp = hm.inputs_of(oracle_mod, row)
    c = context(L, row.dcfg, row.scfg)
    w, h, tw, t_h = row.w, row.h, row.w // 2, row.h // 2
    tag = (row.id,)
    near = measured(c, laid_out(L, inp.ex.s, w, h, row.sp), row.src_sc, laid_out(L, inp.g, tw, t_h, row.dp), row.dst_sc, block, tag + ("near",))
    same(near, inp.words, tag + ("near",))
    src = fl.FarPlanes(L, w, h, row.sp, NF, fill_frames=inp.ex.s, kind="far16")
    given = fl.FarPlanes(L, tw, t_h, row.dp, NF, fill_frames=inp.g, kind="far16")
    assert src.t.numel() + given.t.numel() <= 12 * fl.GIB + (1 << 20), tag
    for pl in (src, given):
        assert all((NF - 1) * pl.pfs[p] >= 1 << 32 for p in range(3)), tag
    same(measured(c, src, row.src_sc, given, row.dst_sc, block, tag + ("far",), w=w, h=h), near, tag + ("far",))
    assert src.unchanged() and given.unchanged(), tag


# ---- 4. refusals
def test_refusals_launch_nothing(L):
    """every refusal before any launch, with its code and its message; where a call has two defects, which of the two is reported: the
    block first, then the plan's order (null arguments, the size, the profiles, the source quantizer, the layouts, the words, the
    supported set); the host forms: null arguments, the block, the staging"""
    import torch
    from lumahdrv_amd.capi import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, LumaHipError
    w, h = 64, 32
    luv = pk.side_cfg(fk.LUV, 3, 2)
    NAME = {None: "half-resolution transcode distortion", 16: "half-resolution transcode distortion map"}

    def lut(cfg):
        return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])

    def call(c, block, out_ptr, w=w, h=h, src=None, given=None, sp=2, dp=2, nf=2, src_ptrs=None, given_ptrs=None):
        args = (src_ptrs or src.ptrs, src.st, src.pfs, sp, 1.0, nf, w, h, given_ptrs or given.ptrs, given.st, given.pfs, dp, 1.0)
        if block is None:
            c.transcode_half_distortion_frames_device(*args, out_ptr)
        else:
            c.transcode_half_distortion_map_frames_device(*args, block, out_ptr)

    def attempt(c, code, text, blocks=(None, 16), out=None, **kw):
        for block in blocks:
            src, given = kw.pop("src", None) or Planes(L, 64, 32, 2, 2), kw.pop("given", None) or Planes(L, 32, 16, 2, 2)
            own = Words(shape_of(2, 32, 16, 16 if block else None))
            with pytest.raises(LumaHipError) as e:
                call(c, block, out(own, src, given) if out else own.ptr, src=src, given=given, **kw)
            msg = c.L.lumahip_last_error(c.h).decode()
            want = text.replace("%CALL%", NAME[16 if block else None])      # (a text ending in * : the message begins with it)
            assert e.value.code == code and (msg.startswith(want[:-1]) if want.endswith("*") else msg == want), (block, kw, code, msg)
            torch.cuda.synchronize()
            assert own.untouched() and src.unchanged() and given.unchanged(), (block, text, "a refused call wrote")
            kw.update(src=src, given=given)

    def works(c):
        for block in (None, 16):
            src, given = Planes(L, w, h, 2, 2), Planes(L, w // 2, h // 2, 2, 2)
            own = Words(shape_of(2, 32, 16, block))
            call(c, block, own.ptr, src=src, given=given)
            torch.cuda.synchronize()
            assert not own.untouched() and own.words(("works",)) is not None

    c = ctx(L, luv)
    attempt(c, ERR_STATE, "source quantizer not set (call lumahip_set_source_quantizer first)")
    attempt(ctx(L, luv, luv, quantizer=False), ERR_STATE, "quantizer not set (call lumahip_set_quantizer first)")
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    # the block: outside {16, 32, 64}, and in front of every other defect
    own, src, given = Words(shape_of(2, 32, 16, 16)), Planes(L, 64, 32, 2, 2), Planes(L, 32, 16, 2, 2)
    for bad in (8, 48, 128):
        with pytest.raises(LumaHipError) as e:
            call(c, bad, own.ptr, src=src, given=given)
        assert e.value.code == ERR_ARG and str(e.value).endswith("%s: block must be 16, 32 or 64 (got %d)" % (NAME[16], bad)), str(e.value)
    with pytest.raises(LumaHipError) as e:      # block 8 + w not a multiple of 4: the block
        call(c, 8, own.ptr, w=62, src=src, given=given)
    assert str(e.value).endswith("block must be 16, 32 or 64 (got 8)") and own.untouched(), str(e.value)
    # null arguments
    for k in (0, 8):                                         # (with a bad block: the block comes first, as in every plan)
        fn = c.L.lumahip_transcode_half_distortion_frames_device if k == 0 else c.L.lumahip_transcode_half_distortion_map_frames_device
        rc = fn(c.h, None, None, None, 2, 1.0, 2, w, h, None, None, None, 2, 1.0, *((None,) if k == 0 else (16, None)))
        assert rc == ERR_ARG and c.L.lumahip_last_error(c.h).decode() == "null argument", k
    gnull = Planes(L, 32, 16, 2, 2)
    attempt(c, ERR_ARG, "null plane 1", given=gnull, given_ptrs=[gnull.ptrs[0], None, gnull.ptrs[2]])
    attempt(c, ERR_ARG, "out_dev must be non-null and 8-byte aligned", blocks=(None,), out=lambda own, s, g: None)
    attempt(c, ERR_ARG, "map_dev must be non-null and 8-byte aligned", blocks=(16,), out=lambda own, s, g: own.ptr + 4)
    # w or h not a multiple of 4: even, and odd (odd: the size's own message comes first)
    for bad in ((62, 32), (66, 32), (64, 30), (64, 34)):
        attempt(c, ERR_ARG, "Invalid frame size %dx%d (half resolution: must be multiples of 4)" % bad, w=bad[0], h=bad[1],
                src=Planes(L, 68, 36, 2, 2), given=Planes(L, 34, 18, 2, 2))
    attempt(c, ERR_ARG, "Invalid frame size 63x32 (must be even, non-zero)", w=63)
    # profiles out of range; with w not a multiple of 4 as well: the target's profile is check_geom's, in front of it, the source's behind
    attempt(c, ERR_ARG, "profile must be 0..3 (got 4)", dp=4)
    attempt(c, ERR_ARG, "profile must be 0..3 (got -1)", dp=-1, w=62)
    attempt(c, ERR_ARG, "source profile must be 0..3 (got 4)", sp=4)
    attempt(c, ERR_ARG, "Invalid frame size 62x32 (half resolution: must be multiples of 4)", sp=4, w=62)
    # the layouts: the source is checked at w x h, the given set at (w/2) x (h/2)
    attempt(c, ERR_ARG, "plane 0: stride 64 < row bytes 128", src=Planes(L, 32, 16, 2, 2, strides=(64, 32, 32)))
    attempt(c, ERR_ARG, "plane 0: stride 32 < row bytes 64", given=Planes(L, 16, 8, 2, 2, strides=(32, 16, 16)))
    attempt(c, ERR_ARG, "plane 0: frame stride %d < plane size %d" % (8 * 128 + GAP, 16 * 128), given=Planes(L, 32, 8, 2, 2, strides=(128, 64, 64)))
    # a given set laid out for w x h where (w/2) x (h/2) is read: accepted, and its extents stop short of the layout's -- the words may
    # lie behind the last half-size row of the last frame, inside what a w x h set would cover, and may not lie inside that row
    big = Planes(L, w, h, 2, 2)
    last_row = big.pfs[0] + 15 * big.st[0]      # plane 0: the last row of (w/2) x (h/2) in frame 1, 64 bytes of it read
    own = Words(shape_of(2, 32, 16, None))
    spare = big.ptrs[0] + last_row + 64
    assert spare % 8 == 0 and last_row + 64 + 2 * 96 <= big.pfs[0] + 32 * big.st[0]
    before = big.host()
    call(c, None, spare, src=Planes(L, w, h, 2, 2), given=big)       # 24 words right behind the extent: taken
    torch.cuda.synchronize()
    assert not all(np.array_equal(a, b) for a, b in zip(before, big.host())), "the words were not written"
    attempt(c, ERR_ARG, "out_dev overlaps given plane 0", blocks=(None,), given=Planes(L, w, h, 2, 2),
            out=lambda own, s, g: g.ptrs[0] + g.pfs[0] + 15 * g.st[0] + 56)
    attempt(c, ERR_ARG, "map_dev overlaps given plane 2", blocks=(16,), out=lambda own, s, g: g.ptrs[2] + 8)
    # the source's extent is the w x h one: its last row of frame 1, which a half-size extent would not reach
    attempt(c, ERR_ARG, "out_dev overlaps source plane 0", blocks=(None,), out=lambda own, s, g: s.ptrs[0] + s.pfs[0] + 31 * s.st[0] + 120)
    attempt(c, ERR_ARG, "map_dev overlaps source plane 1", blocks=(16,), out=lambda own, s, g: s.ptrs[1] + s.pfs[1] + 15 * s.st[1] + 56)
    # the words overlapping a set + an unsupported colour space: the overlap
    works(c)
    for cs in (1, 3):                                        # RGB / XYZ on either side
        bad = (1, 11, cs, 8, 1e4, 0.005)
        c.set_source_quantizer(*bad, lut(bad))
        attempt(c, ERR_UNSUPPORTED, "%%CALL%%: colour spaces Lu'v' and YCbCr only (source %d, target 0)" % cs)
        attempt(c, ERR_ARG, "out_dev overlaps source plane 0", blocks=(None,), out=lambda own, s, g: s.ptrs[0] + 64)
        c.set_source_quantizer(*luv, lut(luv))
        works(c)
        attempt(ctx(L, bad, luv), ERR_UNSUPPORTED, "%%CALL%%: colour spaces Lu'v' and YCbCr only (source 0, target %d)" % cs)
    deep = (1, 14, 0, 8, 1e4, 0.005)                         # source bit depth 14
    c.set_source_quantizer(*deep, lut(deep))
    attempt(c, ERR_UNSUPPORTED, "%CALL%: the source's luminance table must be staged in LDS (bit depth <= 12, got 14)")
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    c.tune("force_literal", 1)                               # target records not in LDS
    attempt(c, ERR_UNSUPPORTED, "%CALL%: the target needs its luminance records in LDS (search mode *")
    c.tune("force_literal", 0)
    works(c)
    big_t, y12 = (1, 13, 0, 8, 1e4, 0.005), (1, 12, 2, 12, 1000.0, 0.01)   # 136 KiB of records + a 12-bit YCbCr source: beyond 160 KiB
    c3 = ctx(L, big_t, y12)
    for block in (None, 16):
        own, src, given = Words(shape_of(2, 32, 16, block)), Planes(L, 64, 32, 2, 2), Planes(L, 32, 16, 2, 2)
        with pytest.raises(LumaHipError) as e:
            call(c3, block, own.ptr, src=src, given=given)
        assert own.untouched() and e.value.code == ERR_UNSUPPORTED and ("%s: the tables of both sides take " % NAME[block]) in str(e.value) and \
            str(e.value).endswith("bytes of LDS, a workgroup has 163840"), str(e.value)
    c3.set_source_quantizer(*luv, lut(luv))                  # ... while PQ-11 Lu'v' beside the 13-bit target fits
    works(c3)
    # the host forms: null arguments, then the block, then the staging
    sp = [np.zeros((32, 128), np.uint8), np.zeros((16, 64), np.uint8), np.zeros((16, 64), np.uint8)]
    gp = [np.zeros((16, 64), np.uint8), np.zeros((8, 32), np.uint8), np.zeros((8, 32), np.uint8)]
    for fn, kw, code, text in (
            ("transcode_half_distortion_map_frame", dict(w=62), ERR_ARG, "Invalid frame size 62x32 (half resolution: must be multiples of 4)"),
            ("transcode_half_distortion_frame", dict(h=30), ERR_ARG, "Invalid frame size 64x30 (half resolution: must be multiples of 4)"),
            ("transcode_half_distortion_frame", dict(gst=(32, 32, 32)), ERR_ARG, "given plane 0: null or stride 32 < row bytes 64"),
            ("transcode_half_distortion_frame", dict(sst=(64, 64, 64)), ERR_ARG, "source plane 0: null or stride 64 < row bytes 128")):
        kw = dict(dict(w=w, h=h, sst=(128, 64, 64), gst=(64, 32, 32)), **kw)
        with pytest.raises(LumaHipError) as e:
            getattr(c, fn)(sp, kw["sst"], kw["w"], kw["h"], gp, kw["gst"], **({"block": kw["block"]} if "block" in kw else {}))
        assert e.value.code == code and str(e.value).endswith(text), (fn, kw, str(e.value))
    with pytest.raises(LumaHipError) as e:
        ctx(L, luv).transcode_half_distortion_frame(sp, (128, 64, 64), w, h, gp, (64, 32, 32))
    assert e.value.code == ERR_STATE and str(e.value).endswith("source quantizer not set (call lumahip_set_source_quantizer first)")
    rc = c.L.lumahip_transcode_half_distortion_map_frame_host(c.h, None, None, 2, 1.0, 62, h, None, None, 2, 1.0, 8, None, 0)
    assert rc == ERR_ARG and c.L.lumahip_last_error(c.h).decode() == "null argument"
    out = np.zeros(12, dtype=np.uint64)
    args = ((C.c_void_p * 3)(*[p.ctypes.data for p in sp]), (C.c_int * 3)(128, 64, 64), 2, 1.0, w, h,
            (C.c_void_p * 3)(*[p.ctypes.data for p in gp]), (C.c_int * 3)(64, 32, 32), 2, 1.0)
    # (the block through the C symbol: Context's map methods ask lumahip_distortion_map_dims for the array's size first, which refuses
    #  a bad block in its own words)
    bad = args[:4] + (62,) + args[5:]
    rc = c.L.lumahip_transcode_half_distortion_map_frame_host(c.h, *bad, 8, out.ctypes.data, 12)       # block 8 + w 62: the block
    assert rc == ERR_ARG and c.L.lumahip_last_error(c.h).decode() == NAME[16] + ": block must be 16, 32 or 64 (got 8)"
    rc = c.L.lumahip_transcode_half_distortion_map_frame_host(c.h, *bad, 16, out.ctypes.data, 12)      # w 62 + too few words: the staging
    assert rc == ERR_ARG and c.L.lumahip_last_error(c.h).decode() == "Invalid frame size 62x32 (half resolution: must be multiples of 4)"
    assert not out.any()
    rc = c.L.lumahip_transcode_half_distortion_map_frame_host(c.h, *args, 16, out.ctypes.data, 12)    # 2 x 1 blocks: 24 words
    assert rc == ERR_ARG and c.L.lumahip_last_error(c.h).decode() == NAME[16] + ": 12 words for a map of 24"
    works(c)
