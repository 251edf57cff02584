"""Plane-to-plane measures (include/lumahip_compare.h): lumahip_planes_distortion_frames_device, lumahip_planes_distortion_map_frames_device,
lumahip_planes_moments_map_frames_device and their host forms -- two sets of code planes compared as they are, e from set A and g from
set B, no quantizer.  Every expectation is exact equality of integers; before every call the output holds the 0xC3 pattern with 16
guard words behind it, which must survive (the per-frame words' too: tests/support/planes_measure.py frame_buf / frame_words); both
plane sets and the sentinel bytes in their paddings and gaps must be as they were after every case.

1. Against numpy (tests/support/host.py, moments.py): profiles 0-3 x sizes (6,4) (34,18) (258,6) (260,6) (264,70) (64,32) x 3 distinct
   frames with a gap between them, all three calls, all blocks; the maps fold to the per-frame words and to each other.
2. The existing cells from the third side: A = what lumahip_encode_frames_device wrote -> word for word the three frame-fed measuring
   calls on the frames (floats and halves) with the same B; A = what lumahip_transcode_frames_device wrote -> the three transcode
   measuring calls.
3. Layouts: each set odd (byte loads), half-aligned and aligned, nine combinations; widths that take two pixels per thread only.
4. Overlap: B = A one frame later in one buffer; A = B exactly.   5. Range: 0 against 0xFFFF / 0xFF.
6. Launch shapes.   7. Context: no quantizer; both quantizers untouched; a 720p frame twice and in an unordered section; host forms.
8. Refusals, each leaving the output untouched.
"""
import ctypes as C

import numpy as np
import pytest

from tests.support.device import (Frames, L, Planes, ctx, dist, dist_map, encode, from_frames, inputs_as_before, map_buf, measure,  # noqa: F401  (L is the module fixture)
                                  random_planes, tmap, transcoded)
from tests.support.host import (BLOCKS, CFG, GAP, GUARD, OUT_FILL, SENTINEL, expect, expect_map, float_frames, layout, map_words, nwords,
                                planes_from_frames)
from tests.support.moments import MOM_BLOCKS, expect_moments, mom_map, mom_nwords, mom_words
from tests.support.planes_measure import (NF, all_three, case_rng, folds, frame_buf, frame_words, model, numpy_cases, pdist, pmap, pmom,
                                          same_results, swapped, two_sets)
from tests.support.transcode_moments import given_frames, kept_block, own_planes_moments, tmom

pytestmark = pytest.mark.gpu


def put(L, frames, w, h, profile, st=None, base=0, gap=GAP):
    """the frames on the device in rows st[p] bytes apart (the library's own strides by default), `base` bytes into their buffers, the
    sentinel in every padding and gap"""
    st = tuple(int(s) for s in (st if st is not None else L.plane_geometry(w, h, profile)[2]))
    fill = planes_from_frames(frames, w, h, profile, st, "sentinel", gap, base)
    return Planes(L, w, h, profile, len(frames), fill=fill, strides=st, gap=gap, base=base)


def bare(L):
    """a context that never had a quantizer set"""
    return ctx(L, None, quantizer=False)


# ---- 1. against numpy
@pytest.mark.parametrize("profile", range(4))
def test_equals_numpy(L, profile):
    c = bare(L)
    n = 0
    for prof, w, h in numpy_cases():
        if prof != profile:
            continue
        fa, fb, _ = two_sets(case_rng(profile, w, h), w, h, profile)
        a, b = put(L, fa, w, h, profile), put(L, fb, w, h, profile)
        abefore, bbefore = a.host(), b.host()
        tag = (profile, w, h)
        want = model(fa, fb, w, h, profile)
        got = all_three(c, a, b)
        same_results(got, want, tag)
        folds(*got, tag)
        inputs_as_before(a, abefore, b, bbefore, tag)
        # exchanging the sets: the same differences, the moments' words 0 <-> 1 and 2 <-> 3
        assert np.array_equal(pdist(c, b, a), want[0]), tag
        blk = MOM_BLOCKS[n % 4]
        assert np.array_equal(pmom(c, b, a, blk), swapped(want[2][blk])), tag + (blk, "swapped")
        n += 1
    assert n == 6


# ---- 2. the existing cells from the third side
@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10", "pq12_rgb", "linear12_xyz"])
def test_equals_the_frame_fed_calls_on_the_encode_calls_planes(L, name, halves):
    cfg = CFG[name]
    c, cmp_ctx = ctx(L, cfg), bare(L)
    rng = np.random.default_rng(len(name) + 2 * halves)
    sc = 20.0 if cfg[2] == 2 else 1.0
    for profile in (2, 3):
        for (w, h) in ((264, 70), (34, 18)):
            frames = float_frames(rng, NF, w, h, halves=True)
            a, abufs = encode(c, L, Frames(frames), sc, profile)
            fr, form = (Frames(frames, dtype=np.float16), "f16") if halves else (Frames(frames), "packed")
            b = from_frames(L, given_frames(rng, a, abufs, w, h, profile, kept_block(w, h, MOM_BLOCKS)), w, h, profile, padding="source")
            bbefore = b.host()
            tag = (name, halves, profile, w, h)
            want = (dist(c, fr, sc, b, form), {blk: dist_map(c, fr, sc, b, blk, form) for blk in BLOCKS},
                    {blk: mom_map(c, fr, sc, b, blk, form) for blk in MOM_BLOCKS})
            assert want[0][..., 3].all() and not own_planes_moments(want[2][8]), tag
            same_results(all_three(cmp_ctx, a, b), want, tag)
            same_results(all_three(c, a, b), want, tag)   # (and on the context that holds the quantizer)
            inputs_as_before(a, abufs, b, bbefore, tag)
            assert fr.unchanged(), tag


@pytest.mark.parametrize("sname,dname,sp,dp", [("pq11_luv8", "log12_luv8", 2, 2), ("pq11_luv8", "pq10_ycbcr10", 3, 2),
                                               ("pq10_ycbcr10", "pq11_luv8", 0, 3), ("pq10_ycbcr10", "pq10_ycbcr10_4000", 2, 3)])
def test_equals_the_transcode_measuring_calls_on_the_transcode_calls_planes(L, sname, dname, sp, dp):
    c, cmp_ctx = ctx(L, CFG[dname], CFG[sname]), bare(L)
    src_sc, dst_sc = (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)
    rng = np.random.default_rng(sp * 4 + dp)
    for (w, h) in ((264, 70), (34, 18)):
        src = random_planes(L, rng, w, h, sp, NF)
        a, abufs = transcoded(c, L, src, src_sc, dp, dst_sc)
        b = from_frames(L, given_frames(rng, a, abufs, w, h, dp, kept_block(w, h, MOM_BLOCKS)), w, h, dp, padding="source")
        bbefore = b.host()
        tag = (sname, dname, sp, dp, w, h)
        want = (measure(c, src, src_sc, b, dst_sc), {blk: tmap(c, src, src_sc, b, dst_sc, blk) for blk in BLOCKS},
                {blk: tmom(c, src, src_sc, b, dst_sc, blk) for blk in MOM_BLOCKS})
        assert want[0][..., 3].all() and not own_planes_moments(want[2][8]), tag
        same_results(all_three(cmp_ctx, a, b), want, tag)
        inputs_as_before(a, abufs, b, bbefore, tag)


# ---- 3. layouts
LAYOUTS = {"odd": dict(base=1, pad=5, gap=GAP + 1), "half": dict(base=4, pad=None, gap=GAP), "aligned": dict(base=0, pad=None, gap=GAP)}


def laid_out(L, frames, w, h, profile, kind):
    """odd: every base and stride odd (byte loads); half: bases 4 bytes off -- the vector accesses of two pixels per thread and row, not
    of four; aligned: both"""
    lay = LAYOUTS[kind]
    st = None
    if lay["pad"] is not None:
        st = tuple((layout_row_bytes(w, h, profile, p) + lay["pad"]) | 1 for p in range(3))
    return put(L, frames, w, h, profile, st=st, base=lay["base"], gap=lay["gap"])


def layout_row_bytes(w, h, profile, p):
    from tests.support.host import plane_rows
    return plane_rows(w, h, profile, p)[1]


@pytest.mark.parametrize("profile", [2, 3])
def test_nine_layout_combinations(L, profile):
    c = bare(L)
    w, h = 264, 70
    fa, fb, _ = two_sets(case_rng(profile, w, h), w, h, profile)
    want = model(fa, fb, w, h, profile)
    n = 0
    for ka in LAYOUTS:
        for kb in LAYOUTS:
            a, b = laid_out(L, fa, w, h, profile, ka), laid_out(L, fb, w, h, profile, kb)
            abefore, bbefore = a.host(), b.host()
            same_results(all_three(c, a, b), want, (profile, ka, kb))
            inputs_as_before(a, abefore, b, bbefore, (profile, ka, kb))
            n += 1
    assert n == 9


@pytest.mark.parametrize("profile", range(4))
def test_widths_that_take_two_pixels_per_thread_only(L, profile):
    c = bare(L)
    for (w, h) in ((258, 6), (34, 18), (6, 4), (130, 66)):
        assert w % 4 == 2
        fa, fb, _ = two_sets(case_rng(profile, w, h), w, h, profile)
        want = model(fa, fb, w, h, profile)
        for ka, kb in (("aligned", "aligned"), ("aligned", "odd"), ("odd", "aligned")):
            a, b = laid_out(L, fa, w, h, profile, ka), laid_out(L, fb, w, h, profile, kb)
            abefore, bbefore = a.host(), b.host()
            same_results(all_three(c, a, b), want, (profile, w, h, ka, kb))
            inputs_as_before(a, abefore, b, bbefore, (profile, w, h, ka, kb))


# ---- 4. overlap
@pytest.mark.parametrize("profile", range(4))
def test_b_is_a_one_frame_later_and_a_is_b(L, profile):
    c = bare(L)
    for (w, h) in ((264, 70), (34, 18)):
        fa, _, _ = two_sets(case_rng(profile, w, h), w, h, profile, nf=4)
        a = put(L, fa, w, h, profile)
        abefore = a.host()
        later = [a.ptrs[p] + a.pfs[p] for p in range(3)]
        want = model(fa[:-1], fa[1:], w, h, profile)
        assert want[0][..., 3].all()
        same_results(all_three(c, a, a, b_ptrs=later, nf=3), want, (profile, w, h, "one frame later"))
        frame, maps, moms = all_three(c, a, a)
        assert not frame.any() and not any(m.any() for m in maps.values()), (profile, w, h, "A against itself")
        assert all(own_planes_moments(m) for m in moms.values())
        same_results((frame, maps, moms), model(fa, fa, w, h, profile), (profile, w, h, "A against itself"))
        inputs_as_before(a, abefore, a, abefore, (profile, w, h))


# ---- 5. range
@pytest.mark.parametrize("profile", range(4))
def test_zeros_against_all_ones(L, profile):
    c = bare(L)
    w, h = 264, 70
    st = tuple(int(s) for s in L.plane_geometry(w, h, profile)[2])
    pfs = layout(w, h, profile, st)[2]
    zeros = Planes(L, w, h, profile, 1, fill=[np.zeros(pfs[p], dtype=np.uint8) for p in range(3)])
    ones = Planes(L, w, h, profile, 1, fill=[np.full(pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
    top = 0xFFFF if profile > 1 else 0xFF
    want = (expect(zeros, zeros.fill, ones, ones.fill), {blk: expect_map(zeros, zeros.fill, ones, ones.fill, blk) for blk in BLOCKS},
            {blk: expect_moments(zeros, zeros.fill, ones, ones.fill, blk) for blk in MOM_BLOCKS})
    assert int(want[0][0, 0, 0]) == w * h * top * top and np.all(want[0][..., 2] == top) and int(want[0][0, 0, 3]) == w * h
    if profile > 1:
        assert np.all(want[0][..., 0] > np.uint64(1) << np.uint64(32)) and int(want[2][64][0, 0, 0, 0, 3]) == 4096 * 65535 ** 2
    same_results(all_three(c, zeros, ones), want, (profile,))
    back = all_three(c, ones, zeros)
    assert np.array_equal(back[0], want[0]) and all(np.array_equal(back[2][blk], swapped(want[2][blk])) for blk in MOM_BLOCKS)
    assert zeros.unchanged() and ones.unchanged()   # (planes of one byte value throughout: their paddings and gaps hold it too)


# ---- 6. launch shapes
@pytest.mark.parametrize("profile", [2, 3, 0])
def test_launch_shapes_give_identical_words(L, profile):
    shapes = {}
    for shape in ("default", "two_workgroups_of_64", "1024_threads"):
        c = bare(L)
        if shape == "two_workgroups_of_64":      # the persistent loop across frames, the most sub-tiles per map tile
            c.tune("block", 64)
            c.tune("grid_enc", 2)
        elif shape == "1024_threads":            # clamped to 32 * block threads (256 at block 8, 512 at 16)
            c.tune("block", 1024)
        shapes[shape] = c
    for (w, h) in ((264, 70), (258, 6), (34, 18)):   # four pixels per thread, two, two
        fa, fb, _ = two_sets(case_rng(profile, w, h), w, h, profile)
        a, b = put(L, fa, w, h, profile), put(L, fb, w, h, profile)
        abefore, bbefore = a.host(), b.host()
        want = model(fa, fb, w, h, profile)
        for shape, c in shapes.items():
            same_results(all_three(c, a, b), want, (profile, w, h, shape))
            inputs_as_before(a, abefore, b, bbefore, (profile, w, h, shape))


# ---- 7. context
def test_a_context_with_both_quantizers_keeps_them(L):
    c = ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    rng = np.random.default_rng(9)
    w, h, profile = 64, 32, 2
    src = random_planes(L, rng, w, h, profile, NF)
    info = c.quantizer_info()
    _, before = transcoded(c, L, src, 1.0, profile, 20.0)
    fa, fb, _ = two_sets(rng, w, h, profile)
    a, b = put(L, fa, w, h, profile), put(L, fb, w, h, profile)
    abefore, bbefore = a.host(), b.host()
    same_results(all_three(c, a, b), model(fa, fb, w, h, profile), ("both quantizers",))
    inputs_as_before(a, abefore, b, bbefore, ("both quantizers",))
    _, after = transcoded(c, L, src, 1.0, profile, 20.0)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert c.quantizer_info() == info


def test_one_720p_frame_twice_and_in_an_unordered_section(L):
    import torch
    c = bare(L)
    w, h, profile = 1280, 720, 2
    fa, fb, _ = two_sets(np.random.default_rng(722), w, h, profile, nf=1)
    a, b = put(L, fa, w, h, profile), put(L, fb, w, h, profile)
    abefore, bbefore = a.host(), b.host()
    ha, hb = a, b
    exp_frame = expect(ha, abefore, hb, bbefore)
    exp_map = expect_map(ha, abefore, hb, bbefore, 16)
    exp_mom = expect_moments(ha, abefore, hb, bbefore, 8)
    for _ in range(2):
        assert np.array_equal(pdist(c, a, b), exp_frame)
        assert np.array_equal(pmap(c, a, b, 16), exp_map)
        assert np.array_equal(pmom(c, a, b, 8), exp_mom)
    outs = [frame_buf(1) for _ in range(2)]
    maps = [map_buf(nwords(1, w, h, 16)) for _ in range(2)]
    moms = [map_buf(mom_nwords(1, w, h, 8)) for _ in range(2)]
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for o, m, q in zip(outs, maps, moms):
        c.planes_distortion_frames_device(a.ptrs, a.st, a.pfs, 1, w, h, b.ptrs, b.st, b.pfs, profile, o.data_ptr())
        c.planes_distortion_map_frames_device(a.ptrs, a.st, a.pfs, 1, w, h, b.ptrs, b.st, b.pfs, profile, 16, m.data_ptr())
        c.planes_moments_map_frames_device(a.ptrs, a.st, a.pfs, 1, w, h, b.ptrs, b.st, b.pfs, profile, 8, q.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for o, m, q in zip(outs, maps, moms):
        assert np.array_equal(frame_words(o, 1), exp_frame)
        assert np.array_equal(map_words(m, 1, w, h, 16), exp_map)
        assert np.array_equal(mom_words(q, 1, w, h, 8), exp_mom)
    inputs_as_before(a, abefore, b, bbefore, ("720p",))


@pytest.mark.parametrize("profile", range(4))
def test_host_forms_equal_the_device_forms(L, profile):
    c = bare(L)
    for (w, h) in ((264, 70), (34, 18)):
        fa, fb, st = two_sets(case_rng(profile, w, h), w, h, profile, nf=1)
        a, b = put(L, fa, w, h, profile), put(L, fb, w, h, profile)
        abefore, bbefore = a.host(), b.host()
        keep = [[p.copy() for p in fr] for fr in (fa[0], fb[0])]
        frame, maps, moms = all_three(c, a, b)
        inputs_as_before(a, abefore, b, bbefore, (profile, w, h))
        hw = c.planes_distortion_frame(fa[0], st, w, h, fb[0], st, profile)
        assert hw.dtype == np.uint64 and hw.shape == (3, 4) and np.array_equal(hw, frame[0]), (profile, w, h, hw, frame)
        for blk in BLOCKS:
            hm = c.planes_distortion_map_frame(fa[0], st, w, h, fb[0], st, profile, blk)
            assert hm.dtype == np.uint64 and np.array_equal(hm, maps[blk][0]), (profile, w, h, blk)
        for blk in MOM_BLOCKS:
            hq = c.planes_moments_map_frame(fa[0], st, w, h, fb[0], st, profile, blk)
            assert hq.dtype == np.uint64 and np.array_equal(hq, moms[blk][0]), (profile, w, h, blk)
        # the host forms leave the caller's planes, paddings included, as they were
        assert all(np.array_equal(x, y) for got, was in zip((fa[0], fb[0]), keep) for x, y in zip(got, was)), (profile, w, h)


# ---- 8. refusals: nothing is launched, the output is left as it was
def test_refusals_leave_the_output_untouched(L):
    import torch
    from lumahdrv_amd.capi import ERR_ARG, LumaHipError
    w, h, profile, nf = 64, 32, 2, 1
    c = bare(L)
    a, b = Planes(L, w, h, profile, nf), Planes(L, w, h, profile, nf)
    calls = {"frame": (c.planes_distortion_frames_device, None, nf * 12 + GUARD),
             "map": (c.planes_distortion_map_frames_device, 16, nwords(nf, w, h, 16) + GUARD),
             "moments": (c.planes_moments_map_frames_device, 8, mom_nwords(nf, w, h, 8) + GUARD)}

    def refused(what, w=w, h=h, profile=profile, block="own", a_ptrs=None, a_st=None, out_ptr="own"):
        fn, blk, words = calls[what]
        buf = torch.full((words,), OUT_FILL, dtype=torch.int64, device=a.t[0].device)
        ptr = buf.data_ptr() if out_ptr == "own" else out_ptr(buf)
        tail = (ptr,) if blk is None else (blk if block == "own" else block, ptr)
        with pytest.raises(LumaHipError) as ei:
            fn(a.ptrs if a_ptrs is None else a_ptrs, a.st if a_st is None else a_st, a.pfs, nf, w, h, b.ptrs, b.st, b.pfs, profile, *tail)
        assert ei.value.code == ERR_ARG, (what, ei.value)
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == OUT_FILL), (what, "an error return wrote to the output or to the guard words behind it")
        assert all(np.all(x == SENTINEL) for x in a.host() + b.host())

    for what in calls:
        refused(what, w=63)                                                # odd w
        refused(what, h=31)                                                # odd h
        refused(what, a_st=(a.st[0], a.st[1] // 4, a.st[2]))               # a stride below the row
        refused(what, profile=4)                                           # profile 4
        refused(what, a_ptrs=[a.ptrs[0], None, a.ptrs[2]])                 # a null plane
        refused(what, out_ptr=lambda o: None)                              # a null output
        refused(what, out_ptr=lambda o: o.data_ptr() + 4)                  # a misaligned output
        refused(what, out_ptr=lambda o: a.ptrs[0] + 64)                    # an output inside A
        refused(what, out_ptr=lambda o: b.ptrs[2] + 8)                     # ... inside B
        refused(what, out_ptr=lambda o: b.ptrs[1] - 40)                    # ... reaching into B from in front of it
    refused("map", block=8)                                                # block 8 is the moments map's only
    for what in ("map", "moments"):
        refused(what, block=4)
        refused(what, block=128)
    # the host forms: word counts one too small, and the same blocks
    pa, pb = a.frame(a.host(), 0), b.frame(b.host(), 0)
    args = ((C.c_void_p * 3)(*[p.ctypes.data for p in pa]), (C.c_int * 3)(*a.st), w, h,
            (C.c_void_p * 3)(*[p.ctypes.data for p in pb]), (C.c_int * 3)(*b.st), profile)
    for fn, blk, need in ((c.L.lumahip_planes_distortion_map_frame_host, 16, nwords(1, w, h, 16)),
                          (c.L.lumahip_planes_moments_map_frame_host, 8, mom_nwords(1, w, h, 8))):
        m = np.full(need + GUARD, OUT_FILL, dtype=np.int64)
        assert fn(c.h, *args, blk, m.ctypes.data, need - 1) == ERR_ARG and np.all(m == OUT_FILL)
        assert fn(c.h, *args, 4, m.ctypes.data, need) == ERR_ARG and np.all(m == OUT_FILL)
        assert fn(c.h, *args, 128, m.ctypes.data, need) == ERR_ARG and np.all(m == OUT_FILL)
        assert fn(c.h, *args, blk, m.ctypes.data, need) == 0 and np.all(m[need:] == OUT_FILL) and not np.any(m[:need] == OUT_FILL)
    m = np.full(nwords(1, w, h, 16) + GUARD, OUT_FILL, dtype=np.int64)
    assert c.L.lumahip_planes_distortion_map_frame_host(c.h, *args, 8, m.ctypes.data, m.size) == ERR_ARG and np.all(m == OUT_FILL)
    o = np.full(12 + GUARD, OUT_FILL, dtype=np.int64)
    assert c.L.lumahip_planes_distortion_frame_host(c.h, *args, o.ctypes.data) == 0 and np.all(o[12:] == OUT_FILL) and not o[:12].any()
    # ... and the same arguments are accepted: planes of the sentinel against themselves
    assert not pdist(c, a, b).any() and pmap(c, a, b, 16).shape == (1, 2, 4, 3, 4) and own_planes_moments(pmom(c, a, b, 8))
