"""Transcode moments map (include/lumahip_measure.h lumahip_transcode_moments_map_frames_device / _frame_host): the moments map's five
sums per plane {sum e, sum g, sum e^2, sum g^2, sum e g} for every block of 8, 16, 32 or 64 luma pixels squared of the target, e the
transcode of source code planes, written by one launch.  Every expectation is exact equality of integers
(tests/support/moments.py expected_moments_map); before every call the buffer holds the 0xC3 pattern with 16 guard words behind it,
which must survive; both plane sets and the sentinel bytes in their paddings and gaps must be as they were.

1. The reference's own decode -> encode (tests/golden/ref_transcode.npz): the fixture's own planes give Se == Sg and
   See == Sgg == Seg, a perturbed copy numpy's map; device call and host form, every block size.
2. Against lumahip_transcode_frames_device into scratch planes + numpy: nine configuration pairs x all 16 profile pairs x 3 frames x
   preScalings from {1, 20, 0.01} x sizes (34,18) (260,6) (258,6) (264,70) (64,32) (6,4); every block at (264,70) -- 33 block columns
   at block 8: one map tile of 32 blocks plus one at four pixels per thread -- and (34,18), the block rotating at the others.
3. Ties, in every case of 2: See - 2 Seg + Sgg is lumahip_transcode_distortion_map_frames_device's sse, the 8-map folds to the 16-map
   and so on up, and summed over a frame's blocks it is lumahip_transcode_distortion_frames_device's sse.
4. Odd given strides and source planes misaligned by two bytes.   5. Sums beyond 2^32, four and two pixels per thread.
6. Launch shapes: the default, 2 workgroups of 64 threads, 1024 threads asked for.   7. A 720p frame twice and in an unordered section.
8. Errors: nothing is launched.   9. Both quantizers untouched.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden import make_transcode_golden as mg
from tests.support.device import (L, Planes, ctx, dev, from_frames, inputs_as_before, map_buf, measure, random_planes, tmap,  # noqa: F401  (L is the module fixture)
                                  transcoded)
from tests.support.host import BLOCKS, CFG, GUARD, OUT_FILL, PAIRS, SENTINEL, fixture_cases, nwords, perturb, perturbed
from tests.support.moments import MOM_BLOCKS, expect_moments, expected_moments_map, fold_2x2, mom_nwords, mom_words, sse_of
from tests.support.transcode_moments import (ALL_BLOCKS_AT, blocks_at, frame_sse, given_frames, kept_block,
                                             own_planes_moments, pairs_cases, tmom)

pytestmark = pytest.mark.gpu

SCS = (1.0, 20.0, 0.01)


def scs_of(sname, dname):
    return (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)


# ---- 1. the reference's own decode -> encode
def test_reference_fixture_and_its_perturbed_copy(L, golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    ctxs, n = {}, 0
    for k, case, w, h, sp in fixture_cases(gt):
        sname, src_sc, dname, dst_sc = mg.CASES[case]
        c = ctxs.setdefault(case, ctx(L, mg.CONFIGS[dname], mg.CONFIGS[sname]))
        planes, st = mg.source_planes(gp, sname, w, h, sp)
        fix = [gt[k + "_plane%d" % p] for p in range(3)]
        est = tuple(int(s) for s in gt[k + "_stride"])
        bad = perturbed(fix, w, h, mg.DST_PROFILE)
        src = from_frames(L, [planes], w, h, sp, strides=st, padding="source")
        sbefore = src.host()
        for block in MOM_BLOCKS:
            own = expected_moments_map(fix, fix, w, h, mg.DST_PROFILE, block)
            exp = expected_moments_map(fix, bad, w, h, mg.DST_PROFILE, block)
            assert own_planes_moments(own) and not own_planes_moments(exp), (k, block)
            for given, want in ((fix, own), (bad, exp)):
                gv = from_frames(L, [given], w, h, mg.DST_PROFILE, strides=est, padding="source")
                gbefore = gv.host()
                got = tmom(c, src, src_sc, gv, dst_sc, block)
                assert np.array_equal(got[0], want), (k, block, "device", got, want)
                inputs_as_before(src, sbefore, gv, gbefore, (k, block), sentinels=False)
                hw = c.transcode_moments_map_frame(planes, st, w, h, given, est, src_sc, sp, dst_sc, mg.DST_PROFILE, block)
                assert hw.dtype == np.uint64 and hw.shape == want.shape
                assert np.array_equal(hw, want), (k, block, "host", hw, want)
        n += 1
    assert n == 16


# ---- 2. against lumahip_transcode_frames_device into scratch planes, 3. and the ties to the calls that exist
@pytest.mark.parametrize("sname,dname", PAIRS)
def test_equals_numpy_on_the_transcode_calls_planes(L, sname, dname):
    c = ctx(L, CFG[dname], CFG[sname])
    if dname == "linear12_luv8":
        assert c.quantizer_info()["mode"] == 7, "the value-keyed records are what this pair is here for"
    rng = np.random.default_rng(len(sname) * 43 + len(dname))
    nf = 3
    cases = pairs_cases()
    for it, sp, dp, w, h in cases:
        src_sc, dst_sc = (float(x) for x in rng.choice(SCS, 2))
        src = random_planes(L, rng, w, h, sp, nf)
        sbefore = src.host()
        enc, ebufs = transcoded(c, L, src, src_sc, dp, dst_sc)
        blocks = blocks_at(w, h, it)
        given = from_frames(L, given_frames(rng, enc, ebufs, w, h, dp, kept_block(w, h, blocks)), w, h, dp, padding="source")
        gbefore = given.host()
        frame_words = measure(c, src, src_sc, given, dst_sc)
        got = {}
        for block in blocks:
            tag = (sname, dname, sp, dp, w, h, src_sc, dst_sc, block)
            exp = expect_moments(enc, ebufs, given, gbefore, block)
            assert not own_planes_moments(exp), tag   # (tests/test_transcode_moments_map_host.py holds given_frames to more)
            got[block] = tmom(c, src, src_sc, given, dst_sc, block)
            assert np.array_equal(got[block], exp), tag + (got[block], exp)
            if block in BLOCKS:
                sse = tmap(c, src, src_sc, given, dst_sc, block)[..., 0]
                assert sse.any() and np.array_equal(sse_of(got[block]), sse), tag + ("sse of the distortion map",)
            if block // 2 in got:
                assert np.array_equal(fold_2x2(got[block // 2]), got[block]), tag + ("fold",)
            assert np.array_equal(frame_sse(got[block]), frame_words[..., 0]), tag + ("frame sse",)
        inputs_as_before(src, sbefore, given, gbefore, (sname, dname, sp, dp, w, h))
    assert len(cases) == 96 and (264, 70) in ALL_BLOCKS_AT and -(-264 // 8) == 33


# ---- 4. byte loads (odd given strides) and two pixels per thread (source planes two bytes into their buffers)
@pytest.mark.parametrize("sname,dname", [("pq11_luv8", "pq10_ycbcr10"), ("pq10_ycbcr10", "log12_luv8"), ("pq11_luv8", "log12_luv8")])
def test_odd_given_strides_and_misaligned_source_planes(L, sname, dname):
    import torch
    c = ctx(L, CFG[dname], CFG[sname])
    rng = np.random.default_rng(34)
    nf = 3
    src_sc, dst_sc = (20.0, 1.0) if CFG[sname][2] == 2 else (1.0, 20.0)
    for (w, h) in ((64, 32), (34, 18)):
        for sp, dp in ((2, 2), (3, 1), (0, 3)):
            src = random_planes(L, rng, w, h, sp, nf)
            sbefore = src.host()
            enc, ebufs = transcoded(c, L, src, src_sc, dp, dst_sc)
            shifted = [torch.cat([torch.full((2,), SENTINEL, dtype=torch.uint8, device=dev()), t]) for t in src.t]
            frames = given_frames(rng, enc, ebufs, w, h, dp, 16)
            given = from_frames(L, frames, w, h, dp, padding="source")
            # the same samples in rows three bytes longer
            longer = [[np.concatenate([a, np.full((a.shape[0], 3), SENTINEL, np.uint8)], axis=1) for a in fr] for fr in frames]
            odd = from_frames(L, longer, w, h, dp, strides=tuple(s + 3 for s in enc.st), padding="source")
            gbefore, obefore = given.host(), odd.host()
            for block in MOM_BLOCKS:
                tag = (sname, dname, w, h, sp, dp, block)
                exp = expect_moments(enc, ebufs, given, gbefore, block)
                assert not own_planes_moments(exp) and np.array_equal(exp, expect_moments(enc, ebufs, odd, obefore, block)), tag
                assert np.array_equal(tmom(c, src, src_sc, odd, dst_sc, block), exp), tag + ("odd strides",)
                got = tmom(c, src, src_sc, given, dst_sc, block, src_ptrs=[t.data_ptr() + 2 for t in shifted])
                assert np.array_equal(got, exp), tag + ("misaligned source", got, exp)
                both = tmom(c, src, src_sc, odd, dst_sc, block, src_ptrs=[t.data_ptr() + 2 for t in shifted])
                assert np.array_equal(both, exp), tag + ("both",)
            inputs_as_before(src, sbefore, odd, obefore, (sname, dname, w, h, sp, dp))
            inputs_as_before(src, sbefore, given, gbefore, (sname, dname, w, h, sp, dp))
            for t, s in zip(shifted, src.t):
                assert bool((t[:2] == SENTINEL).all()) and torch.equal(t[2:], s)


# ---- 5. the 64-bit paths: Sgg of one block is about 1.76e13, Seg beyond 2^32
@pytest.mark.parametrize("vw4", [True, False])
def test_one_block_sums_beyond_32_bits(L, vw4):
    import torch
    c = ctx(L, CFG["log12_luv8"], CFG["pq11_luv8"])
    rng = np.random.default_rng(4)
    w, h, profile = 64, 64, 2
    src = random_planes(L, rng, w, h, profile, 1)
    enc, ebufs = transcoded(c, L, src, 1.0, profile, 1.0)
    ones = Planes(L, w, h, profile, 1, fill=[np.full(enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
    exp = expect_moments(enc, ebufs, ones, ones.host(), 64)
    assert exp.shape == (1, 1, 1, 3, 5) and int(exp[0, 0, 0, 0, 3]) == 4096 * 65535 ** 2 and 1.75e13 < float(exp[0, 0, 0, 0, 3]) < 1.77e13
    assert np.all(exp[..., 3] > np.uint64(1) << np.uint64(32)) and exp[0, 0, 0, 0, 4] > np.uint64(1) << np.uint64(32)
    ptrs = None
    if not vw4:   # a source plane two bytes into its buffer: two pixels per thread, 32 lanes per block
        shifted = [torch.cat([torch.full((2,), SENTINEL, dtype=torch.uint8, device=dev()), t]) for t in src.t]
        ptrs = [t.data_ptr() + 2 for t in shifted]
    got = tmom(c, src, 1.0, ones, 1.0, 64, src_ptrs=ptrs)
    assert np.array_equal(got, exp), (got, exp)


# ---- 6. launch shapes: one pair from each of the four colour-space families, four and two pixels per thread
@pytest.mark.parametrize("vw4", [True, False])
@pytest.mark.parametrize("sname,dname,sp,dp", [("pq11_luv8", "log12_luv8", 2, 2), ("pq11_luv8", "pq10_ycbcr10", 3, 0),
                                               ("pq10_ycbcr10", "pq11_luv8", 0, 3), ("pq10_ycbcr10", "pq10_ycbcr10_4000", 2, 1)])
def test_launch_shapes_give_identical_maps(L, sname, dname, sp, dp, vw4):
    import torch
    src_sc, dst_sc = scs_of(sname, dname)
    rng = np.random.default_rng(60 + sp)
    nf = 3
    shapes = {}
    for shape in ("default", "two_workgroups_of_64", "1024_threads"):
        c = ctx(L, CFG[dname], CFG[sname])
        if shape == "two_workgroups_of_64":      # the persistent loop across frames, the most sub-tiles per map tile
            c.tune("block", 64)
            c.tune("grid_enc", 2)
        elif shape == "1024_threads":            # clamped to 32 * block threads (256 at 8) and to what the kernel is compiled for
            c.tune("block", 1024)
        shapes[shape] = c
    for (w, h) in ((264, 70), (34, 18)):
        src = random_planes(L, rng, w, h, sp, nf)
        ptrs = None
        if not vw4:
            shifted = [torch.cat([torch.full((2,), SENTINEL, dtype=torch.uint8, device=dev()), t]) for t in src.t]
            ptrs = [t.data_ptr() + 2 for t in shifted]
        enc, ebufs = transcoded(shapes["default"], L, src, src_sc, dp, dst_sc)
        given = from_frames(L, given_frames(rng, enc, ebufs, w, h, dp, 16), w, h, dp, padding="source")
        for block in MOM_BLOCKS:
            exp = expect_moments(enc, ebufs, given, given.host(), block)
            assert not own_planes_moments(exp)
            for shape, c in shapes.items():
                got = tmom(c, src, src_sc, given, dst_sc, block, src_ptrs=ptrs)
                assert np.array_equal(got, exp), (sname, dname, w, h, block, shape, vw4, got, exp)


# ---- 7. repeatability and section
@pytest.mark.parametrize("sname,dname", [("pq11_luv8", "pq10_ycbcr10"), ("pq11_luv8", "log12_luv8")])
def test_one_720p_frame_twice_and_in_an_unordered_section(L, sname, dname):
    import torch
    c = ctx(L, CFG[dname], CFG[sname])
    src_sc, dst_sc = scs_of(sname, dname)
    rng = np.random.default_rng(722)
    w, h, profile, block = 1280, 720, 2, 8
    src = random_planes(L, rng, w, h, profile, 1)
    enc, ebufs = transcoded(c, L, src, src_sc, profile, dst_sc)
    given = from_frames(L, [perturb(rng, enc.frame(ebufs, 0), w, h, profile, frac=0.5)], w, h, profile, padding="source")
    sbefore, gbefore = src.host(), given.host()
    exp = expect_moments(enc, ebufs, given, gbefore, block)
    a = tmom(c, src, src_sc, given, dst_sc, block)
    b = tmom(c, src, src_sc, given, dst_sc, block)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(b, exp)
    bufs = [map_buf(mom_nwords(1, w, h, block)) for _ in range(2)]
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for buf in bufs:
        c.transcode_moments_map_frames_device(src.ptrs, src.st, src.pfs, profile, src_sc, 1, w, h, given.ptrs, given.st, given.pfs,
                                              profile, dst_sc, block, buf.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for buf in bufs:
        assert np.array_equal(mom_words(buf, 1, w, h, block), exp)
    inputs_as_before(src, sbefore, given, gbefore, (sname, dname))


# ---- 8. errors: nothing is launched, the buffer is left as it was
def test_errors_launch_nothing(L):
    import torch
    from lumahdrv_amd.capi import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, LumaHipError
    w, h, profile, nf = 64, 32, 2, 1
    luv, rgb, deep = CFG["pq11_luv8"], (1, 11, 1, 8, 1e4, 0.005), CFG["pq14_luv8"]
    src, given = Planes(L, w, h, profile, nf), Planes(L, w, h, profile, nf)
    # 8 blocks of 16: 960 bytes of moments; the distortion map's 768 would end 32 bytes in front of a plane 800 bytes behind the buffer
    assert mom_nwords(nf, w, h, 16) * 8 == 960 and nwords(nf, w, h, 16) * 8 == 768

    def refused(c, code, w=w, block=16, mom_ptr="own"):
        buf = map_buf(mom_nwords(nf, 64, 32, 8))
        ptr = buf.data_ptr() if mom_ptr == "own" else mom_ptr(buf)
        with pytest.raises(LumaHipError) as ei:
            c.transcode_moments_map_frames_device(src.ptrs, src.st, src.pfs, profile, 1.0, nf, w, h, given.ptrs, given.st, given.pfs,
                                                  profile, 1.0, block, ptr)
        assert ei.value.code == code, ei.value
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == OUT_FILL), "an error return wrote to mom_dev"
        assert all(np.all(b == SENTINEL) for b in src.host() + given.host())

    good = ctx(L, luv, luv)
    for block in (0, 4, 48, 128):
        refused(good, ERR_ARG, block=block)                                         # bad block
    refused(ctx(L, luv), ERR_STATE)                                                # no source quantizer
    refused(good, ERR_ARG, w=63)                                                    # odd width
    refused(good, ERR_ARG, mom_ptr=lambda o: None)                                  # null mom_dev
    refused(good, ERR_ARG, mom_ptr=lambda o: o.data_ptr() + 4)                      # misaligned mom_dev
    refused(good, ERR_ARG, mom_ptr=lambda o: src.ptrs[0] + 64)                      # mom_dev inside a source plane
    refused(good, ERR_ARG, mom_ptr=lambda o: given.ptrs[2] + 8)                     # mom_dev inside a given plane
    # ... and one whose first 200 bytes lie in front of the plane: the map's own byte count decides (120 bytes per block)
    refused(good, ERR_ARG, mom_ptr=lambda o: given.ptrs[1] - 200)
    refused(good, ERR_ARG, mom_ptr=lambda o: src.ptrs[1] - 200)
    # ... and 800 bytes in front of it: 960 bytes of moments reach the plane, the distortion map's 768 would not
    refused(good, ERR_ARG, mom_ptr=lambda o: given.ptrs[1] - 800)
    refused(ctx(L, luv, rgb), ERR_UNSUPPORTED)                                     # an RGB source quantizer
    refused(ctx(L, deep, luv), ERR_UNSUPPORTED)                                    # a 14-bit target: records in global memory
    lit = ctx(L, luv, luv)
    lit.tune("force_literal", 1)
    refused(lit, ERR_UNSUPPORTED)                                                   # force_literal
    # the host form: mom_words one short, and a bad block
    sp, gp = src.frame(src.host(), 0), given.frame(given.host(), 0)
    need = mom_nwords(1, w, h, 8)
    m = np.full(need + GUARD, OUT_FILL, dtype=np.int64)

    def host_form(words, block=8):
        return good.L.lumahip_transcode_moments_map_frame_host(
            good.h, (C.c_void_p * 3)(*[p.ctypes.data for p in sp]), (C.c_int * 3)(*src.st), profile, 1.0, w, h,
            (C.c_void_p * 3)(*[p.ctypes.data for p in gp]), (C.c_int * 3)(*given.st), profile, 1.0, block, m.ctypes.data, words)

    assert host_form(need - 1) == ERR_ARG and np.all(m == OUT_FILL)
    assert host_form(need, block=4) == ERR_ARG and np.all(m == OUT_FILL)
    # ... and the same arguments are accepted by a context that can
    got = tmom(good, src, 1.0, given, 1.0, 8)
    assert got.shape == (1, 4, 8, 3, 5)
    assert host_form(need) == 0 and np.all(m[need:] == OUT_FILL)
    assert np.array_equal(m[:need].view(np.uint64).reshape(4, 8, 3, 5), got[0])
    assert tmom(good, src, 1.0, given, 1.0, 16).shape == (1, 2, 4, 3, 5)
    lit.tune("force_literal", 0)
    assert np.array_equal(tmom(lit, src, 1.0, given, 1.0, 8), got)
    assert good.transcode_moments_map_frame(sp, src.st, w, h, gp, given.st, block=8).shape == (4, 8, 3, 5)
    # ... and the distortion map's own rule stands: it still refuses blocks of 8
    with pytest.raises(LumaHipError) as ei:
        tmap(good, src, 1.0, given, 1.0, 8)
    assert ei.value.code == ERR_ARG
    assert tmap(good, src, 1.0, given, 1.0, 16).shape == (1, 2, 4, 3, 4)


# ---- 9. both quantizers are what they were
def test_the_quantizers_are_untouched(L):
    c = ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    rng = np.random.default_rng(9)
    w, h, nf = 64, 32, 3
    src = random_planes(L, rng, w, h, 2, nf)
    info = c.quantizer_info()
    _, before = transcoded(c, L, src, 1.0, 2, 20.0)
    given = random_planes(L, rng, w, h, 2, nf)
    dmap = tmap(c, src, 1.0, given, 20.0, 16)
    first = tmom(c, src, 1.0, given, 20.0, 8)
    c.tune("grid_enc", 2)
    c.tune("block", 64)
    assert np.array_equal(tmom(c, src, 1.0, given, 20.0, 8), first)
    c.tune("grid_enc", 0)
    c.tune("block", 0)
    tmom(c, src, 1.0, given, 20.0, 64)
    _, after = transcoded(c, L, src, 1.0, 2, 20.0)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(tmap(c, src, 1.0, given, 20.0, 16), dmap)
    assert c.quantizer_info() == info
