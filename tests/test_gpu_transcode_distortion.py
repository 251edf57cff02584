"""Transcode distortion (include/lumahip.h lumahip_transcode_distortion_frames_device / _frame_host): twelve exact integers per
frame -- per plane {sum (e-g)^2, sum |e-g|, max |e-g|, #(e != g)} -- of given planes against the planes
lumahip_transcode_frames_device would write for the same source planes.  Every expectation is exact equality with numpy's integers
(tests/support/host.py expected_distortion).

1. The reference's own decode -> encode (tests/golden/ref_transcode.npz): zeros against the fixture, numpy's integers against a
   perturbed copy; device call and host call.
2. Against lumahip_transcode_frames_device into scratch planes + numpy: nine configuration pairs, all 16 profile pairs, sizes
   (34,18) (258,6) (64,32) (6,4) x 3 frames, preScalings from {1, 20, 0.01}; given = the perturbed result or random bytes; sentinel
   bytes in every padding and gap; both plane sets unchanged; out_dev pre-filled.
3. Odd given strides and misaligned source planes.  4. One wave beyond 2^32.  5. Two workgroups, three frames.
6. 1280x720, an unordered section, two runs.  7. Errors.  8. Both quantizers untouched.
"""
import os

import numpy as np
import pytest

from tests.golden import make_transcode_golden as mg
from tests.support.device import (L, Planes, ctx, dev, from_frames, measure, out_buf, out_words, random_planes,  # noqa: F401  (L is the module fixture)
                                  transcoded)
from tests.support.host import CFG, OUT_FILL, PAIRS, SENTINEL, SIZES, expect, expected_distortion, fixture_cases, perturb, perturbed

pytestmark = pytest.mark.gpu

SCS = (1.0, 20.0, 0.01)


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
        exp = expected_distortion(fix, bad, w, h, mg.DST_PROFILE)
        assert exp[:, 3].all(), k
        src = from_frames(L, [planes], w, h, sp, strides=st, padding="source")
        for given, want in ((fix, np.zeros((3, 4), dtype=np.uint64)), (bad, exp)):
            got = measure(c, src, src_sc, from_frames(L, [given], w, h, mg.DST_PROFILE, strides=est, padding="source"), dst_sc)
            assert np.array_equal(got[0], want), (k, "device", got, want)
            hw = c.transcode_distortion_frame(planes, st, w, h, given, est, src_sc, sp, dst_sc, mg.DST_PROFILE)
            assert hw.dtype == np.uint64 and hw.shape == (3, 4)
            assert np.array_equal(hw, want), (k, "host", hw, want)
        n += 1
    assert n == 16


# ---- 2. against lumahip_transcode_frames_device into scratch planes
@pytest.mark.parametrize("sname,dname", PAIRS)
def test_equals_numpy_on_the_transcode_calls_planes(L, sname, dname):
    scfg, dcfg = CFG[sname], CFG[dname]
    c = ctx(L, dcfg, scfg)
    if dname == "linear12_luv8":
        assert c.quantizer_info()["mode"] == 7, "the value-keyed records are what this pair is here for"
    rng = np.random.default_rng(len(sname) * 37 + len(dname))
    nf, it = 3, 0
    for sp in range(4):
        for dp in range(4):
            for (w, h) in SIZES:
                it += 1
                src_sc, dst_sc = (float(x) for x in rng.choice(SCS, 2))
                src = random_planes(L, rng, w, h, sp, nf)
                enc, ebufs = transcoded(c, L, src, src_sc, dp, dst_sc)
                if it % 2:
                    given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)], w, h, dp, padding="source")
                else:
                    given = random_planes(L, rng, w, h, dp, nf)
                sbefore, gbefore = src.host(), given.host()
                exp = expect(enc, ebufs, given, gbefore)
                got = measure(c, src, src_sc, given, dst_sc)
                tag = (sname, dname, sp, dp, w, h, src_sc, dst_sc, it % 2)
                assert np.array_equal(got, exp), tag + (got, exp)
                assert exp[:, :, 3].any(), tag
                for a, b in zip(sbefore + gbefore, src.host() + given.host()):
                    assert np.array_equal(a, b), tag + ("an input plane changed",)
                assert src.gaps_intact(sbefore) and given.gaps_intact(gbefore), tag
    assert it == 64


# ---- 3. odd given strides (byte loads), misaligned source planes
@pytest.mark.parametrize("sname,dname", [("pq11_luv8", "pq10_ycbcr10"), ("pq10_ycbcr10", "log12_luv8")])
def test_odd_given_strides_and_misaligned_source_planes(L, sname, dname):
    import torch
    c = ctx(L, CFG[dname], CFG[sname])
    rng = np.random.default_rng(33)
    nf = 3
    src_sc, dst_sc = (20.0, 1.0) if CFG[sname][2] == 2 else (1.0, 20.0)
    for (w, h) in ((64, 32), (34, 18)):
        for sp, dp in ((2, 2), (3, 1), (0, 3)):
            src = random_planes(L, rng, w, h, sp, nf)
            enc, ebufs = transcoded(c, L, src, src_sc, dp, dst_sc)
            want = None
            for odd in (False, True):
                st = tuple(s + 1 for s in enc.st) if odd else None
                frames = [perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)]
                if odd:   # the same samples in rows one byte longer
                    frames = [[np.concatenate([a, np.full((a.shape[0], 1), SENTINEL, np.uint8)], axis=1) for a in fr] for fr in frames]
                given = from_frames(L, frames, w, h, dp, strides=st, padding="source")
                gb = given.host()
                exp = expect(enc, ebufs, given, gb)
                got = measure(c, src, src_sc, given, dst_sc)
                assert np.array_equal(got, exp), (sname, dname, w, h, sp, dp, odd, got, exp)
                assert given.gaps_intact(given.host())
            # the source planes one byte into their buffers: same integers as from the aligned ones
            given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)], w, h, dp, padding="source")
            want = measure(c, src, src_sc, given, dst_sc)
            shifted = [torch.cat([torch.full((1,), SENTINEL, dtype=torch.uint8, device=dev()), t]) for t in src.t]
            out = out_buf(nf)
            c.transcode_distortion_frames_device([t.data_ptr() + 1 for t in shifted], src.st, src.pfs, sp, src_sc, nf, w, h,
                                                 given.ptrs, given.st, given.pfs, dp, dst_sc, out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out_words(out, nf), want), (sname, dname, w, h, sp, dp, "misaligned source")
            assert np.array_equal(want, expect(enc, ebufs, given, given.host()))


# ---- 4. accumulator width: one wave carries more than 2^32 of squared difference per plane
def test_one_wave_accumulates_beyond_32_bits(L):
    c = ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    c.tune("grid_enc", 1)
    c.tune("block", 64)
    rng = np.random.default_rng(3)
    w, h, nf = 64, 32, 3
    for dp in (2, 3):
        src = random_planes(L, rng, w, h, 2, nf)
        enc, ebufs = transcoded(c, L, src, 1.0, dp, 20.0)
        ones = Planes(L, w, h, dp, nf, fill=[np.full(nf * enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
        exp = expect(enc, ebufs, ones, ones.host())
        assert np.all(exp[:, :, 0] > np.uint64(1) << np.uint64(32))
        got = measure(c, src, 1.0, ones, 20.0)
        assert np.array_equal(got, exp), (dp, got, exp)


# ---- 5. persistent loop and frame change
@pytest.mark.parametrize("size", [(6, 4), (258, 6), (64, 32)])
def test_two_workgroups_book_every_frame_to_itself(L, size):
    w, h = size
    rng = np.random.default_rng(w)
    nf = 3
    for sname, dname, sp, dp in (("pq11_luv8", "pq10_ycbcr10", 2, 2), ("pq10_ycbcr10", "pq11_luv8", 3, 0), ("pq11_luv8", "log12_luv8", 1, 3)):
        c = ctx(L, CFG[dname], CFG[sname])
        src_sc, dst_sc = (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)
        src = random_planes(L, rng, w, h, sp, nf)
        enc, ebufs = transcoded(c, L, src, src_sc, dp, dst_sc)
        # frame f: its own share of perturbed samples and its own amplitude
        given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, dp, frac=0.2 + 0.3 * f, amp=1 + 3 * f, extremes=f)
                                for f in range(nf)], w, h, dp, padding="source")
        exp = expect(enc, ebufs, given, given.host())
        assert len({tuple(e.ravel()) for e in exp}) == nf
        c.tune("grid_enc", 2)
        c.tune("block", 64)
        got = measure(c, src, src_sc, given, dst_sc)
        assert np.array_equal(got, exp), (sname, dname, size, got, exp)


# ---- 6. other shapes and sections
@pytest.mark.parametrize("sname,dname", [("pq11_luv8", "pq10_ycbcr10"), ("pq10_ycbcr10", "log12_luv8")])
def test_one_720p_frame_twice(L, sname, dname):
    c = ctx(L, CFG[dname], CFG[sname])
    src_sc, dst_sc = (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)
    rng = np.random.default_rng(720)
    w, h = 1280, 720
    src = random_planes(L, rng, w, h, 2, 1)
    enc, ebufs = transcoded(c, L, src, src_sc, 2, dst_sc)
    given = from_frames(L, [perturb(rng, enc.frame(ebufs, 0), w, h, 2)], w, h, 2, padding="source")
    exp = expect(enc, ebufs, given, given.host())
    a = measure(c, src, src_sc, given, dst_sc)
    b = measure(c, src, src_sc, given, dst_sc)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(a, b)


def test_unordered_section_two_batches_on_two_lanes(L):
    import torch
    c = ctx(L, CFG["log12_luv8"], CFG["pq10_ycbcr10"])
    rng = np.random.default_rng(5)
    w, h, nf = 258, 6, 3
    batches = []
    for _ in range(2):
        src = random_planes(L, rng, w, h, 2, nf)
        enc, ebufs = transcoded(c, L, src, 20.0, 2, 1.0)
        given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, 2) for f in range(nf)], w, h, 2, padding="source")
        batches.append((src, given, expect(enc, ebufs, given, given.host()), out_buf(nf)))
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for src, given, _, out in batches:
        c.transcode_distortion_frames_device(src.ptrs, src.st, src.pfs, 2, 20.0, nf, w, h, given.ptrs, given.st, given.pfs, 2, 1.0, out.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for _, _, exp, out in batches:
        assert np.array_equal(out_words(out, nf), exp)


# ---- 7. errors
def test_errors_launch_nothing(L):
    import torch
    from lumahdrv_amd.capi import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, LumaHipError
    w, h = 64, 32
    luv = CFG["pq11_luv8"]

    def lut(cfg):
        return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])

    def attempt(c, code, w=w, h=h, out_ptr=None, src=None, given=None):
        src = src or Planes(L, w & ~1, h & ~1, 2, 1)
        given = given or Planes(L, w & ~1, h & ~1, 2, 1)
        out = out_buf(2)
        with pytest.raises(LumaHipError) as e:
            c.transcode_distortion_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 1, w, h, given.ptrs, given.st, given.pfs, 2, 1.0,
                                                 out.data_ptr() if out_ptr is None else out_ptr(out))
        assert e.value.code == code, str(e.value)
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == OUT_FILL), "an error return wrote to out_dev"
        assert np.all(src.host()[0] == SENTINEL) and np.all(given.host()[0] == SENTINEL)

    def works(c, src=None, given=None):
        src = src or Planes(L, w, h, 2, 1)
        given = given or src
        got = measure(c, src, 1.0, given, 1.0)
        assert got.shape == (1, 3, 4)
        return got

    c = ctx(L, luv)
    attempt(c, ERR_STATE)                                    # no source quantizer
    c.set_source_quantizer(*luv, lut(luv))
    src = Planes(L, w, h, 2, 1)
    works(c, src, src)                                       # source planes identical to given planes: accepted
    attempt(c, ERR_ARG, w=63)                                # odd sizes
    attempt(c, ERR_ARG, h=31)
    attempt(c, ERR_ARG, out_ptr=lambda o: None)              # null, misaligned, overlapping out_dev
    attempt(c, ERR_ARG, out_ptr=lambda o: o.data_ptr() + 4)
    attempt(c, ERR_ARG, src=src, out_ptr=lambda o: src.ptrs[0] + 8)
    attempt(c, ERR_ARG, given=src, out_ptr=lambda o: src.ptrs[2] + src.size[2] - 8)
    works(c)
    rgb = (1, 11, 1, 8, 1e4, 0.005)                          # RGB target
    attempt(ctx(L, rgb, luv), ERR_UNSUPPORTED)
    deep = (1, 13, 0, 8, 1e4, 0.005)                         # a 13-bit source
    c.set_source_quantizer(*deep, lut(deep))
    attempt(c, ERR_UNSUPPORTED)
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    c.tune("force_literal", 1)                               # literal-bisection target
    attempt(c, ERR_UNSUPPORTED)
    c.tune("force_literal", 0)
    works(c)
    with pytest.raises(LumaHipError) as e:                   # the host call refuses the same way
        pl = [np.zeros((32, 128), np.uint8), np.zeros((16, 64), np.uint8), np.zeros((16, 64), np.uint8)]
        ctx(L, luv).transcode_distortion_frame(pl, (128, 64, 64), w, h, pl, (128, 64, 64))
    assert e.value.code == ERR_STATE


# ---- 8. both quantizers are what they were
def test_the_quantizers_are_untouched(L):
    c = ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    rng = np.random.default_rng(8)
    w, h, nf = 64, 32, 3
    src = random_planes(L, rng, w, h, 2, nf)
    info = c.quantizer_info()
    _, before = transcoded(c, L, src, 1.0, 2, 20.0)
    given = random_planes(L, rng, w, h, 2, nf)
    measure(c, src, 1.0, given, 20.0)
    c.tune("grid_enc", 2)
    c.tune("block", 64)
    measure(c, src, 1.0, given, 20.0)
    c.tune("grid_enc", 0)
    c.tune("block", 0)
    _, after = transcoded(c, L, src, 1.0, 2, 20.0)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert c.quantizer_info() == info
