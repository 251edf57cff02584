"""Transcode distortion (include/lumahip.h lumahip_transcode_distortion_frames_device / _frame_host): twelve exact integers per
frame -- per plane {sum (e-g)^2, sum |e-g|, max |e-g|, #(e != g)} -- of given planes against the planes
lumahip_transcode_frames_device would write for the same source planes.  Every expectation is exact equality with numpy's integers
(tests/test_distortion_host.py expected_distortion).

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
from tests.test_distortion_host import expected_distortion
from tests.test_gpu_distortion import OUT_FILL, _out, _perturb, _words
from tests.test_gpu_transcode import CFG, PAIRS, SENTINEL, SIZES, Planes, _ctx, _dev, _from_frames, _fused
from tests.test_transcode_distortion_host import fixture_cases, perturbed

pytestmark = pytest.mark.gpu

SCS = (1.0, 20.0, 0.01)


@pytest.fixture(scope="module")
def L():
    import lumahdrv_amd
    return lumahdrv_amd


def _measure(c, src, src_sc, given, dst_sc, out=None):
    """the twelve words per frame of the device call"""
    import torch
    out = _out(src.nf) if out is None else out
    c.transcode_distortion_frames_device(src.ptrs, src.st, src.pfs, src.profile, src_sc, src.nf, src.w, src.h,
                                         given.ptrs, given.st, given.pfs, given.profile, dst_sc, out.data_ptr())
    torch.cuda.synchronize()
    return _words(out, src.nf)


def _transcoded(c, L, src, src_sc, dp, dst_sc, strides=None):
    """what lumahip_transcode_frames_device writes for src: its Planes and their host buffers"""
    import torch
    dst = Planes(L, src.w, src.h, dp, src.nf, strides=strides)
    _fused(c, src, src_sc, dst, dst_sc)
    torch.cuda.synchronize()
    return dst, dst.host()


def _expect(enc, ebufs, given, gbufs):
    return np.stack([expected_distortion(enc.frame(ebufs, f), given.frame(gbufs, f), enc.w, enc.h, enc.profile) for f in range(enc.nf)])


def _random_planes(L, rng, w, h, profile, nf, strides=None):
    """random bytes in the samples (out-of-range codes included), the sentinel in every row padding and gap"""
    pl = Planes(L, w, h, profile, nf, strides=strides)
    sub, bps = profile in (0, 2), 2 if profile > 1 else 1
    frames = []
    for _ in range(nf):
        fr = []
        for p in range(3):
            a = np.full((pl.hs[p], pl.st[p]), SENTINEL, dtype=np.uint8)
            rb = (w // 2 if (p and sub) else w) * bps
            a[:, :rb] = rng.integers(0, 256, size=(pl.hs[p], rb), dtype=np.uint8)
            fr.append(a)
        frames.append(fr)
    return _from_frames(L, frames, w, h, profile, strides=strides)


# ---- 1. the reference's own decode -> encode
def test_reference_fixture_and_its_perturbed_copy(L, golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    ctxs, n = {}, 0
    for k, case, w, h, sp in fixture_cases(gt):
        sname, src_sc, dname, dst_sc = mg.CASES[case]
        c = ctxs.setdefault(case, _ctx(L, mg.CONFIGS[dname], mg.CONFIGS[sname]))
        planes, st = mg.source_planes(gp, sname, w, h, sp)
        fix = [gt[k + "_plane%d" % p] for p in range(3)]
        est = tuple(int(s) for s in gt[k + "_stride"])
        bad = perturbed(fix, w, h, mg.DST_PROFILE)
        exp = expected_distortion(fix, bad, w, h, mg.DST_PROFILE)
        assert exp[:, 3].all(), k
        src = _from_frames(L, [planes], w, h, sp, strides=st)
        for given, want in ((fix, np.zeros((3, 4), dtype=np.uint64)), (bad, exp)):
            got = _measure(c, src, src_sc, _from_frames(L, [given], w, h, mg.DST_PROFILE, strides=est), dst_sc)
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
    c = _ctx(L, dcfg, scfg)
    if dname == "linear12_luv8":
        assert c.quantizer_info()["mode"] == 7, "the value-keyed records are what this pair is here for"
    rng = np.random.default_rng(len(sname) * 37 + len(dname))
    nf, it = 3, 0
    for sp in range(4):
        for dp in range(4):
            for (w, h) in SIZES:
                it += 1
                src_sc, dst_sc = (float(x) for x in rng.choice(SCS, 2))
                src = _random_planes(L, rng, w, h, sp, nf)
                enc, ebufs = _transcoded(c, L, src, src_sc, dp, dst_sc)
                if it % 2:
                    given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)], w, h, dp)
                else:
                    given = _random_planes(L, rng, w, h, dp, nf)
                sbefore, gbefore = src.host(), given.host()
                exp = _expect(enc, ebufs, given, gbefore)
                got = _measure(c, src, src_sc, given, dst_sc)
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
    c = _ctx(L, CFG[dname], CFG[sname])
    rng = np.random.default_rng(33)
    nf = 3
    src_sc, dst_sc = (20.0, 1.0) if CFG[sname][2] == 2 else (1.0, 20.0)
    for (w, h) in ((64, 32), (34, 18)):
        for sp, dp in ((2, 2), (3, 1), (0, 3)):
            src = _random_planes(L, rng, w, h, sp, nf)
            enc, ebufs = _transcoded(c, L, src, src_sc, dp, dst_sc)
            want = None
            for odd in (False, True):
                st = tuple(s + 1 for s in enc.st) if odd else None
                frames = [_perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)]
                if odd:   # the same samples in rows one byte longer
                    frames = [[np.concatenate([a, np.full((a.shape[0], 1), SENTINEL, np.uint8)], axis=1) for a in fr] for fr in frames]
                given = _from_frames(L, frames, w, h, dp, strides=st)
                gb = given.host()
                exp = _expect(enc, ebufs, given, gb)
                got = _measure(c, src, src_sc, given, dst_sc)
                assert np.array_equal(got, exp), (sname, dname, w, h, sp, dp, odd, got, exp)
                assert given.gaps_intact(given.host())
            # the source planes one byte into their buffers: same integers as from the aligned ones
            given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, dp) for f in range(nf)], w, h, dp)
            want = _measure(c, src, src_sc, given, dst_sc)
            shifted = [torch.cat([torch.full((1,), SENTINEL, dtype=torch.uint8, device=_dev()), t]) for t in src.t]
            out = _out(nf)
            c.transcode_distortion_frames_device([t.data_ptr() + 1 for t in shifted], src.st, src.pfs, sp, src_sc, nf, w, h,
                                                 given.ptrs, given.st, given.pfs, dp, dst_sc, out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(_words(out, nf), want), (sname, dname, w, h, sp, dp, "misaligned source")
            assert np.array_equal(want, _expect(enc, ebufs, given, given.host()))


# ---- 4. accumulator width: one wave carries more than 2^32 of squared difference per plane
def test_one_wave_accumulates_beyond_32_bits(L):
    c = _ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    c.tune("grid_enc", 1)
    c.tune("block", 64)
    rng = np.random.default_rng(3)
    w, h, nf = 64, 32, 3
    for dp in (2, 3):
        src = _random_planes(L, rng, w, h, 2, nf)
        enc, ebufs = _transcoded(c, L, src, 1.0, dp, 20.0)
        ones = Planes(L, w, h, dp, nf, fill=[np.full(nf * enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
        exp = _expect(enc, ebufs, ones, ones.host())
        assert np.all(exp[:, :, 0] > np.uint64(1) << np.uint64(32))
        got = _measure(c, src, 1.0, ones, 20.0)
        assert np.array_equal(got, exp), (dp, got, exp)


# ---- 5. persistent loop and frame change
@pytest.mark.parametrize("size", [(6, 4), (258, 6), (64, 32)])
def test_two_workgroups_book_every_frame_to_itself(L, size):
    w, h = size
    rng = np.random.default_rng(w)
    nf = 3
    for sname, dname, sp, dp in (("pq11_luv8", "pq10_ycbcr10", 2, 2), ("pq10_ycbcr10", "pq11_luv8", 3, 0), ("pq11_luv8", "log12_luv8", 1, 3)):
        c = _ctx(L, CFG[dname], CFG[sname])
        src_sc, dst_sc = (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)
        src = _random_planes(L, rng, w, h, sp, nf)
        enc, ebufs = _transcoded(c, L, src, src_sc, dp, dst_sc)
        # frame f: its own share of perturbed samples and its own amplitude
        given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, dp, frac=0.2 + 0.3 * f, amp=1 + 3 * f, extremes=f)
                                 for f in range(nf)], w, h, dp)
        exp = _expect(enc, ebufs, given, given.host())
        assert len({tuple(e.ravel()) for e in exp}) == nf
        c.tune("grid_enc", 2)
        c.tune("block", 64)
        got = _measure(c, src, src_sc, given, dst_sc)
        assert np.array_equal(got, exp), (sname, dname, size, got, exp)


# ---- 6. other shapes and sections
@pytest.mark.parametrize("sname,dname", [("pq11_luv8", "pq10_ycbcr10"), ("pq10_ycbcr10", "log12_luv8")])
def test_one_720p_frame_twice(L, sname, dname):
    c = _ctx(L, CFG[dname], CFG[sname])
    src_sc, dst_sc = (20.0 if CFG[sname][2] == 2 else 1.0), (20.0 if CFG[dname][2] == 2 else 1.0)
    rng = np.random.default_rng(720)
    w, h = 1280, 720
    src = _random_planes(L, rng, w, h, 2, 1)
    enc, ebufs = _transcoded(c, L, src, src_sc, 2, dst_sc)
    given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, 0), w, h, 2)], w, h, 2)
    exp = _expect(enc, ebufs, given, given.host())
    a = _measure(c, src, src_sc, given, dst_sc)
    b = _measure(c, src, src_sc, given, dst_sc)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(a, b)


def test_unordered_section_two_batches_on_two_lanes(L):
    import torch
    c = _ctx(L, CFG["log12_luv8"], CFG["pq10_ycbcr10"])
    rng = np.random.default_rng(5)
    w, h, nf = 258, 6, 3
    batches = []
    for _ in range(2):
        src = _random_planes(L, rng, w, h, 2, nf)
        enc, ebufs = _transcoded(c, L, src, 20.0, 2, 1.0)
        given = _from_frames(L, [_perturb(rng, enc.frame(ebufs, f), w, h, 2) for f in range(nf)], w, h, 2)
        batches.append((src, given, _expect(enc, ebufs, given, given.host()), _out(nf)))
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for src, given, _, out in batches:
        c.transcode_distortion_frames_device(src.ptrs, src.st, src.pfs, 2, 20.0, nf, w, h, given.ptrs, given.st, given.pfs, 2, 1.0, out.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for _, _, exp, out in batches:
        assert np.array_equal(_words(out, nf), exp)


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
        out = _out(2)
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
        got = _measure(c, src, 1.0, given, 1.0)
        assert got.shape == (1, 3, 4)
        return got

    c = _ctx(L, luv)
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
    attempt(_ctx(L, rgb, luv), ERR_UNSUPPORTED)
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
        _ctx(L, luv).transcode_distortion_frame(pl, (128, 64, 64), w, h, pl, (128, 64, 64))
    assert e.value.code == ERR_STATE


# ---- 8. both quantizers are what they were
def test_the_quantizers_are_untouched(L):
    c = _ctx(L, CFG["pq10_ycbcr10"], CFG["pq11_luv8"])
    rng = np.random.default_rng(8)
    w, h, nf = 64, 32, 3
    src = _random_planes(L, rng, w, h, 2, nf)
    info = c.quantizer_info()
    _, before = _transcoded(c, L, src, 1.0, 2, 20.0)
    given = _random_planes(L, rng, w, h, 2, nf)
    _measure(c, src, 1.0, given, 20.0)
    c.tune("grid_enc", 2)
    c.tune("block", 64)
    _measure(c, src, 1.0, given, 20.0)
    c.tune("grid_enc", 0)
    c.tune("block", 0)
    _, after = _transcoded(c, L, src, 1.0, 2, 20.0)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert c.quantizer_info() == info
