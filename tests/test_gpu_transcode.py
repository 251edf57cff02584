"""Fused transcode (include/lumahip.h lumahip_transcode_frames_device / lumahip_transcode_frame_host): code planes under the
source quantizer -> code planes under the context's quantizer in one launch.

1. Against the reference's own decode -> encode (tests/golden/ref_transcode.npz), device call and host call, bit for bit.
2. Against the oracle's decode -> encode and against lumahip_decode_frames_device + lumahip_encode_frames_device through a float
   buffer: nine configuration pairs (the four colour-space pairs; record and value-keyed targets), all 16 profile pairs, sizes
   (34,18) (258,6) (64,32) (6,4) x 3 frames, random bytes and real planes, preScalings from {1, 20, 0.01, 3e5} (0 and NaN against
   the two-call pair only), frame strides with a gap that must survive, statistics, the host call's mean luminance.
3. Persistent loop and prefetch tail (2 workgroups of 64 threads).  4. Unordered section.  5. One 1280x720 frame (VW = 4,
   many tiles).  6. Errors, none of which launches anything.  7. The quantizer of lumahip_set_quantizer is untouched.
"""
import hashlib
import os

import numpy as np
import pytest

from tests.golden import make_transcode_golden as mg
from tests.support.device import L, Planes, ctx, dev, from_frames, fused, table_for, two_calls  # noqa: F401  (L is the module fixture)
from tests.support.host import CFG, PAIRS, SENTINEL, SIZES, same_rows

pytestmark = pytest.mark.gpu


# ---- 1. the reference's own decode -> encode
def test_fused_equals_the_reference_fixture(L, golden_dir):
    import torch
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    gt = np.load(os.path.join(golden_dir, "ref_transcode.npz"))
    n = 0
    for case, (sname, src_sc, dname, dst_sc) in sorted(mg.CASES.items()):
        c = ctx(L, mg.CONFIGS[dname], mg.CONFIGS[sname])
        for (w, h) in mg.SIZES:
            for sp in mg.SRC_PROFILES:
                k = mg.key_of(case, w, h, sp)
                planes, st = mg.source_planes(gp, sname, w, h, sp)
                exp = [gt[k + "_plane%d" % p] for p in range(3)]
                est = tuple(int(s) for s in gt[k + "_stride"])
                src = from_frames(L, [planes], w, h, sp, strides=st, padding="source")
                dst = Planes(L, w, h, mg.DST_PROFILE, 1, strides=est)
                fused(c, src, src_sc, dst, dst_sc)
                torch.cuda.synchronize()
                bufs = dst.host()
                assert same_rows(dst.frame(bufs, 0), exp, w, h, mg.DST_PROFILE), (k, "device")
                assert dst.gaps_intact(bufs), k
                hp, hst, _ = c.transcode_frame(planes, st, w, h, src_sc, sp, dst_sc, mg.DST_PROFILE, dst_strides=est)
                assert same_rows(hp, exp, w, h, mg.DST_PROFILE), (k, "host")
                n += 1
    assert n == 16


# ---- 2. oracle and two-call pair
SCS = (1.0, 20.0, 0.01, 3e5)


def _real_planes(o, cfg, w, h, profile, nf, sc):
    orc = o.Oracle(*cfg, table=table_for(o, cfg))
    return [orc.encode(o.synth_frame(w, h, frame=3 + i), sc, profile)[0] for i in range(nf)]


@pytest.mark.parametrize("sname,dname", PAIRS)
def test_fused_equals_oracle_and_the_two_call_pair(L, oracle_mod, sname, dname):
    import torch
    o = oracle_mod
    scfg, dcfg = CFG[sname], CFG[dname]
    ct, cd = ctx(L, dcfg, scfg), ctx(L, scfg)
    if dname == "linear12_luv8":
        assert ct.quantizer_info()["mode"] == 7, "the value-keyed records are what this pair is here for"
    odec, oenc = o.Oracle(*scfg, table=table_for(o, scfg)), o.Oracle(*dcfg, table=table_for(o, dcfg))
    rng = np.random.default_rng(len(sname) * 31 + len(dname))
    nf, it = 3, 0
    for sp in range(4):
        for dp in range(4):
            for (w, h) in SIZES:
                it += 1
                real = it % 3 == 0
                src_sc, dst_sc = (float(x) for x in rng.choice(SCS, 2))
                special = None
                if it % 7 == 0:   # x / 0 and NaN inputs to the target side: against the two-call pair only
                    src_sc = special = (0.0, float("nan"))[(it // 7) % 2]
                if real:
                    src = from_frames(L, _real_planes(o, scfg, w, h, sp, nf, src_sc if special is None else 1.0), w, h, sp, padding="source")
                else:
                    src = Planes(L, w, h, sp, nf)
                    fill = [rng.integers(0, 256, size=nf * src.pfs[p], dtype=np.uint8) for p in range(3)]   # out-of-range codes included
                    src = Planes(L, w, h, sp, nf, fill=fill)
                dst, ref = Planes(L, w, h, dp, nf), Planes(L, w, h, dp, nf)
                with_stats = it % 2 == 0
                s1 = torch.zeros(3 * nf, dtype=torch.float32, device=dev()) if with_stats else None
                s2 = torch.zeros(3 * nf, dtype=torch.float32, device=dev()) if with_stats else None
                fused(ct, src, src_sc, dst, dst_sc, s1)
                buf = two_calls(cd, ct, src, src_sc, ref, dst_sc, s2)
                torch.cuda.synchronize()
                tag = (sname, dname, sp, dp, w, h, src_sc, dst_sc, real)
                got, exp = dst.host(), ref.host()
                for p in range(3):
                    assert np.array_equal(got[p], exp[p]), tag + ("two-call pair, plane %d" % p,)
                assert dst.gaps_intact(got), tag
                if with_stats:
                    a, b = s1.cpu().numpy().reshape(nf, 3), s2.cpu().numpy().reshape(nf, 3)
                    assert np.array_equal(a[:, 1:], b[:, 1:], equal_nan=True), tag + ("min / max",)
                    assert np.allclose(a[:, 0], b[:, 0], rtol=1e-4, atol=0, equal_nan=True), tag + ("sum",)
                sh = src.host()
                if special is None:
                    for f in range(nf):
                        dec = odec.decode(src.frame(sh, f), src.st, w, h, src_sc, sp)
                        ep, est, _ = oenc.encode(dec, dst_sc, dp)
                        assert tuple(est) == tuple(dst.st)
                        assert same_rows(dst.frame(got, f), ep, w, h, dp), tag + ("oracle, frame %d" % f,)
                # the host call on frame 0: planes, and the mean luminance lumahip_encode_frame_host reports for the decoded frame
                hp, _, mean = ct.transcode_frame(src.frame(sh, 0), src.st, w, h, src_sc, sp, dst_sc, dp)
                assert same_rows(hp, dst.frame(got, 0), w, h, dp), tag + ("host call",)
                dec0 = buf[:3 * w * h].cpu().numpy().reshape(3, h, w)
                _, _, emean = ct.encode_frame(dec0, dst_sc, dp)
                assert (np.isnan(mean) and np.isnan(emean)) or mean == pytest.approx(emean, rel=1e-4), tag + ("mean luminance", mean, emean)
    assert it == 64


def test_host_mean_takes_the_reference_sum_where_the_encode_call_does(L, oracle_mod):
    """a frame whose mean luminance lies in [0.25, 4]: both calls answer with the reference's sequential sum, which is exact"""
    o = oracle_mod
    scfg, dcfg = CFG["pq10_ycbcr10"], CFG["pq11_luv8"]
    ct, cd = ctx(L, dcfg, scfg), ctx(L, scfg)
    w, h = 64, 32
    planes, st, _ = o.Oracle(*scfg).encode(o.synth_frame(w, h, frame=9), 20.0, 2)
    dec = cd.decode_frame(planes, st, w, h, 20.0, 2)
    _, _, m1 = ct.encode_frame(dec, 1.0, 2)
    sc = 1.0 / m1   # (luminance is linear in the frame: the mean lands near 1)
    _, _, em = ct.encode_frame(dec, sc, 2)
    assert 0.25 <= em <= 4.0
    _, _, tm = ct.transcode_frame(planes, st, w, h, 20.0, 2, sc, 2)
    assert tm == em


# ---- 3. few workgroups: every workgroup walks many tiles, the last prefetch runs off the end
@pytest.mark.parametrize("w,h", [(258, 6), (64, 32)])
def test_persistent_loop_and_prefetch_tail(L, w, h):
    import torch
    scfg, dcfg = CFG["pq11_luv8"], CFG["pq10_ycbcr10"]
    ct = ctx(L, dcfg, scfg)
    rng = np.random.default_rng(w)
    for sp, dp in ((2, 2), (3, 0), (1, 3)):
        src = Planes(L, w, h, sp, 3)
        src = Planes(L, w, h, sp, 3, fill=[rng.integers(0, 256, size=3 * src.pfs[p], dtype=np.uint8) for p in range(3)])
        a, b = Planes(L, w, h, dp, 3), Planes(L, w, h, dp, 3)
        fused(ct, src, 1.0, a, 20.0)
        ct.tune("grid_enc", 2)
        ct.tune("block", 64)
        fused(ct, src, 1.0, b, 20.0)
        ct.tune("grid_enc", 0)
        ct.tune("block", 0)
        torch.cuda.synchronize()
        for x, y in zip(a.host(), b.host()):
            assert np.array_equal(x, y), (w, h, sp, dp)


# ---- 4. unordered section
def test_unordered_section_gives_the_ordered_planes(L):
    import torch
    scfg, dcfg = CFG["pq10_ycbcr10"], CFG["log12_luv8"]
    ct = ctx(L, dcfg, scfg)
    rng = np.random.default_rng(4)
    w, h, nf = 64, 32, 3
    srcs, ordered, lanes = [], [], []
    for i in range(4):
        s = Planes(L, w, h, 2, nf)
        srcs.append(Planes(L, w, h, 2, nf, fill=[rng.integers(0, 256, size=nf * s.pfs[p], dtype=np.uint8) for p in range(3)]))
        ordered.append(Planes(L, w, h, 2, nf))
        lanes.append(Planes(L, w, h, 2, nf))
        fused(ct, srcs[i], 20.0, ordered[i], 1.0)
    ct.begin_unordered(2)
    for i in range(4):
        fused(ct, srcs[i], 20.0, lanes[i], 1.0)
    ct.end_unordered()
    ct.sync()
    torch.cuda.synchronize()
    for i in range(4):
        for x, y in zip(ordered[i].host(), lanes[i].host()):
            assert np.array_equal(x, y), i


# ---- 5. one 1280x720 frame: many tiles, four pixels per thread and row
def test_720p_frame_against_the_oracle(L, oracle_mod):
    import torch
    o = oracle_mod
    scfg, dcfg = CFG["pq11_luv8"], CFG["pq10_ycbcr10"]
    w, h = 1280, 720
    planes, st, _ = o.Oracle(*scfg).encode(o.test_frame(w, h), 1.0, 2)
    dec = o.Oracle(*scfg).decode(planes, st, w, h, 1.0, 2)
    exp, est, _ = o.Oracle(*dcfg).encode(dec, 20.0, 2)
    ct = ctx(L, dcfg, scfg)
    src = from_frames(L, [planes], w, h, 2, strides=st, padding="source")
    dst = Planes(L, w, h, 2, 1, strides=est)
    fused(ct, src, 1.0, dst, 20.0)
    torch.cuda.synchronize()
    bufs = dst.host()
    assert same_rows(dst.frame(bufs, 0), exp, w, h, 2)
    assert dst.gaps_intact(bufs)


# ---- 6. errors
def test_errors_launch_nothing_and_leave_the_context_usable(L):
    import torch
    from lumahdrv_amd.capi import ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, LumaHipError
    w, h = 64, 32
    luv, ycc = CFG["pq11_luv8"], CFG["pq10_ycbcr10"]

    def lut(cfg):
        return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])

    def attempt(c, code, w=w, h=h, dst=None, src=None):
        src = src or Planes(L, w & ~1, h & ~1, 2, 1)
        dst = dst or Planes(L, w & ~1, h & ~1, 2, 1)
        with pytest.raises(LumaHipError) as e:
            c.transcode_frames_device(src.ptrs, src.st, src.pfs, 2, 1.0, 1, w, h, dst.ptrs, dst.st, dst.pfs, 2, 1.0)
        assert e.value.code == code, str(e.value)
        assert c.L.lumahip_last_error(c.h).decode() != ""
        torch.cuda.synchronize()
        assert np.all(dst.host()[0] == SENTINEL), "an error return wrote to the destination"

    def works(c):
        src, dst = Planes(L, w, h, 2, 1), Planes(L, w, h, 2, 1)
        fused(c, src, 1.0, dst, 1.0)
        torch.cuda.synchronize()
        assert not np.all(dst.host()[0] == SENTINEL)

    c = ctx(L, luv)
    attempt(c, ERR_STATE)                                    # no source quantizer
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    attempt(c, ERR_ARG, w=63)                                # odd sizes
    attempt(c, ERR_ARG, h=31)
    works(c)
    src = Planes(L, w, h, 2, 1)
    attempt(c, ERR_ARG, src=src, dst=src)                    # overlapping extents
    works(c)
    for cs in (1, 3):                                        # RGB / XYZ on either side
        bad = (1, 11, cs, 8, 1e4, 0.005)
        c.set_source_quantizer(*bad, lut(bad))
        attempt(c, ERR_UNSUPPORTED)
        c.set_source_quantizer(*luv, lut(luv))
        works(c)
        c2 = ctx(L, bad, luv)
        attempt(c2, ERR_UNSUPPORTED)
    deep = (1, 14, 0, 8, 1e4, 0.005)                         # source bit depth 14
    c.set_source_quantizer(*deep, lut(deep))
    attempt(c, ERR_UNSUPPORTED)
    c.set_source_quantizer(*luv, lut(luv))
    works(c)
    c.tune("force_literal", 1)                               # literal-bisection target
    attempt(c, ERR_UNSUPPORTED)
    c.tune("force_literal", 0)
    works(c)
    big, y12 = (1, 13, 0, 8, 1e4, 0.005), (1, 12, 2, 12, 1000.0, 0.01)   # 136 KiB of records + a 12-bit YCbCr source: beyond 160 KiB
    c3 = ctx(L, big, y12)
    attempt(c3, ERR_UNSUPPORTED)
    c3.set_source_quantizer(*luv, lut(luv))                  # ... while PQ-11 Lu'v' beside the 13-bit target fits
    works(c3)
    with pytest.raises(LumaHipError) as e:                   # the host call refuses the same way
        ctx(L, luv).transcode_frame([np.zeros((32, 128), np.uint8), np.zeros((16, 64), np.uint8), np.zeros((16, 64), np.uint8)], (128, 64, 64), w, h)
    assert e.value.code == ERR_STATE


# ---- 7. the quantizer of lumahip_set_quantizer does not notice the source quantizer
def test_set_source_quantizer_leaves_encode_and_decode_alone(L, oracle_mod):
    o = oracle_mod
    cfg = CFG["pq11_luv8"]
    c = ctx(L, cfg)
    f = o.synth_frame(64, 32, frame=2)

    def digests():
        planes, st, mean = c.encode_frame(f, 1.0, 2)
        dec = c.decode_frame(planes, st, 64, 32, 1.0, 2)
        return [hashlib.sha1(np.ascontiguousarray(p).tobytes()).hexdigest() for p in planes + [dec]], c.quantizer_info()

    before = digests()
    for other in ("pq10_ycbcr10", "log12_luv8"):
        oc = CFG[other]
        c.set_source_quantizer(*oc, L.build_lut(oc[0], oc[1], oc[4], oc[5]))
        assert digests() == before, other
    # ... and the other way round: a new quantizer keeps the source quantizer
    import torch
    src, a, b = Planes(L, 64, 32, 2, 1), Planes(L, 64, 32, 2, 1), Planes(L, 64, 32, 2, 1)
    fused(c, src, 1.0, a, 1.0)
    c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
    fused(c, src, 1.0, b, 1.0)
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(a.host(), b.host()))
