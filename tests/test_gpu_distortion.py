"""Code-domain distortion (include/lumahip.h lumahip_distortion_frames_device / _planar / _f16 / _planar_f16 /
lumahip_distortion_frame_host): per frame and plane {sse, sad, max_abs, n_differ} of the planes the encode call would write
against GIVEN planes.  Every expectation is exact equality of all twelve integers per frame.

1. The reference's planes (tests/golden/ref_planes.npz): `_in` against `_plane*` is all zeros, against the garbled `_dec_plane*`
   it is numpy's sums over the two sets.
2. Against lumahip_encode_frames_device: its planes, perturbed on the host, six configurations x profiles 0-3 x sizes (34,18)
   (258,6) (64,32) (6,4) x 3 frames x preScalings {1, 20, 0.01}; sentinel bytes in every gap; the planar and binary16 forms.
3. Accumulator width (one wave carries more than 2^32).  4. Persistent loop and frame change (2 workgroups of 64 threads).
5. Unordered section, one 1280x720 frame, repeatability, inputs untouched.  6. The host form.  7. Errors: nothing is launched.
Every k_distortion instantiation, against the oracle's planes: tests/test_gpu_measuring_kernels.py test_measuring_matrix[distortion-*].
"""
import os

import numpy as np
import pytest

from tests.golden.make_golden import CONFIGS
from tests.support.device import Frames, L, Planes, ctx, dist, encode, from_frames, out_buf, out_words  # noqa: F401  (L is the module fixture)
from tests.support.host import (CFG, ENC_CASES, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, OUT_FILL, SIZES, expect, expected_distortion, fixture_keys,
                                float_frames, key_parts, perturb)

pytestmark = pytest.mark.gpu


# ---- 1. the reference's planes
def test_reference_planes_and_their_garbled_copies(L, golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        name, w, h, profile = key_parts(key)
        cfg = CONFIGS[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = ctx(L, cfg)
        fr = Frames(gp[key + "_in"][None])
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        same = from_frames(L, [pl], w, h, profile, strides=gp[key + "_stride"], padding="sentinel")
        got = dist(c, fr, sc, same)
        assert not got.any(), (key, got)
        garbled = from_frames(L, [dpl], w, h, profile, strides=gp[key + "_dec_stride"], padding="sentinel")
        got = dist(c, fr, sc, garbled)
        exp = expected_distortion(pl, dpl, w, h, profile)
        assert exp.any() and np.array_equal(got[0], exp), (key, got, exp)
        assert np.array_equal(c.distortion_frame(gp[key + "_in"], dpl, garbled.st, sc, profile), exp), (key, "host")


# ---- 2. against the existing encode call
@pytest.mark.parametrize("name", ENC_CASES)
def test_equals_numpy_on_the_encode_calls_planes(L, name):
    cfg = CFG[name]
    rng = np.random.default_rng(len(name) * 7 + cfg[1])
    c = ctx(L, cfg)
    nf = 3
    scs = (1.0, 20.0, 0.01)
    first = True
    for profile in range(4):
        for i, (w, h) in enumerate(SIZES):
            sc = scs[(i + profile) % 3]
            fr = Frames(float_frames(rng, nf, w, h), pad=4 if i % 2 == 0 else 2)
            enc, ebufs = encode(c, L, fr, sc, profile)
            if first:
                first = False
                mode = c.quantizer_info()["mode"]
                if mode not in (3, 7):   # ("where its records are in LDS": anything else is refused)
                    with pytest.raises(L.LumaHipError) as ei:
                        dist(c, fr, sc, enc)
                    assert ei.value.code == ERR_UNSUPPORTED
                    return
                if name == "linear12_luv8":
                    assert mode == 7
            given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile, padding="sentinel")
            exp = expect(enc, ebufs, given, given.fill)
            assert exp[:, :, 3].any(axis=1).all(), "every frame differs somewhere"
            got = dist(c, fr, sc, given)
            assert np.array_equal(got, exp), (name, profile, w, h, sc, got, exp)
            assert not dist(c, fr, sc, enc).any(), (name, profile, w, h, sc, "its own planes")
            assert fr.unchanged() and given.unchanged()
            # rows the vector loads cannot take: odd strides
            if profile in (1, 2) and (w, h) != (6, 4):
                odd = from_frames(L, [given.frame(given.fill, f) for f in range(nf)], w, h, profile,
                                  strides=[given.st[p] + 3 for p in range(3)], padding="sentinel")
                assert np.array_equal(dist(c, fr, sc, odd), exp), (name, profile, w, h, "odd strides")


@pytest.mark.parametrize("name,half_table", [("pq11_luv8", 1), ("pq12_rgb", 1), ("pq10_ycbcr10", 2), ("pq10_ycbcr10", 0)])
def test_planar_and_binary16_forms_equal_the_float_call(L, name, half_table):
    cfg = CFG[name]
    rng = np.random.default_rng(11 + half_table)
    c = ctx(L, cfg)
    c.tune("half_table", half_table)
    nf = 3
    for profile in (2, 3, 0):
        for (w, h) in SIZES:
            sc = 20.0 if cfg[2] == 2 else 1.0
            frames = float_frames(rng, nf, w, h, halves=True)
            fr = Frames(frames)
            fr16 = Frames(frames, dtype=np.float16)
            enc, ebufs = encode(c, L, fr, sc, profile)
            given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile, padding="sentinel")
            exp = expect(enc, ebufs, given, given.fill)
            for form, src in (("packed", fr), ("planar", fr), ("f16", fr16), ("planar_f16", fr16)):
                got = dist(c, src, sc, given, form)
                assert np.array_equal(got, exp), (name, half_table, profile, w, h, form, got, exp)
            assert fr16.unchanged()
    if cfg[2] == 2:
        info = c.half_table_info(20.0)
        assert info["used"] == (half_table != 0)


# ---- 3. accumulator width: one wave carries more than 2^32 of squared difference per plane
def test_one_wave_accumulates_beyond_32_bits(L):
    c = ctx(L, CFG["pq11_luv8"])
    c.tune("grid_enc", 1)
    c.tune("block", 64)
    rng = np.random.default_rng(3)
    w, h, nf, profile = 64, 32, 3, 2
    fr = Frames(float_frames(rng, nf, w, h))
    enc, ebufs = encode(c, L, fr, 1.0, profile)
    ones = Planes(L, w, h, profile, nf, fill=[np.full(nf * enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
    exp = expect(enc, ebufs, ones, ones.fill)
    assert np.all(exp[:, :, 0] > np.uint64(1) << np.uint64(32))
    got = dist(c, fr, 1.0, ones)
    assert np.array_equal(got, exp), (got, exp)


# ---- 4. persistent loop and frame change
@pytest.mark.parametrize("size", [(6, 4), (258, 6)])
def test_two_workgroups_book_every_frame_to_itself(L, size):
    w, h = size
    rng = np.random.default_rng(w)
    nf = 3
    for name, profile in (("pq11_luv8", 2), ("pq10_ycbcr10", 3), ("pq12_rgb", 0)):
        cfg = CFG[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = ctx(L, cfg)
        c.tune("grid_enc", 2)
        c.tune("block", 64)
        fr = Frames(float_frames(rng, nf, w, h))
        enc, ebufs = encode(c, L, fr, sc, profile)
        # frame f: its own share of perturbed samples and its own amplitude
        given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, profile, frac=0.2 + 0.3 * f, amp=1 + 3 * f, extremes=f)
                                for f in range(nf)], w, h, profile, padding="sentinel")
        exp = expect(enc, ebufs, given, given.fill)
        assert len({tuple(e.ravel()) for e in exp}) == nf
        got = dist(c, fr, sc, given)
        assert np.array_equal(got, exp), (name, size, got, exp)


# ---- 5. run-time behaviour
def test_unordered_section_two_batches_on_two_lanes(L):
    import torch
    c = ctx(L, CFG["pq11_luv8"])
    rng = np.random.default_rng(5)
    w, h, nf, profile = 258, 6, 3, 2
    batches = []
    for _ in range(2):
        fr = Frames(float_frames(rng, nf, w, h))
        enc, ebufs = encode(c, L, fr, 1.0, profile)
        given = from_frames(L, [perturb(rng, enc.frame(ebufs, f), w, h, profile) for f in range(nf)], w, h, profile, padding="sentinel")
        batches.append((fr, given, expect(enc, ebufs, given, given.fill), out_buf(nf)))
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for fr, given, _, out in batches:
        c.distortion_frames_device(fr.ptr, fr.fs, nf, w, h, 1.0, profile, given.ptrs, given.st, given.pfs, out.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for fr, given, exp, out in batches:
        assert np.array_equal(out_words(out, nf), exp)


@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10"])
def test_one_720p_frame_twice(L, name):
    cfg = CFG[name]
    sc = 20.0 if cfg[2] == 2 else 1.0
    c = ctx(L, cfg)
    rng = np.random.default_rng(720)
    w, h, profile = 1280, 720, 2
    fr = Frames(float_frames(rng, 1, w, h))
    enc, ebufs = encode(c, L, fr, sc, profile)
    given = from_frames(L, [perturb(rng, enc.frame(ebufs, 0), w, h, profile)], w, h, profile, padding="sentinel")
    exp = expect(enc, ebufs, given, given.fill)
    a = dist(c, fr, sc, given)
    b = dist(c, fr, sc, given)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(a, b)
    assert fr.unchanged() and given.unchanged()


# ---- 6. the host form
def test_host_form_equals_the_device_call(L):
    rng = np.random.default_rng(6)
    for name, profile, (w, h) in (("pq11_luv8", 2, (258, 6)), ("pq10_ycbcr10", 3, (34, 18)), ("linear12_luv8", 1, (64, 32))):
        cfg = CFG[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = ctx(L, cfg)
        frames = float_frames(rng, 1, w, h)
        fr = Frames(frames)
        enc, ebufs = encode(c, L, fr, sc, profile)
        g = perturb(rng, enc.frame(ebufs, 0), w, h, profile)
        given = from_frames(L, [g], w, h, profile, padding="sentinel")
        dev = dist(c, fr, sc, given)
        host = c.distortion_frame(frames[0], given.frame(given.fill, 0), given.st, sc, profile)
        assert host.dtype == np.uint64 and np.array_equal(host, dev[0]), (name, host, dev)
        assert dev.any()


# ---- 7. errors: nothing is launched, out_dev is left as it was
def test_errors_launch_nothing(L):
    import torch
    rng = np.random.default_rng(7)
    w, h, nf, profile = 34, 18, 1, 2
    frames = float_frames(rng, nf, w, h)
    fr = Frames(frames)
    given = Planes(L, w, h, profile, nf)

    def refused(c, code, fr=fr, w=w, out_ptr="own", given=given):
        out = out_buf(nf)
        ptr = out.data_ptr() if out_ptr == "own" else out_ptr(out)
        with pytest.raises(L.LumaHipError) as ei:
            c.distortion_frames_device(fr.ptr, fr.fs, nf, w, h, 1.0, profile, given.ptrs, given.st, given.pfs, ptr)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == OUT_FILL)

    good = ctx(L, CFG["pq11_luv8"])
    refused(ctx(L, CFG["pq11_luv8"], quantizer=False), ERR_STATE)                  # no quantizer
    refused(good, ERR_ARG, w=33)                                                    # odd size
    refused(good, ERR_ARG, out_ptr=lambda o: o.data_ptr() + 4)                      # misaligned out_dev
    refused(good, ERR_ARG, out_ptr=lambda o: None)                                  # null out_dev
    refused(good, ERR_ARG, out_ptr=lambda o: given.ptrs[0] + 64)                    # out_dev inside a given plane
    refused(good, ERR_ARG, out_ptr=lambda o: fr.ptr + 8 * (w * h // 2))             # out_dev inside the frame
    refused(ctx(L, CFG["pq11_luv8"], literal=True), ERR_UNSUPPORTED)               # force_literal
    refused(ctx(L, CFG["pq14_luv8"]), ERR_UNSUPPORTED)                             # a 14-bit table: records in global memory
    assert fr.unchanged() and given.unchanged()
    # ... and the same arguments are accepted by a context that can
    assert dist(good, fr, 1.0, given).shape == (1, 3, 4)
