"""Distortion map (include/lumahip.h lumahip_distortion_map_frames_device / _planar / _f16 / _planar_f16 /
lumahip_distortion_map_frame_host): lumahip_distortion_frames_device's four words per plane for every block of 16, 32 or 64 luma
pixels squared, written by one launch.  Every expectation is exact equality of integers
(tests/support/host.py expected_distortion_map); before every call the map buffer holds the 0xC3 pattern with 16 guard
words behind it, which must survive.

1. The reference's planes (tests/golden/ref_planes.npz): zeros written over the fill, and numpy's map of the garbled copies.
2. Against lumahip_encode_frames_device's planes perturbed on the host: six configurations x profiles 0-3 x 3 frames x preScalings
   {1, 20, 0.01} x blocks {16, 32, 64} x sizes (34,18) (260,6) (258,6) (264,70) (64,32) (6,4); frame 1 keeps its rightmost block
   column and bottom block row unperturbed; the planar and binary16 forms.
3. The map folds to lumahip_distortion_frames_device's words (in every case of 2).   4. One block's sse beyond 2^32.
5. Launch shapes: 2 workgroups of 64 threads, 1024 threads asked for, the default.   6. A 720p frame twice and in an unordered section.
7. The host form.   8. Errors: nothing is launched.
Every k_distortion_map instantiation, against the oracle's planes: tests/test_gpu_measuring_kernels.py test_measuring_matrix[distortion_map-*].
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden.make_golden import CONFIGS
from tests.support.device import Frames, L, Planes, ctx, dist, dist_map, encode, from_frames, map_buf  # noqa: F401  (L is the module fixture)
from tests.support.host import (BLOCKS, CFG, ENC_CASES, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED, GUARD, MAP_SIZES, OUT_FILL, expect_map,
                                expected_distortion_map, fixture_keys, float_frames, fold_map, key_parts, map_perturbed, map_words,
                                neither_path_is_vacuous, nwords, perturb)

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
        garbled = from_frames(L, [dpl], w, h, profile, strides=gp[key + "_dec_stride"], padding="sentinel")
        for block in BLOCKS:
            got = dist_map(c, fr, sc, same, block)
            assert not got.any(), (key, block, got)
            exp = expected_distortion_map(pl, dpl, w, h, profile, block)
            got = dist_map(c, fr, sc, garbled, block)
            assert exp.any() and np.array_equal(got[0], exp), (key, block, got, exp)


# ---- 2. against the existing encode call, 3. and the map folds to the existing distortion call's words
@pytest.mark.parametrize("name", ENC_CASES)
def test_equals_numpy_on_the_encode_calls_planes(L, name):
    cfg = CFG[name]
    rng = np.random.default_rng(len(name) * 5 + cfg[1])
    c = ctx(L, cfg)
    nf = 3
    scs = (1.0, 20.0, 0.01)
    for profile in range(4):
        for i, (w, h) in enumerate(MAP_SIZES):
            sc = scs[(i + profile) % 3]
            fr = Frames(float_frames(rng, nf, w, h), pad=4 if i % 2 == 0 else 2)
            enc, ebufs = encode(c, L, fr, sc, profile)
            assert c.quantizer_info()["mode"] in (3, 7), "the six configurations are the supported ones"
            for block in BLOCKS:
                given = from_frames(L, map_perturbed(rng, enc, ebufs, w, h, profile, block), w, h, profile, padding="sentinel")
                exp = expect_map(enc, ebufs, given, given.fill, block)
                neither_path_is_vacuous(exp, (w, h))
                assert exp[..., 3].any()
                got = dist_map(c, fr, sc, given, block)
                assert np.array_equal(got, exp), (name, profile, w, h, sc, block, got, exp)
                frame_words = dist(c, fr, sc, given)
                assert np.array_equal(np.stack([fold_map(m) for m in got]), frame_words), (name, profile, w, h, sc, block)
                assert fr.unchanged() and given.unchanged()
            assert not dist_map(c, fr, sc, enc, BLOCKS[(i + profile) % 3]).any(), (name, profile, w, h, sc, "its own planes")
            # rows the vector loads cannot take: odd strides
            if profile in (1, 2) and (w, h) in ((34, 18), (260, 6), (264, 70)):
                block = BLOCKS[(i + profile) % 3]
                odd = from_frames(L, [given.frame(given.fill, f) for f in range(nf)], w, h, profile,
                                  strides=[given.st[p] + 3 for p in range(3)], padding="sentinel")
                assert np.array_equal(dist_map(c, fr, sc, odd, block), expect_map(enc, ebufs, odd, odd.fill, block)), \
                    (name, profile, w, h, "odd strides")


@pytest.mark.parametrize("name,half_table", [("pq11_luv8", 1), ("pq12_rgb", 1), ("pq10_ycbcr10", 2), ("pq10_ycbcr10", 0)])
def test_planar_and_binary16_forms_equal_the_float_call(L, name, half_table):
    cfg = CFG[name]
    rng = np.random.default_rng(17 + half_table)
    c = ctx(L, cfg)
    c.tune("half_table", half_table)
    nf = 3
    for profile in (2, 3, 0):
        for i, (w, h) in enumerate(MAP_SIZES):
            sc = 20.0 if cfg[2] == 2 else 1.0
            frames = float_frames(rng, nf, w, h, halves=True)
            fr = Frames(frames)
            fr16 = Frames(frames, dtype=np.float16)
            enc, ebufs = encode(c, L, fr, sc, profile)
            for block in BLOCKS:
                given = from_frames(L, map_perturbed(rng, enc, ebufs, w, h, profile, block), w, h, profile, padding="sentinel")
                exp = expect_map(enc, ebufs, given, given.fill, block)
                neither_path_is_vacuous(exp, (w, h))
                for form, src in (("packed", fr), ("planar", fr), ("f16", fr16), ("planar_f16", fr16)):
                    got = dist_map(c, src, sc, given, block, form)
                    assert np.array_equal(got, exp), (name, half_table, profile, w, h, block, form, got, exp)
            assert fr16.unchanged()
    if cfg[2] == 2:
        info = c.half_table_info(20.0)
        assert info["used"] == (half_table != 0)


# ---- 4. the 64-bit path: one block's sum of squares is about 1.6e13
@pytest.mark.parametrize("vw4", [True, False])
def test_one_block_sums_beyond_32_bits(L, vw4):
    c = ctx(L, CFG["pq11_luv8"])
    rng = np.random.default_rng(4)
    w, h, profile = 64, 64, 2
    fr = Frames(float_frames(rng, 1, w, h), pad=4 if vw4 else 2)   # (a frame stride of 2 mod 4 floats: two pixels per thread, 32 lanes per block)
    enc, ebufs = encode(c, L, fr, 1.0, profile)
    ones = Planes(L, w, h, profile, 1, fill=[np.full(enc.pfs[p], 0xFF, dtype=np.uint8) for p in range(3)])
    exp = expect_map(enc, ebufs, ones, ones.fill, 64)
    assert exp.shape == (1, 1, 1, 3, 4) and exp[0, 0, 0, 0, 0] > np.uint64(10) ** np.uint64(13)
    assert np.all(exp[..., 0] > np.uint64(1) << np.uint64(32))
    got = dist_map(c, fr, 1.0, ones, 64)
    assert np.array_equal(got, exp), (got, exp)


# ---- 5. launch shapes
@pytest.mark.parametrize("name,profile", [("pq11_luv8", 2), ("pq10_ycbcr10", 3), ("pq12_rgb", 0)])
def test_launch_shapes_give_identical_maps(L, name, profile):
    cfg = CFG[name]
    sc = 20.0 if cfg[2] == 2 else 1.0
    rng = np.random.default_rng(50 + profile)
    nf = 3
    shapes = {}
    for shape in ("default", "two_workgroups_of_64", "1024_threads"):
        c = ctx(L, cfg)
        if shape == "two_workgroups_of_64":      # the persistent loop, the frame change, the most sub-tiles per map tile
            c.tune("block", 64)
            c.tune("grid_enc", 2)
        elif shape == "1024_threads":            # more rows per standard tile than a block of 16 has: the dispatcher clamps
            c.tune("block", 1024)
        shapes[shape] = c
    for (w, h) in ((264, 70), (34, 18)):
        fr = Frames(float_frames(rng, nf, w, h))
        enc, ebufs = encode(shapes["default"], L, fr, sc, profile)
        for block in BLOCKS:
            given = from_frames(L, map_perturbed(rng, enc, ebufs, w, h, profile, block), w, h, profile, padding="sentinel")
            exp = expect_map(enc, ebufs, given, given.fill, block)
            for shape, c in shapes.items():
                got = dist_map(c, fr, sc, given, block)
                assert np.array_equal(got, exp), (name, w, h, block, shape, got, exp)


# ---- 6. repeatability and section
@pytest.mark.parametrize("name", ["pq11_luv8", "pq10_ycbcr10"])
def test_one_720p_frame_twice_and_in_an_unordered_section(L, name):
    import torch
    cfg = CFG[name]
    sc = 20.0 if cfg[2] == 2 else 1.0
    c = ctx(L, cfg)
    rng = np.random.default_rng(721)
    w, h, profile, block = 1280, 720, 2, 64
    fr = Frames(float_frames(rng, 1, w, h))
    enc, ebufs = encode(c, L, fr, sc, profile)
    given = from_frames(L, map_perturbed(rng, enc, ebufs, w, h, profile, block)[:1], w, h, profile, padding="sentinel")
    exp = expect_map(enc, ebufs, given, given.fill, block)
    a = dist_map(c, fr, sc, given, block)
    b = dist_map(c, fr, sc, given, block)
    assert np.array_equal(a, exp), (a, exp)
    assert np.array_equal(a, b)
    bufs = [map_buf(nwords(1, w, h, block)) for _ in range(2)]
    torch.cuda.synchronize()
    c.begin_unordered(2)
    for buf in bufs:
        c.distortion_map_frames_device(fr.ptr, fr.fs, 1, w, h, sc, profile, given.ptrs, given.st, given.pfs, block, buf.data_ptr())
    c.end_unordered()
    c.sync()
    torch.cuda.synchronize()
    for buf in bufs:
        assert np.array_equal(map_words(buf, 1, w, h, block), a)
    assert fr.unchanged() and given.unchanged()


# ---- 7. the host form
def test_host_form_equals_the_device_call(L):
    rng = np.random.default_rng(8)
    for name, profile, (w, h), block in (("pq11_luv8", 2, (260, 6), 16), ("pq10_ycbcr10", 3, (34, 18), 16), ("linear12_luv8", 1, (264, 70), 64),
                                         ("pq11_luv8", 0, (264, 70), 32)):
        cfg = CFG[name]
        sc = 20.0 if cfg[2] == 2 else 1.0
        c = ctx(L, cfg)
        frames = float_frames(rng, 1, w, h)
        fr = Frames(frames)
        enc, ebufs = encode(c, L, fr, sc, profile)
        given = from_frames(L, [perturb(rng, enc.frame(ebufs, 0), w, h, profile, frac=0.5)], w, h, profile, padding="sentinel")
        dev = dist_map(c, fr, sc, given, block)
        host = c.distortion_map_frame(frames[0], given.frame(given.fill, 0), given.st, sc, profile, block)
        assert host.dtype == np.uint64 and host.shape == dev[0].shape and np.array_equal(host, dev[0]), (name, host, dev)
        assert dev.any()


# ---- 8. errors: nothing is launched, the map is left as it was
def test_errors_launch_nothing(L):
    import torch
    rng = np.random.default_rng(9)
    w, h, nf, profile = 34, 18, 1, 2
    frames = float_frames(rng, nf, w, h)
    fr = Frames(frames)
    given = Planes(L, w, h, profile, nf)

    def refused(c, code, w=w, block=16, map_ptr="own"):
        buf = map_buf(nwords(nf, 34, 18, 16))
        ptr = buf.data_ptr() if map_ptr == "own" else map_ptr(buf)
        with pytest.raises(L.LumaHipError) as ei:
            c.distortion_map_frames_device(fr.ptr, fr.fs, nf, w, h, 1.0, profile, given.ptrs, given.st, given.pfs, block, ptr)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == OUT_FILL)

    good = ctx(L, CFG["pq11_luv8"])
    for block in (8, 48, 0, 128):
        refused(good, ERR_ARG, block=block)                                         # bad block
    refused(ctx(L, CFG["pq11_luv8"], quantizer=False), ERR_STATE)                  # no quantizer
    refused(good, ERR_ARG, w=33)                                                    # odd size
    refused(good, ERR_ARG, map_ptr=lambda o: o.data_ptr() + 4)                      # misaligned map_dev
    refused(good, ERR_ARG, map_ptr=lambda o: None)                                  # null map_dev
    refused(good, ERR_ARG, map_ptr=lambda o: given.ptrs[0] + 64)                    # map_dev inside a given plane
    # ... and one whose first 12 words lie in front of the plane: the map's own byte count decides (6 blocks: 576 bytes)
    refused(good, ERR_ARG, map_ptr=lambda o: given.ptrs[1] - 200)
    refused(good, ERR_ARG, map_ptr=lambda o: fr.ptr + 8 * (w * h // 2))             # map_dev inside the frame
    refused(good, ERR_ARG, map_ptr=lambda o: fr.ptr - 200)                          # ... reaching into it
    refused(ctx(L, CFG["pq11_luv8"], literal=True), ERR_UNSUPPORTED)               # force_literal
    refused(ctx(L, CFG["pq14_luv8"]), ERR_UNSUPPORTED)                             # a 14-bit table: records in global memory
    # the host form: map_words one short, and a bad block
    planes = given.frame(given.fill, 0)
    need = nwords(1, w, h, 16)
    for block, words in ((16, need - 1), (8, need)):
        m = np.full(need + GUARD, OUT_FILL, dtype=np.int64)
        rc = good.L.lumahip_distortion_map_frame_host(good.h, frames[0].ctypes.data, w, h, 1.0, profile,
                                                      (C.c_void_p * 3)(*[p.ctypes.data for p in planes]), (C.c_int * 3)(*given.st), block,
                                                      m.ctypes.data, words)
        assert rc == ERR_ARG and np.all(m == OUT_FILL), (block, words, rc)
    assert fr.unchanged() and given.unchanged()
    # ... and the same arguments are accepted by a context that can
    assert dist_map(good, fr, 1.0, given, 16).shape == (1, 2, 3, 3, 4)
    assert good.distortion_map_frame(frames[0], planes, given.st, 1.0, profile, 16).shape == (2, 3, 3, 4)
