"""The distortion map without a GPU: the exported symbols, lumahip_distortion_map_dims, block_sample_counts, and the numpy
expectation the GPU test (tests/test_gpu_distortion_map.py) holds the kernels to -- checked here against the per-frame expectation
(both in tests/support/host.py) on the reference's own planes in tests/golden/ref_planes.npz, and on a hand-made case that pins which
block a 4:2:0 chroma sample belongs to."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.support.host import BLOCKS, expected_distortion, expected_distortion_map, fixture_keys, fold_map, key_parts

MAP_SYMBOLS = ["lumahip_distortion_map_dims", "lumahip_distortion_map_frames_device", "lumahip_distortion_map_frames_device_planar",
               "lumahip_distortion_map_frames_device_f16", "lumahip_distortion_map_frames_device_planar_f16",
               "lumahip_distortion_map_frame_host"]


def test_library_exports_the_map_symbols():
    from lumahdrv_amd import capi
    L = capi.lib()
    for s in MAP_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.lumahip_abi_version() == 5


def test_map_dims():
    from lumahdrv_amd import capi
    assert capi.distortion_map_dims(34, 18, 16) == (3, 2)
    assert capi.distortion_map_dims(64, 32, 64) == (1, 1)
    assert capi.distortion_map_dims(3840, 2160, 64) == (60, 34)
    L = capi.lib()
    for block in (8, 48, 0):
        nbx, nby = C.c_uint(77), C.c_uint(77)
        assert L.lumahip_distortion_map_dims(64, 64, block, C.byref(nbx), C.byref(nby)) == capi.ERR_ARG, block
        assert (nbx.value, nby.value) == (77, 77)
        with pytest.raises(capi.LumaHipError):
            capi.distortion_map_dims(64, 64, block)


def test_expected_map_folds_to_the_frame_expectation(golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        _, w, h, profile = key_parts(key)
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        frame = expected_distortion(pl, dpl, w, h, profile)
        for block in BLOCKS:
            m = expected_distortion_map(pl, dpl, w, h, profile, block)
            assert m.shape == (-(-h // block), -(-w // block), 3, 4)
            assert np.array_equal(fold_map(m), frame), (key, block)
            assert not expected_distortion_map(pl, pl, w, h, profile, block).any(), (key, block)


def test_expected_map_puts_chroma_samples_into_their_blocks():
    # 40 x 36 pixels, 4:2:0, 16-bit, blocks of 16: 3 x 3 blocks; the chroma planes are 20 x 18 samples in blocks of 8
    w, h = 40, 36
    ya = np.full((h + 2, 2 * w + 6), 0xC3, dtype=np.uint8)
    ca = np.full((h // 2 + 2, w + 6), 0xC3, dtype=np.uint8)
    ya[:h, :2 * w] = 0
    ca[:h // 2, :w] = 0
    yb, ub, vb = ya.copy(), ca.copy(), ca.copy()
    yb[17, 2 * 33], yb[17, 2 * 33 + 1] = 0x34, 0x12      # luma pixel (x 33, y 17) = 0x1234: block (2, 1)
    ub[7, 2 * 8] = 5                                     # U sample (x 8, y 7): co-sited with luma (16..17, 14..15): block (1, 0)
    ub[8, 2 * 7] = 3                                     # U sample (x 7, y 8): block (0, 1)
    vb[17, 2 * 19], vb[17, 2 * 19 + 1] = 2, 1            # V sample (x 19, y 17) = 0x0102: the last one, block (2, 2)
    yb[h, 0] = yb[0, 2 * w] = ub[h // 2, 0] = ub[0, w] = vb[0, w + 1] = 1   # bytes outside the samples do not count
    m = expected_distortion_map([ya, ca, ca], [yb, ub, vb], w, h, 2, 16)
    assert m.shape == (3, 3, 3, 4)
    want = np.zeros((3, 3, 3, 4), dtype=np.uint64)
    want[1, 2, 0] = (0x1234 ** 2, 0x1234, 0x1234, 1)
    want[0, 1, 1] = (25, 5, 5, 1)
    want[1, 0, 1] = (9, 3, 3, 1)
    want[2, 2, 2] = (0x0102 ** 2, 0x0102, 0x0102, 1)
    assert np.array_equal(m, want)
    # 4:4:4 (profile 3): the same bytes are chroma samples of full-size blocks -- only planes of the luma's size make sense there
    m3 = expected_distortion_map([ya, ya, ya], [yb, ya, yb], w, h, 3, 16)
    assert m3[1, 2, 0].tolist() == m3[1, 2, 2].tolist() == [0x1234 ** 2, 0x1234, 0x1234, 1] and not m3[:, :, 1].any()
    assert int(np.count_nonzero(m3[:, :, :, 3])) == 2


def test_block_sample_counts():
    from lumahdrv_amd import block_sample_counts
    for w, h in ((34, 18), (64, 32), (264, 70), (6, 4)):
        for profile in range(4):
            for block in BLOCKS:
                n = block_sample_counts(w, h, profile, block)
                assert n.shape == (-(-h // block), -(-w // block), 3) and n.dtype == np.int64
                cw, ch = (w // 2, h // 2) if profile in (0, 2) else (w, h)
                assert n.sum(axis=(0, 1)).tolist() == [w * h, cw * ch, cw * ch]
                assert (n > 0).all()
    # 34 x 18 in blocks of 16: columns of 16, 16, 2 pixels, rows of 16 and 2
    n2 = block_sample_counts(34, 18, 2, 16)
    assert n2[:, :, 0].tolist() == [[256, 256, 32], [32, 32, 4]]
    assert n2[:, :, 1].tolist() == n2[:, :, 2].tolist() == [[64, 64, 8], [8, 8, 1]]
    n3 = block_sample_counts(34, 18, 3, 16)
    assert n3[:, :, 0].tolist() == n3[:, :, 1].tolist() == n3[:, :, 2].tolist() == [[256, 256, 32], [32, 32, 4]]
    assert block_sample_counts(34, 18, 3, 64).tolist() == [[[612, 612, 612]]]
    assert block_sample_counts(34, 18, 2, 32).tolist() == [[[576, 144, 144], [36, 9, 9]]]
