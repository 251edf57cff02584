"""Code-domain distortion without a GPU: the exported symbols, code_psnr, and the numpy expectation (tests/support/host.py
expected_distortion) the GPU test (tests/test_gpu_distortion.py) holds the kernels to -- checked here on the reference's own planes in tests/golden/ref_planes.npz:
zeros for `_plane*` against itself, something else than zeros against the garbled `_dec_plane*` copies, for every key (so that
the fixture cases of the GPU test are not vacuous)."""
import math
import os

import numpy as np
import pytest

from tests.support.host import expected_distortion, fixture_keys, key_parts

DIST_SYMBOLS = ["lumahip_distortion_frames_device", "lumahip_distortion_frames_device_planar", "lumahip_distortion_frames_device_f16",
                "lumahip_distortion_frames_device_planar_f16", "lumahip_distortion_frame_host"]


def test_library_exports_the_distortion_symbols():
    from lumahdrv_amd import capi
    L = capi.lib()
    for s in DIST_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.lumahip_abi_version() == 5


def test_code_psnr_is_its_formula():
    from lumahdrv_amd import code_psnr
    assert code_psnr(0, 100, 2047) == float("inf")
    for sse, n, peak in ((1, 1, 255), (123456789, 3840 * 2160, 2047), (2 ** 40, 64 * 32, 65535), (7, 3, 1023)):
        assert code_psnr(sse, n, peak) == pytest.approx(10.0 * math.log10(peak * peak * n / sse), rel=1e-12)
    assert code_psnr(255 * 255 * 10, 10, 255) == pytest.approx(0.0, abs=1e-12)
    assert code_psnr(np.uint64(4), np.uint64(1), 2) == pytest.approx(0.0, abs=1e-12)
    with pytest.raises(ValueError):
        code_psnr(1, 0, 255)


def test_expectation_is_zero_on_equal_planes_and_not_on_the_garbled_ones(golden_dir):
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = fixture_keys(gp)
    assert len(keys) == 16
    for key in keys:
        _, w, h, profile = key_parts(key)
        pl = [gp[key + "_plane%d" % p] for p in range(3)]
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        assert not expected_distortion(pl, pl, w, h, profile).any(), key
        e = expected_distortion(pl, dpl, w, h, profile)
        assert e.any(), key
        assert np.all(e[:, 0] >= e[:, 1]) and np.all(e[:, 1] >= e[:, 2]) and np.all(e[:, 1] >= e[:, 3]), key


def test_expectation_reads_samples_as_the_decoder_does():
    # 16-bit: low byte first; the columns beyond the samples and the rows beyond the plane are not read
    a = np.full((6, 16), 0xC3, dtype=np.uint8)
    b = a.copy()
    a[:4, :8] = 0
    b[:4, :8] = 0
    b[1, 2], b[1, 3] = 0x34, 0x12          # sample (1, 1) = 0x1234
    b[5, 0] = b[0, 9] = 1                  # outside the plane's samples
    e = expected_distortion([a, a, a], [b, a, b], 4, 4, 2)
    assert e[0].tolist() == [0x1234 ** 2, 0x1234, 0x1234, 1]
    assert e[1].tolist() == [0, 0, 0, 0]
    assert e[2].tolist() == [0x1234 ** 2, 0x1234, 0x1234, 1]   # (4:2:0 chroma: 2 x 2 samples, sample (1, 1) at the same bytes)
