"""CPU-only checks of the binary16 frame calls (lumahip_*_f16):

1. liblumahip.so exports the seven new symbols and include/lumahip.h declares them.
2. The kernels' narrowing (lumahdrv_amd/csrc/f16_narrow.hpp), compiled by the host compilers into tests/cpp/f16_narrow_check.cpp,
   equals ExrInterface::floatToHalf for all 2^32 float bit patterns.
3. A numpy restatement of floatToHalf (tests/support/host.py float_to_half_np, which the GPU tests use as their expectation) equals numpy's own
   float32 -> float16 conversion for non-NaN floats, on a dense sample and on every rounding boundary; its NaN rule is checked
   separately (numpy keeps a signalling NaN signalling, floatToHalf sets the quiet bit).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.host import float_to_half_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F16_SYMBOLS = ["lumahip_encode_frames_device_f16", "lumahip_encode_frames_device_planar_f16", "lumahip_decode_frames_device_f16",
               "lumahip_decode_frames_device_planar_f16", "lumahip_encode_frame_host_f16", "lumahip_decode_frame_host_f16",
               "lumahip_f16_narrow_probe_device"]


def test_f16_symbols_exported_and_declared(L):
    from lumahdrv_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    declared = set(re.findall(r"\b(lumahip_[a-z0-9_]+)\s*\(", hdr))
    lib = capi.lib()
    for s in F16_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS, s
    assert lib.lumahip_abi_version() == 5
    for cls, names in ((capi.Context, ("encode_frames_device_f16", "encode_frames_device_planar_f16", "decode_frames_device_f16",
                                       "decode_frames_device_planar_f16", "encode_frame_f16", "decode_frame_f16")),
                       (L.LumaFrameCodec, ("encode_half", "decode_half"))):
        for n in names:
            assert callable(getattr(cls, n, None)), n


def _compilers():
    out = []
    for cxx in ("g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if shutil.which(cxx):
            out.append(cxx)
    return out


@pytest.mark.parametrize("cxx", _compilers())
def test_narrowing_equals_float_to_half_for_every_float(L, tmp_path, cxx):
    """tests/cpp/f16_narrow_check.cpp: f16_narrow (as the host compiler builds it) == ExrInterface::floatToHalf, all 2^32 floats"""
    exe = str(tmp_path / "f16_narrow_check")
    lib = os.path.join(ROOT, "lumahdrv_amd", "lib")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lumahdrv_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "f16_narrow_check.cpp"), "-o", exe, "-L" + lib, "-lluma_hip", "-llumahip",
                    "-pthread", "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout


def _boundaries() -> np.ndarray:
    """every rounding boundary of float32 -> float16: the midpoints between adjacent finite halves (exact in float32), the
    overflow threshold, and their float32 neighbours, both signs"""
    h = np.arange(0, 0x7c00, dtype=np.uint16)            # +0 .. 65504
    a = h.view(np.float16).astype(np.float32)
    b = (h + 1).view(np.float16).astype(np.float32)       # (0x7c00: +inf for the last one)
    b[-1] = np.float32(65536.0)                           # the overflow threshold sits where the next binade would start
    mid = (a.astype(np.float64) + b.astype(np.float64)) / 2
    mid32 = mid.astype(np.float32)
    assert np.array_equal(mid32.astype(np.float64), mid)   # exact
    pts = np.concatenate([mid32, a, np.nextafter(mid32, np.float32(np.inf)), np.nextafter(mid32, np.float32(0)),
                          np.array([65504, 65519.996, 65520, 65536, 3.4e38], dtype=np.float32)])
    return np.concatenate([pts, -pts]).astype(np.float32)


def test_numpy_restatement_equals_numpy_conversion_on_non_nan():
    """float_to_half_np == np.float32.astype(np.float16) on a dense sample of all float bit patterns and on every rounding
    boundary (non-NaN floats only: numpy's NaN payloads differ, see the next test)"""
    bits = np.arange(0, 1 << 32, 509, dtype=np.uint64).astype(np.uint32)   # ~8.4 M patterns, every exponent and sign
    for x in (bits.view(np.float32), _boundaries()):
        x = x[~np.isnan(x)]
        with np.errstate(over="ignore"):
            exp = x.astype(np.float16).view(np.uint16)
        got = float_to_half_np(x)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, [(hex(int(x.view(np.uint32)[i])), hex(int(got[i])), hex(int(exp[i]))) for i in bad[:8]]


def test_numpy_restatement_nan_rule():
    """NaN: sign | 0x7e00 | (mantissa >> 13) -- quiet, payload kept, signalling NaNs quieted (0x7f8cfc76 -> 0x7e67)"""
    x = np.array([0x7f8cfc76, 0xff800001, 0x7fc00000, 0xffffffff, 0x7f801fff, 0x7f800000, 0xff800000], dtype=np.uint32)
    got = float_to_half_np(x.view(np.float32))
    assert [hex(int(v)) for v in got] == ["0x7e67", "0xfe00", "0x7e00", "0xffff", "0x7e00", "0x7c00", "0xfc00"]
