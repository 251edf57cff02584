"""ctypes binding of include/lumahip.h (the C ABI of liblumahip.so).  Nothing here computes pixels."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# LUMAHIP_LIB: load another build of the same ABI (A/B measurements, the -DLH_NO_FAST_DIV comparison build of the tests)
_LIB_PATH = os.environ.get("LUMAHIP_LIB") or os.path.join(HERE, "lib", "liblumahip.so")

# include/luma/luma_quantizer.h:95-96 (values are serialised in the stream metadata)
PTF_PSI, PTF_PQ, PTF_LOG, PTF_JND_HDRVDP, PTF_LINEAR = range(5)
CS_LUV, CS_RGB, CS_YCBCR, CS_XYZ = range(4)

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = range(5)

PROBE_FN = C.CFUNCTYPE(C.c_double, C.c_int, C.c_int, C.c_void_p)


class PoolConfig(C.Structure):
    """lumahip_pool_config (include/lumahip.h)"""
    _fields_ = [("chunk_bytes", C.c_size_t), ("n_float", C.c_int), ("n_y", C.c_int), ("n_uv", C.c_int), ("n_striped", C.c_int),
                ("keep_free_bytes", C.c_size_t), ("max_chunks", C.c_int), ("probe_iters", C.c_int)]


_vp, _u, _i, _f, _sz, _str = C.c_void_p, C.c_uint, C.c_int, C.c_float, C.c_size_t, C.c_char_p
_p3, _i3, _s3 = C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_size_t)       # T name[3] and other T * parameters
_fp, _up, _dp, _lp = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_double), C.POINTER(C.c_long)
# the parameter runs that many entry points share, ctx first
_QUANTIZER = (_vp, _i, _u, _i, _u, _f, _f, _vp, _sz)                        # ptf, bitdepth, cs, bitdepthC, max_lum, min_lum, lut, n
_FRAMES = (_vp, _vp, _sz, _u, _u, _u, _f, _i, _p3, _i3, _s3)                # frames, frame_stride, nframes, w, h, sc, profile, plane triplets
_PLANAR = (_vp, _p3) + _FRAMES[2:]                                          # the same with three colour-plane pointers
_PLANES = (_vp, _p3, _i3, _s3, _u, _u, _u, _i, _f)                          # plane triplets, nframes, w, h, profile, sc
_TWO_SETS = (_vp, _p3, _i3, _s3, _i, _f, _u, _u, _u, _p3, _i3, _s3, _i, _f)  # source triplets, profile, sc, nframes, w, h, target ...
_FRAME_HOST = (_vp, _vp, _u, _u, _f, _i, _p3, _i3)                          # rgb, w, h, sc, profile, planes, strides
_PLANES_HOST = (_vp, _p3, _i3, _u, _u, _i, _f)                              # planes, strides, w, h, profile, sc
_TWO_SETS_HOST = (_vp, _p3, _i3, _i, _f, _u, _u, _p3, _i3, _i, _f)
_FRAMES_HOST = (_vp, _p3, _u, _u, _u, _f, _i, _p3, _i3, _fp)                # frames[n], n, w, h, sc, profile, planes[3n], strides, means
_PLANES_FRAMES_HOST = (_vp, _p3, _i3, _u, _u, _u, _i, _f, _p3)
_ARRAY = (_vp, _vp, _vp, _sz, _u)                                           # in, out, n, channel
_MAP_DIMS = (_u, _u, _u, _up, _up)
_PROBE = (_vp, _vp, C.c_uint32, _sz)                                        # out, first_bits, n

# include/lumahip.h, one entry per declaration: name -> (restype, argtypes).  The only place a signature is written: lib() applies it,
# SYMBOLS lists it, tests/test_capi_abi_host.py holds it against the header.
_ABI = {
    "lumahip_abi_version": (_i, ()),
    "lumahip_device_count": (_i, (_i3,)),
    "lumahip_create": (_i, (_p3, _i)),
    "lumahip_destroy": (None, (_vp,)),
    "lumahip_last_error": (_str, (_vp,)),
    "lumahip_set_stream": (_i, (_vp, _vp)),
    "lumahip_reset_stream": (_i, (_vp,)),
    "lumahip_sync": (_i, (_vp,)),
    "lumahip_tune": (_i, (_vp, _str, C.c_long)),
    "lumahip_set_quantizer": (_i, _QUANTIZER),
    "lumahip_build_lut": (_i, (_i, _u, _f, _f, _vp, _sz)),
    "lumahip_thresh_index_host": (_i, (_vp, _sz, _i3, _vp, _sz)),
    "lumahip_lin_index_host": (_i, (_vp, _sz, _i3, _vp, _sz)),
    "lumahip_ycbcr_luma_index_host": (_i, (_vp, _sz, _f, _i3, _vp, _sz)),
    "lumahip_ycbcr_ytab_host": (_i, (_vp, _sz, _f, _vp)),
    "lumahip_ycbcr_half_table_host": (_i, (_f, _f, _vp, _sz)),
    "lumahip_half_table_info": (_i, (_vp, _f, _i3)),
    "lumahip_rb_table_info": (_i, (_vp, _f, _i3)),
    "lumahip_quantize_value_host": (_i, (_vp, _sz, _i, _u, _f, _u, _fp)),
    "lumahip_dequantize_value_host": (_i, (_vp, _sz, _i, _u, _f, _u, _fp)),
    "lumahip_half_upload_info": (_i, (_vp, _lp)),
    "lumahip_numa_info": (_i, (_vp, _i3)),
    "lumahip_numa_pin_current_thread": (_i, (_vp,)),
    "lumahip_numa_plan_host": (_i, (_str, _str, _str, _i3, _i3, _i, _i3)),
    "lumahip_quantizer_info": (_i, (_vp, _i3)),
    "lumahip_encode_stream_push": (_i, _FRAME_HOST),
    "lumahip_encode_stream_pop": (_i, (_vp, _fp)),
    "lumahip_encode_stream_pending": (_i, (_vp,)),
    "lumahip_decode_stream_push": (_i, _PLANES_HOST + (_vp,)),
    "lumahip_decode_stream_pop": (_i, (_vp,)),
    "lumahip_decode_stream_pending": (_i, (_vp,)),
    "lumahip_encode_frame_host": (_i, _FRAME_HOST + (_fp, _vp)),
    "lumahip_decode_frame_host": (_i, _PLANES_HOST + (_vp,)),
    "lumahip_encode_frames_host": (_i, _FRAMES_HOST),
    "lumahip_decode_frames_host": (_i, _PLANES_FRAMES_HOST),
    "lumahip_pack_frame_host": (_i, (_vp, _vp, _u, _u, _i, _p3, _i3, _fp)),
    "lumahip_unpack_frame_host": (_i, (_vp, _p3, _i3, _u, _u, _i, _vp)),
    "lumahip_transform_color_space_host": (_i, (_vp, _vp, _u, _u, _i, _f)),
    "lumahip_quantize_array_host": (_i, _ARRAY),
    "lumahip_dequantize_array_host": (_i, _ARRAY),
    "lumahip_quantize_array_device": (_i, _ARRAY),
    "lumahip_dequantize_array_device": (_i, _ARRAY),
    "lumahip_encode_frames_device": (_i, _FRAMES + (_vp,)),
    "lumahip_mean_luminance_reference_device": (_i, (_vp, _vp, _u, _u, _f, _fp)),
    "lumahip_decode_frames_device": (_i, _PLANES + (_vp, _sz)),
    "lumahip_decode_frames_device_rotating": (_i, _PLANES + (_p3, _sz)),
    "lumahip_decode_display_frames_device": (_i, _PLANES + (_vp, _sz, _vp, _i, _sz, _f, _f, _i, _i)),
    "lumahip_transform_color_space_device": (_i, (_vp, _vp, _sz, _u, _u, _u, _i, _f)),
    "lumahip_synth_frames_device": (_i, (_vp, _vp, _sz, _u, _u, _u, C.c_uint64, C.c_uint64)),
    "lumahip_device": (_i, (_vp,)),
    "lumahip_encode_frames_device_planar": (_i, _PLANAR + (_vp,)),
    "lumahip_decode_frames_device_planar": (_i, _PLANES + (_p3, _sz)),
    "lumahip_begin_unordered": (_i, (_vp, _i)),
    "lumahip_end_unordered": (_i, (_vp,)),
    "lumahip_probe_decode_traffic_device": (_i, _PLANES[:7] + (_p3, _sz, _i, _fp)),
    "lumahip_decoded_ring_create": (_i, (_vp, _u, _u, _u, _u, _p3)),
    "lumahip_decoded_ring_destroy": (None, (_vp,)),
    "lumahip_decoded_ring_info": (_i, (_vp, _i3, _s3)),
    "lumahip_decoded_ring_frame": (_vp, (_vp, _u, _u)),
    "lumahip_decode_frames_device_ring": (_i, (_vp, _p3, _i3, _s3, _u, _i, _f, _vp, _u)),
    "lumahip_pool_create": (_i, (_vp, C.POINTER(PoolConfig), _p3)),
    "lumahip_pool_create_small": (_i, (_vp, _i, _i, _i, _i, _p3)),
    "lumahip_pool_destroy": (None, (_vp,)),
    "lumahip_pool_alloc": (_i, (_vp, _i, _i, _p3)),
    "lumahip_pool_release": (_i, (_vp, _vp)),
    "lumahip_pool_available": (_i, (_vp, _i, _i)),
    "lumahip_pool_group_of": (_i, (_vp, _vp)),
    "lumahip_pool_stats_json": (_str, (_vp,)),
    "lumahip_pool_find_groups": (_i, (_i, PROBE_FN, _vp, _vp, _i3, _dp, _i3)),
    "lumahip_multi_create": (_i, (_p3, _i3, _i)),
    "lumahip_multi_destroy": (None, (_vp,)),
    "lumahip_multi_shards": (_i, (_vp,)),
    "lumahip_multi_ctx": (_vp, (_vp, _i)),
    "lumahip_multi_last_error": (_str, (_vp,)),
    "lumahip_multi_used_rccl": (_i, (_vp,)),
    "lumahip_multi_set_transport": (_i, (_vp, _i)),
    "lumahip_multi_transport_note": (_str, (_vp,)),
    "lumahip_shard_range": (_i, (_u, _i, _i, _up, _up)),
    "lumahip_multi_set_quantizer": (_i, _QUANTIZER),
    "lumahip_multi_encode_frames_host": (_i, _FRAMES_HOST),
    "lumahip_multi_decode_frames_host": (_i, _PLANES_FRAMES_HOST),
    "lumahip_multi_encode_frames_device": (_i, (_vp, _p3, _sz, _up, _u, _u, _f, _i, _p3, _i3, _s3)),
    "lumahip_multi_decode_frames_device": (_i, (_vp, _p3, _i3, _s3, _up, _u, _u, _i, _f, _p3, _sz)),
    "lumahip_multi_sync": (_i, (_vp,)),
    "lumahip_encode_frames_device_f16": (_i, _FRAMES + (_vp,)),
    "lumahip_encode_frames_device_planar_f16": (_i, _PLANAR + (_vp,)),
    "lumahip_decode_frames_device_f16": (_i, _PLANES + (_vp, _sz)),
    "lumahip_decode_frames_device_planar_f16": (_i, _PLANES + (_p3, _sz)),
    "lumahip_encode_frame_host_f16": (_i, _FRAME_HOST + (_fp,)),
    "lumahip_decode_frame_host_f16": (_i, _PLANES_HOST + (_vp,)),
    "lumahip_f16_narrow_probe_device": (_i, _PROBE),
    "lumahip_set_source_quantizer": (_i, _QUANTIZER),
    "lumahip_transcode_frames_device": (_i, _TWO_SETS + (_vp,)),
    "lumahip_transcode_frame_host": (_i, _TWO_SETS_HOST + (_fp,)),
    "lumahip_distortion_frames_device": (_i, _FRAMES + (_vp,)),
    "lumahip_distortion_frames_device_planar": (_i, _PLANAR + (_vp,)),
    "lumahip_distortion_frames_device_f16": (_i, _FRAMES + (_vp,)),
    "lumahip_distortion_frames_device_planar_f16": (_i, _PLANAR + (_vp,)),
    "lumahip_distortion_frame_host": (_i, _FRAME_HOST + (_vp,)),
    "lumahip_transcode_distortion_frames_device": (_i, _TWO_SETS + (_vp,)),
    "lumahip_transcode_distortion_frame_host": (_i, _TWO_SETS_HOST + (_vp,)),
    "lumahip_distortion_map_dims": (_i, _MAP_DIMS),
    "lumahip_distortion_map_frames_device": (_i, _FRAMES + (_u, _vp)),
    "lumahip_distortion_map_frames_device_planar": (_i, _PLANAR + (_u, _vp)),
    "lumahip_distortion_map_frames_device_f16": (_i, _FRAMES + (_u, _vp)),
    "lumahip_distortion_map_frames_device_planar_f16": (_i, _PLANAR + (_u, _vp)),
    "lumahip_distortion_map_frame_host": (_i, _FRAME_HOST + (_u, _vp, _sz)),
    "lumahip_transcode_distortion_map_frames_device": (_i, _TWO_SETS + (_u, _vp)),
    "lumahip_transcode_distortion_map_frame_host": (_i, _TWO_SETS_HOST + (_u, _vp, _sz)),
    "lumahip_moments_map_dims": (_i, _MAP_DIMS),
    "lumahip_moments_map_frames_device": (_i, _FRAMES + (_u, _vp)),
    "lumahip_moments_map_frames_device_planar": (_i, _PLANAR + (_u, _vp)),
    "lumahip_moments_map_frames_device_f16": (_i, _FRAMES + (_u, _vp)),
    "lumahip_moments_map_frames_device_planar_f16": (_i, _PLANAR + (_u, _vp)),
    "lumahip_moments_map_frame_host": (_i, _FRAME_HOST + (_u, _vp, _sz)),
    "lumahip_time_launches": (_i, (_vp, _i, _i) + _FRAMES[1:] + (_fp,)),
    "lumahip_probe_encode_traffic_device": (_i, _FRAMES[:6] + (_p3, _i3, _s3, _i, _fp)),
    "lumahip_powf_probe_device": (_i, _PROBE + (_f, _i)),
    "lumahip_quantize_probe_device": (_i, _PROBE + (_i,)),
    "lumahip_ycbcr_luma_probe_device": (_i, _PROBE + (_i,)),
    "lumahip_host_register": (_i, (_vp, _vp, _sz)),
    "lumahip_host_unregister": (_i, (_vp, _vp)),
    "lumahip_malloc": (_i, (_vp, _p3, _sz)),
    "lumahip_free": (_i, (_vp, _vp)),
    "lumahip_memcpy_h2d": (_i, (_vp, _vp, _vp, _sz)),
    "lumahip_memcpy_d2h": (_i, (_vp, _vp, _vp, _sz)),
}
SYMBOLS = tuple(_ABI)

# The calls include/lumahip_measure.h declares (measuring calls added after lumahip.h's list was closed), bound like _ABI's:
# tests/test_transcode_moments_map_host.py holds this table against that header.
_ABI_MEASURE = {
    "lumahip_transcode_moments_map_frames_device": (_i, _TWO_SETS + (_u, _vp)),
    "lumahip_transcode_moments_map_frame_host": (_i, _TWO_SETS_HOST + (_u, _vp, _sz)),
}
MEASURE_SYMBOLS = tuple(_ABI_MEASURE)

# The calls include/lumahip_compare.h declares, bound like _ABI's.  That header is the open one -- later additions to the library go
# there and here --, and tests/test_planes_measure_host.py holds this table and the header to each other whatever their number.
_TWO_PLANE_SETS = (_vp, _p3, _i3, _s3, _u, _u, _u, _p3, _i3, _s3, _i)          # A's triplets, nframes, w, h, B's triplets, profile
_TWO_PLANE_SETS_HOST = (_vp, _p3, _i3, _u, _u, _p3, _i3, _i)                   # A's planes, strides, w, h, B's planes, strides, profile
_LIGHT_FRAMES = (_vp, _vp, _sz, _u, _u, _u, _f, _vp)                            # frames, frame_stride, nframes, w, h, scale, out
_ABI_COMPARE = {
    "lumahip_planes_distortion_frames_device": (_i, _TWO_PLANE_SETS + (_vp,)),
    "lumahip_planes_distortion_map_frames_device": (_i, _TWO_PLANE_SETS + (_u, _vp)),
    "lumahip_planes_moments_map_frames_device": (_i, _TWO_PLANE_SETS + (_u, _vp)),
    "lumahip_planes_distortion_frame_host": (_i, _TWO_PLANE_SETS_HOST + (_vp,)),
    "lumahip_planes_distortion_map_frame_host": (_i, _TWO_PLANE_SETS_HOST + (_u, _vp, _sz)),
    "lumahip_planes_moments_map_frame_host": (_i, _TWO_PLANE_SETS_HOST + (_u, _vp, _sz)),
    "lumahip_light_level_frames_device": (_i, _LIGHT_FRAMES),
    "lumahip_light_level_frames_device_planar": (_i, (_vp, _p3) + _LIGHT_FRAMES[2:]),
    "lumahip_light_level_frames_device_f16": (_i, _LIGHT_FRAMES),
    "lumahip_light_level_frames_device_planar_f16": (_i, (_vp, _p3) + _LIGHT_FRAMES[2:]),
    "lumahip_planes_light_level_frames_device": (_i, _PLANES + (_f, _vp)),
    "lumahip_light_level_frame_host": (_i, (_vp, _vp, _u, _u, _f, _vp)),
    "lumahip_planes_light_level_frame_host": (_i, _PLANES_HOST + (_f, _vp)),
    "lumahip_transcode_half_frames_device": (_i, _TWO_SETS + (_vp,)),
    "lumahip_transcode_half_frame_host": (_i, _TWO_SETS_HOST),
}
COMPARE_SYMBOLS = tuple(_ABI_COMPARE)

# The calls include/lumahip_ladder.h declares (a half-size rendition scored against the source's half-resolution transcode), bound
# like _ABI's; tests/test_transcode_half_distortion_host.py holds this table and the header to each other.
_ABI_LADDER = {
    "lumahip_transcode_half_distortion_frames_device": (_i, _TWO_SETS + (_vp,)),
    "lumahip_transcode_half_distortion_map_frames_device": (_i, _TWO_SETS + (_u, _vp)),
    "lumahip_transcode_half_distortion_frame_host": (_i, _TWO_SETS_HOST + (_vp,)),
    "lumahip_transcode_half_distortion_map_frame_host": (_i, _TWO_SETS_HOST + (_u, _vp, _sz)),
}
LADDER_SYMBOLS = tuple(_ABI_LADDER)

# The calls include/lumahip_rungs.h declares (the lower rungs of a ladder made from the source planes: the quarter-resolution
# transcode), bound like _ABI's; tests/test_transcode_quarter_host.py holds this table and the header to each other.
_ABI_RUNGS = {
    "lumahip_transcode_quarter_frames_device": (_i, _TWO_SETS + (_vp,)),
    "lumahip_transcode_quarter_frame_host": (_i, _TWO_SETS_HOST),
}
RUNGS_SYMBOLS = tuple(_ABI_RUNGS)


class LumaHipError(RuntimeError):
    """Counterpart of the reference's LumaException (include/luma/luma_exception.h:53-71)."""

    def __init__(self, code, msg):
        super().__init__("lumahip error %d: %s" % (code, msg))
        self.code = code


def library_path() -> str:
    return _LIB_PATH


def build_library(force: bool = False, nofastdiv: bool = False) -> str:
    """Compile every HIP source for gfx950 into lumahdrv_amd/lib/liblumahip.so (hipcc cross-compiles
    without a GPU).  nofastdiv: additionally the -DLH_NO_FAST_DIV comparison build of the C ABI library
    (lumahdrv_amd/lib_nofastdiv/liblumahip.so) that tests/test_gpu_parity.py loads through LUMAHIP_LIB."""
    cmd = ["make", "-s", "-j", str(min(8, os.cpu_count() or 1)), "-C", os.path.join(HERE, "csrc")]
    if force:
        subprocess.run(cmd + ["clean"], check=True)
    subprocess.run(cmd, check=True)
    if nofastdiv:
        out = os.path.join(HERE, "lib_nofastdiv")
        subprocess.run(cmd + ["OUT=" + out, "EXTRA=-DLH_NO_FAST_DIV", os.path.join(out, "liblumahip.so")], check=True)
    return os.path.join(HERE, "lib", "liblumahip.so")


# device code + launch geometry + compiler flags (NOT the host plumbing: lumahip_core / _host / _pool / _multi, lumahip_internal.hpp)
KERNEL_SOURCES = ("luma_device.hpp", "luma_kernels.hpp", "pow_glibc.hpp", "lumahip_launch.hip", "lumahip_encode.hip",
                  "lumahip_decode.hip", "lumahip_misc.hip", "lut_index.cpp", "lut_index.hpp", "flags.mk", "f16_narrow.hpp",
                  "lumahip_encode_f16.hip", "lumahip_decode_f16.hip", "lumahip_pick.hpp", "lumahip_transcode.hip", "lumahip_distortion.hip", "lumahip_distortion_f16.hip",
                  "lumahip_transcode_distortion.hip", "lumahip_distortion_map.hip", "lumahip_distortion_map_f16.hip",
                  "lumahip_transcode_distortion_map.hip", "lumahip_moments_map.hip", "lumahip_moments_map_f16.hip",
                  "lumahip_transcode_moments_map.hip", "lumahip_planes_measure.hip", "lumahip_light_level.hip",
                  "lumahip_transcode_half.hip", "lumahip_transcode_half_distortion.hip", "lumahip_transcode_half_distortion_map.hip",
                  "lumahip_transcode_quarter.hip")


def kernel_source_sha() -> str:
    """short SHA-1 over the device sources; profiles/*.json captured by rocprofv3 carry it so that bench.py never
    reports a counter-derived figure measured on different kernels"""
    import hashlib
    hsh = hashlib.sha1()
    for f in KERNEL_SOURCES:
        with open(os.path.join(HERE, "csrc", f), "rb") as fh:
            hsh.update(fh.read())
    return hsh.hexdigest()[:12]


_lib = None


def lib():
    """Load liblumahip.so.  torch, when installed, is imported FIRST: its wheel bundles its own
    libamdhip64.so (same SONAME as /opt/rocm's), and the process must end up with exactly one HIP
    runtime so that device pointers from torch tensors are valid in our launches."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise LumaHipError(ERR_STATE, "%s not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                      "(there is no CPU fallback)" % _LIB_PATH)
    if "torch" not in sys.modules and not os.environ.get("LUMAHIP_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in list(_ABI.items()) + list(_ABI_MEASURE.items()) + list(_ABI_COMPARE.items()) + list(_ABI_LADDER.items()) + \
            list(_ABI_RUNGS.items()):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = L
    return L


POOL_FLOAT, POOL_Y, POOL_UV, POOL_STRIPED, POOL_ROTATING = range(5)


def shard_range(nframes: int, shard: int, nshards: int) -> range:
    """lumahip_shard_range: the contiguous block of frames shard `shard` of `nshards` owns"""
    a, b = C.c_uint(0), C.c_uint(0)
    rc = lib().lumahip_shard_range(nframes, shard, nshards, C.byref(a), C.byref(b))
    if rc != OK:
        raise LumaHipError(rc, "lumahip_shard_range(%d, %d, %d)" % (nframes, shard, nshards))
    return range(a.value, a.value + b.value)


def pool_find_groups(n: int, probe):
    """host-only: the chunk pool's grouping step (lumahip_pool_find_groups) with a Python measurement probe(i, r) -> time of
    reading chunk i while writing chunk r.  Returns (groups or None when there is no contrast, fastest pair time, probes)."""
    g = np.full(n, -1, dtype=np.int32)
    ng, npr, fast = C.c_int(0), C.c_int(0), C.c_double(0.0)
    cb = PROBE_FN(lambda i, r, _u: float(probe(i, r)))
    rc = lib().lumahip_pool_find_groups(n, cb, None, g.ctypes.data, C.byref(ng), C.byref(fast), C.byref(npr))
    if rc != OK:
        raise LumaHipError(rc, "lumahip_pool_find_groups failed")
    groups = None if ng.value == 0 else [[int(i) for i in np.nonzero(g == k)[0]] for k in range(ng.value)]
    return groups, fast.value, npr.value


def plane_geometry(w: int, h: int, profile: int, align: int = 32):
    """(widths, heights, strides-in-bytes, bytes-per-sample) of the Y/U/V planes as
    vpx_img_alloc(fmt(profile), w, h, 32) lays them out (src/luma_encoder.cpp:121-128)."""
    sub = profile in (0, 2)
    bps = 2 if profile > 1 else 1
    s0 = (w + align - 1) // align * align * bps
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub else (w, h)
    s1 = s0 // 2 if sub else s0
    return (w, cw, cw), (h, ch, ch), (s0, s1, s1), bps


def build_lut(ptf: int, bitdepth: int, max_lum: float = 1e4, min_lum: float = 0.005) -> np.ndarray:
    """The transfer-function table of LumaQuantizer::setQuantizer, built by the library's host code with the
    host libm exactly as the reference does (no GPU needed)."""
    out = np.empty(1 << bitdepth, dtype=np.float32)
    rc = lib().lumahip_build_lut(ptf, bitdepth, max_lum, min_lum, out.ctypes.data, out.size)
    if rc != OK:
        raise LumaHipError(rc, "lumahip_build_lut(ptf=%d, bitdepth=%d) failed" % (ptf, bitdepth))
    return out


def _index_records(name, lut, mid, ninfo, shape):
    """the index calls' two passes: ask for the size (records NULL), then, when the table qualifies (info[0]), fetch the records
    into an array of shape(info).  Returns (info, rec or None)"""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    fn, info, rec = getattr(lib(), name), (C.c_int * ninfo)(), None
    while True:
        rc = fn(lut.ctypes.data, lut.size, *mid, info, None if rec is None else rec.ctypes.data, 0 if rec is None else rec.size)
        if rc != OK:
            raise LumaHipError(rc, name + " failed")
        if rec is not None or not info[0]:
            return info, rec
        rec = np.zeros(shape(info), dtype=np.uint32)


def _thresh_records(name, lut, *mid):
    info, rec = _index_records(name, lut, mid, 5, lambda info: info[4])
    return dict(ok=bool(info[0]), mant_bits=info[1], shift=info[2], kmin=info[3], nbuckets=info[4], rec=rec)


def thresh_index(lut: np.ndarray):
    """host-only: the threshold records of a table (include/lumahip.h lumahip_thresh_index_host); no GPU needed"""
    return _thresh_records("lumahip_thresh_index_host", lut)


def lin_index(lut: np.ndarray):
    """host-only: the value-keyed records of an evenly spaced table (include/lumahip.h lumahip_lin_index_host); no GPU needed.
    dict(ok, nbuckets, kscale (np.float32), rec (nbuckets x 2 uint32: bits(T) - 1, start) | None)"""
    info, rec = _index_records("lumahip_lin_index_host", lut, (), 3, lambda info: (info[1], 2))
    return dict(ok=bool(info[0]), nbuckets=info[1], kscale=np.array([info[2]], dtype=np.int32).view(np.float32)[0], rec=rec)


def lin_lookup(ix, v: np.ndarray) -> np.ndarray:
    """numpy evaluation of value-keyed records, as the kernels evaluate them (luma_device.hpp quantize_linkey)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        p = np.fmin(v * np.float32(ix["kscale"]), np.float32(ix["nbuckets"] - 1))      # fmin: a NaN product -> the top bucket
        k = np.where(p > 0, p, np.float32(0)).astype(np.int64)                            # truncation; negatives and -0 -> 0
    rec = ix["rec"]
    return rec[k, 1].astype(np.int64) + (v.view(np.int32) > rec[k, 0].view(np.int32)).astype(np.int64)


def ycbcr_luma_index(lut: np.ndarray, max_lum: float):
    """host-only: the composite luma -> luminance code records of the YCbCr encode kernels (same dict as thresh_index)"""
    return _thresh_records("lumahip_ycbcr_luma_index_host", lut, max_lum)


def ycbcr_ytab(lut: np.ndarray, max_lum: float) -> np.ndarray:
    """host-only: the per-stream y table of the YCbCr decode kernels"""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    out = np.empty_like(lut)
    rc = lib().lumahip_ycbcr_ytab_host(lut.ctypes.data, lut.size, max_lum, out.ctypes.data)
    if rc != OK:
        raise LumaHipError(rc, "lumahip_ycbcr_ytab_host failed")
    return out


def quantize_value(lut: np.ndarray, cs: int, bitdepth_c: int, val: float, ch: int = 0, dequantize: bool = False) -> float:
    """host-only: LumaQuantizer::quantize / dequantize for one value (include/lumahip.h lumahip_quantize_value_host)"""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    out = C.c_float(0)
    fn = lib().lumahip_dequantize_value_host if dequantize else lib().lumahip_quantize_value_host
    rc = fn(lut.ctypes.data, lut.size, cs, bitdepth_c, val, ch, C.byref(out))
    if rc != OK:
        raise LumaHipError(rc, "lumahip_(de)quantize_value_host: bad argument")
    return float(out.value)


def numa_plan(sysfs_root, pci_bus_id: str, allowed: str = ""):
    """host-only: (node, [cpus]) the library would place the host side of a context on for the GPU at `pci_bus_id`"""
    node, n = C.c_int(-1), C.c_int(0)
    cpus = (C.c_int * 4096)()
    rc = lib().lumahip_numa_plan_host(sysfs_root.encode() if sysfs_root else None, pci_bus_id.encode(), allowed.encode(), C.byref(node), cpus,
                                      4096, C.byref(n))
    if rc != OK:
        raise LumaHipError(rc, "lumahip_numa_plan_host: bad argument")
    return node.value, list(cpus[:min(n.value, 4096)])


HALF_TABLE_LEN = 0x7C00 + 1


def ycbcr_half_table(sc: float, max_lum: float):
    """host-only: the half-input table of the YCbCr encode kernels for (preScaling, maxLum), or None when the pair does not qualify"""
    out = np.empty(HALF_TABLE_LEN, dtype=np.float32)
    rc = lib().lumahip_ycbcr_half_table_host(sc, max_lum, out.ctypes.data, out.size)
    if rc == ERR_UNSUPPORTED:
        return None
    if rc != OK:
        raise LumaHipError(rc, "lumahip_ycbcr_half_table_host failed")
    return out


def thresh_lookup(ix, v: np.ndarray) -> np.ndarray:
    """numpy evaluation of the record table exactly as the kernels do it (sign-set NaNs excluded by the caller)"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.int32)
    k = np.clip(b >> ix["shift"], ix["kmin"], ix["kmin"] + ix["nbuckets"] - 1) - ix["kmin"]
    low = b.view(np.uint32) & np.uint32((1 << ix["shift"]) - 1)
    return ((ix["rec"][k] + low) >> np.uint32(ix["shift"])).astype(np.int64)


def code_psnr(sse, nsamples, peak) -> float:
    """PSNR in the code domain from a sum of squared code differences (Context.distortion_*): 10 log10(peak^2 * nsamples / sse),
    `peak` the largest code of the plane (2**bitdepth - 1); infinity for identical planes"""
    if nsamples <= 0 or peak <= 0:
        raise ValueError("code_psnr needs nsamples > 0 and peak > 0")
    if int(sse) == 0:
        return float("inf")
    return 10.0 * float(np.log10(float(peak) * float(peak) * float(nsamples) / float(sse)))


LIGHT_WORDS = 8   # include/lumahip_compare.h LUMAHIP_LIGHT_WORDS


def content_light_level(words, w: int, h: int):
    """(MaxCLL, MaxFALL) in cd/m2 of a stream from the eight words per frame of the light-level calls (run with scale = the stream's
    preScaling): words is (nframes, 8), or one frame's 8.  MaxCLL = ceil(max_f words[f][1] / 256), MaxFALL = ceil(max_f words[f][0] /
    (256 w h)) -- every pixel is in the divisor, as CTA-861.3 averages over the whole picture -- both capped at 65535, the largest value
    the HDR10 side data holds.  Python integers throughout."""
    rows = np.asarray(words, dtype=np.uint64).reshape(-1, LIGHT_WORDS)
    if rows.shape[0] == 0:
        return 0, 0
    peak = max(int(r[1]) for r in rows)
    total = max(int(r[0]) for r in rows)
    den = 256 * int(w) * int(h)
    return min(65535, -(-peak // 256)), min(65535, -(-total // den))


def distortion_map_dims(w: int, h: int, block: int):
    """(nbx, nby): blocks per frame of a distortion map, ceil(w / block) x ceil(h / block); block is 16, 32 or 64"""
    nbx, nby = C.c_uint(0), C.c_uint(0)
    rc = lib().lumahip_distortion_map_dims(w, h, block, C.byref(nbx), C.byref(nby))
    if rc != 0:
        raise LumaHipError(rc, "distortion map: block must be 16, 32 or 64 (got %r)" % (block,))
    return int(nbx.value), int(nby.value)


def block_sample_counts(w: int, h: int, profile: int, block: int) -> np.ndarray:
    """(nby, nbx, 3) int64: how many samples of each plane a block of a distortion map covers -- block x block luma pixels cut at
    the frame's edges, and on the 4:2:0 chroma planes (profiles 0 and 2) the samples co-sited with them.  code_psnr(map[by, bx, p, 0],
    counts[by, bx, p], peak) is the block's PSNR"""
    return _block_sample_counts(w, h, profile, block, *distortion_map_dims(w, h, block))


def _block_sample_counts(w, h, profile, block, nbx, nby) -> np.ndarray:
    out = np.empty((nby, nbx, 3), dtype=np.int64)
    for p in range(3):
        sub = p > 0 and profile in (0, 2)
        pw, ph, b = (w // 2, h // 2, block // 2) if sub else (w, h, block)
        nx = np.minimum(pw, (np.arange(nbx) + 1) * b) - np.arange(nbx) * b
        ny = np.minimum(ph, (np.arange(nby) + 1) * b) - np.arange(nby) * b
        out[:, :, p] = ny[:, None] * nx[None, :]
    return out


def moments_map_dims(w: int, h: int, block: int):
    """(nbx, nby): blocks per frame of a moments map, ceil(w / block) x ceil(h / block); block is 8, 16, 32 or 64"""
    nbx, nby = C.c_uint(0), C.c_uint(0)
    rc = lib().lumahip_moments_map_dims(w, h, block, C.byref(nbx), C.byref(nby))
    if rc != 0:
        raise LumaHipError(rc, "moments map: block must be 8, 16, 32 or 64 (got %r)" % (block,))
    return int(nbx.value), int(nby.value)


def moments_sample_counts(w: int, h: int, profile: int, block: int) -> np.ndarray:
    """(nby, nbx, 3) int64: the samples N behind each entry of a moments map -- block_sample_counts with blocks of 8 allowed"""
    return _block_sample_counts(w, h, profile, block, *moments_map_dims(w, h, block))


def code_ssim(moments, counts, peak, k1=0.01, k2=0.03) -> np.ndarray:
    """Structural similarity in the code domain from the five sums of a moments map (Context.moments_map_*): moments (..., 5) =
    {Se, Sg, See, Sgg, Seg}, counts (...) = the samples N behind them, `peak` the largest code of the plane.  The usual SSIM with
    population variances and C1 = (k1 peak)^2, C2 = (k2 peak)^2, multiplied through by N^4:
        (2 Se Sg + N^2 C1) (2 (N Seg - Se Sg) + N^2 C2) / ((Se^2 + Sg^2 + N^2 C1) ((N See - Se^2) + (N Sgg - Sg^2) + N^2 C2))
    The four integer parts are formed exactly in int64 (N <= 2^12, sums <= 2^28, second moments <= 2^44: every product is below
    2^57), so the cancellation in N See - Se^2 never happens in floating point and identical planes give exactly 1.0.  Returns a
    float64 array (...)."""
    m = np.asarray(moments)
    if m.shape[-1:] != (5,):
        raise ValueError("code_ssim needs moments of shape (..., 5)")
    m = m.astype(np.int64)
    n = np.asarray(counts).astype(np.int64)
    if n.shape != m.shape[:-1]:
        raise ValueError("code_ssim needs counts of the moments' shape without its last axis")
    if peak <= 0 or np.any(n <= 0) or np.any(n > 4096):
        raise ValueError("code_ssim needs peak > 0 and 0 < counts <= 4096")
    se, sg, see, sgg, seg = (m[..., k] for k in range(5))
    mean_num = 2 * se * sg
    mean_den = se * se + sg * sg
    cov_num = 2 * (n * seg - se * sg)
    var_den = (n * see - se * se) + (n * sgg - sg * sg)
    n2 = (n * n).astype(np.float64)
    c1 = n2 * (float(k1) * float(peak)) ** 2
    c2 = n2 * (float(k2) * float(peak)) ** 2
    return ((mean_num + c1) * (cov_num + c2)) / ((mean_den + c1) * (var_den + c2))


def _arr3(ctype, vals):
    return (ctype * 3)(*vals)


class Context:
    """One GPU, one stream, one quantizer configuration (lumahip_ctx)."""

    def __init__(self, device: int = -1):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.lumahip_create(C.byref(h), device)
        if rc != OK:
            raise LumaHipError(rc, "lumahip_create failed: no usable HIP device (there is no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.lumahip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise LumaHipError(rc, self.L.lumahip_last_error(self.h).decode())

    # ---- one body per argument shape; `tail` is whatever the C function takes after the shared run
    def _frame_fed(self, fn, frames, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides, plane_frame_strides, *tail):
        """the frame-fed device calls; frames: a packed pointer, or _arr3 of three colour-plane pointers for the _planar forms"""
        self._chk(fn(self.h, frames, frame_stride, nframes, w, h, sc, profile, _arr3(C.c_void_p, plane_ptrs), _arr3(C.c_int, strides),
                     _arr3(C.c_size_t, plane_frame_strides), *tail))

    def _plane_fed(self, fn, plane_ptrs, strides, plane_frame_strides, *tail):
        """the plane-fed device calls (the decode forms)"""
        self._chk(fn(self.h, _arr3(C.c_void_p, plane_ptrs), _arr3(C.c_int, strides), _arr3(C.c_size_t, plane_frame_strides), *tail))

    def _two_sets(self, fn, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h, dst_plane_ptrs,
                  dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, *tail):
        """the device calls over source planes and target planes (transcode and its measuring forms)"""
        self._chk(fn(self.h, _arr3(C.c_void_p, src_plane_ptrs), _arr3(C.c_int, src_strides), _arr3(C.c_size_t, src_plane_frame_strides),
                     src_profile, src_sc, nframes, w, h, _arr3(C.c_void_p, dst_plane_ptrs), _arr3(C.c_int, dst_strides),
                     _arr3(C.c_size_t, dst_plane_frame_strides), dst_profile, dst_sc, *tail))

    def _measured(self, fn, args, w, h, words, dims, block):
        """the measuring host forms: fn(ctx, *args, tail) into a (3, words) uint64 array of the frame, or with dims into a
        (nby, nbx, 3, words) one per block"""
        if dims is None:
            out = np.zeros((3, words), dtype=np.uint64)
            self._chk(fn(self.h, *args, out.ctypes.data))
        else:
            nbx, nby = dims(w, h, block)
            out = np.zeros((nby, nbx, 3, words), dtype=np.uint64)
            self._chk(fn(self.h, *args, block, out.ctypes.data, out.size))
        return out

    def _measure_frame(self, fn, rgb, planes, strides, sc, profile, words, dims=None, block=None):
        """the frame-fed measuring host forms"""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        _, h, w = rgb.shape
        planes = [np.ascontiguousarray(p) for p in planes]
        args = (rgb.ctypes.data, w, h, sc, profile, _arr3(C.c_void_p, [p.ctypes.data for p in planes]), _arr3(C.c_int, strides))
        return self._measured(fn, args, w, h, words, dims, block)

    def _measure_planes(self, fn, planes, strides, w, h, given_planes, given_strides, src_sc, src_profile, dst_sc, dst_profile, dims=None,
                        block=None, words=4, scale=1):
        """the plane-fed measuring host forms; scale 2: w x h is the source's size, the given planes and the words are of (w/2) x (h/2)"""
        planes = [np.ascontiguousarray(p) for p in planes]
        given_planes = [np.ascontiguousarray(p) for p in given_planes]
        args = (_arr3(C.c_void_p, [p.ctypes.data for p in planes]), _arr3(C.c_int, strides), src_profile, src_sc, w, h,
                _arr3(C.c_void_p, [p.ctypes.data for p in given_planes]), _arr3(C.c_int, given_strides), dst_profile, dst_sc)
        return self._measured(fn, args, w // scale, h // scale, words, dims, block)

    def _measure_two_sets(self, fn, a_planes, a_strides, w, h, b_planes, b_strides, profile, words, dims=None, block=None):
        """the plane-to-plane measuring host forms"""
        a_planes = [np.ascontiguousarray(p) for p in a_planes]
        b_planes = [np.ascontiguousarray(p) for p in b_planes]
        args = (_arr3(C.c_void_p, [p.ctypes.data for p in a_planes]), _arr3(C.c_int, a_strides), w, h,
                _arr3(C.c_void_p, [p.ctypes.data for p in b_planes]), _arr3(C.c_int, b_strides), profile)
        return self._measured(fn, args, w, h, words, dims, block)

    def _two_plane_sets(self, fn, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h, b_plane_ptrs, b_strides,
                        b_plane_frame_strides, profile, *tail):
        """the plane-to-plane measuring device calls"""
        self._chk(fn(self.h, _arr3(C.c_void_p, a_plane_ptrs), _arr3(C.c_int, a_strides), _arr3(C.c_size_t, a_plane_frame_strides), nframes,
                     w, h, _arr3(C.c_void_p, b_plane_ptrs), _arr3(C.c_int, b_strides), _arr3(C.c_size_t, b_plane_frame_strides), profile,
                     *tail))

    # ---- configuration
    def set_stream(self, hip_stream: int | None):
        """hip_stream: a hipStream_t handle (0 = the default stream, as torch's default stream reports);
        None = back to the context's own stream"""
        if hip_stream is None:
            self._chk(self.L.lumahip_reset_stream(self.h))
        else:
            self._chk(self.L.lumahip_set_stream(self.h, C.c_void_p(hip_stream)))

    def sync(self):
        self._chk(self.L.lumahip_sync(self.h))

    def tune(self, key: str, value: int):
        """measurement override (include/lumahip.h lumahip_tune); never changes a result"""
        self._chk(self.L.lumahip_tune(self.h, key.encode(), int(value)))

    def set_quantizer(self, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum, lut: np.ndarray):
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        self._chk(self.L.lumahip_set_quantizer(self.h, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum,
                                               lut.ctypes.data, lut.size))

    def set_source_quantizer(self, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum, lut: np.ndarray):
        """the stream the transcode calls READ (held beside the quantizer of set_quantizer, independent of it)"""
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        self._chk(self.L.lumahip_set_source_quantizer(self.h, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum,
                                                      lut.ctypes.data, lut.size))

    def quantizer_info(self):
        a = (C.c_int * 5)()
        self._chk(self.L.lumahip_quantizer_info(self.h, a))
        return dict(mode=a[0], mant_bits=a[1], buckets=a[2], shift=a[3], lds_bytes=a[4])

    def half_upload_info(self):
        a = (C.c_long * 3)()
        self._chk(self.L.lumahip_half_upload_info(self.h, a))
        return dict(half_frames=a[0], float_fallbacks=a[1], pause_left=a[2])

    def numa_info(self):
        a = (C.c_int * 3)()
        self._chk(self.L.lumahip_numa_info(self.h, a))
        return dict(node=a[0], cpus=a[1], first_cpu=a[2])

    def rb_table_info(self, sc: float):
        a = (C.c_int * 4)()
        self._chk(self.L.lumahip_rb_table_info(self.h, sc, a))
        return dict(used=bool(a[0]), bytes=a[1], table_launches=a[2], backoff_launches=a[3])

    def half_table_info(self, sc: float):
        a = (C.c_int * 6)()
        self._chk(self.L.lumahip_half_table_info(self.h, sc, a))
        return dict(used=bool(a[0]), lds_bytes=a[1], device_copies=a[2], entries=a[3], table_launches=a[4], backoff_launches=a[5])

    # ---- host entry points (numpy)
    def encode_frame(self, rgb: np.ndarray, sc=1.0, profile=2, align=32, want_transformed=False, strides=None):
        """rgb: (3,h,w) float32 (LumaFrame layout).  Returns (planes, strides, mean_lum[, transformed])."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        _, h, w = rgb.shape
        _, hs, st, _ = plane_geometry(w, h, profile, align)
        if strides is not None:
            st = tuple(strides)
        planes = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        mean = C.c_float(0)
        tr = np.empty_like(rgb) if want_transformed else None
        self._chk(self.L.lumahip_encode_frame_host(self.h, rgb.ctypes.data, w, h, sc, profile,
                                                   _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                   _arr3(C.c_int, st), C.byref(mean),
                                                   tr.ctypes.data if tr is not None else None))
        if want_transformed:
            return planes, st, float(mean.value), tr
        return planes, st, float(mean.value)

    def decode_frame(self, planes, strides, w, h, sc=1.0, profile=2) -> np.ndarray:
        planes = [np.ascontiguousarray(p) for p in planes]
        out = np.empty((3, h, w), dtype=np.float32)
        self._chk(self.L.lumahip_decode_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                   _arr3(C.c_int, strides), w, h, profile, sc, out.ctypes.data))
        return out

    def transcode_frame(self, planes, strides, w, h, src_sc=1.0, src_profile=2, dst_sc=1.0, dst_profile=2, align=32, dst_strides=None,
                        want_mean=True):
        """code planes under the source quantizer -> (planes, strides, mean_lum) under the quantizer, one fused launch; equal to
        decode_frame on a context with the source quantizer followed by encode_frame on this one"""
        planes = [np.ascontiguousarray(p) for p in planes]
        _, hs, st, _ = plane_geometry(w, h, dst_profile, align)
        if dst_strides is not None:
            st = tuple(dst_strides)
        out = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        mean = C.c_float(0)
        self._chk(self.L.lumahip_transcode_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]), _arr3(C.c_int, strides),
                                                      src_profile, src_sc, w, h, _arr3(C.c_void_p, [p.ctypes.data for p in out]),
                                                      _arr3(C.c_int, st), dst_profile, dst_sc, C.byref(mean) if want_mean else None))
        return out, st, (float(mean.value) if want_mean else None)

    def transcode_half_frame(self, planes, strides, w, h, src_sc=1.0, src_profile=2, dst_sc=1.0, dst_profile=2, align=32, dst_strides=None):
        """code planes of w x h under the source quantizer -> (planes, strides) of (w/2) x (h/2) under the quantizer, averaged 2x2
        in linear light, one fused launch; w and h multiples of 4"""
        planes = [np.ascontiguousarray(p) for p in planes]
        _, hs, st, _ = plane_geometry(w // 2, h // 2, dst_profile, align)
        if dst_strides is not None:
            st = tuple(dst_strides)
        out = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        self._chk(self.L.lumahip_transcode_half_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]), _arr3(C.c_int, strides),
                                                           src_profile, src_sc, w, h, _arr3(C.c_void_p, [p.ctypes.data for p in out]),
                                                           _arr3(C.c_int, st), dst_profile, dst_sc))
        return out, st

    def transcode_quarter_frame(self, planes, strides, w, h, src_sc=1.0, src_profile=2, dst_sc=1.0, dst_profile=2, align=32, dst_strides=None):
        """code planes of w x h under the source quantizer -> (planes, strides) of (w/4) x (h/4) under the quantizer, averaged 2x2
        in linear light twice with nothing quantized in between, one fused launch; w and h multiples of 8"""
        planes = [np.ascontiguousarray(p) for p in planes]
        _, hs, st, _ = plane_geometry(w // 4, h // 4, dst_profile, align)
        if dst_strides is not None:
            st = tuple(dst_strides)
        out = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        self._chk(self.L.lumahip_transcode_quarter_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]), _arr3(C.c_int, strides),
                                                              src_profile, src_sc, w, h, _arr3(C.c_void_p, [p.ctypes.data for p in out]),
                                                              _arr3(C.c_int, st), dst_profile, dst_sc))
        return out, st

    def distortion_frame(self, rgb: np.ndarray, planes, strides, sc=1.0, profile=2) -> np.ndarray:
        """rgb: (3,h,w) float32; planes: the given code planes as three (rows, stride) uint8 arrays.  Returns a (3, 4) uint64 array:
        per plane {sse, sad, max_abs, n_differ} of the planes encode_frame would write against the given ones"""
        return self._measure_frame(self.L.lumahip_distortion_frame_host, rgb, planes, strides, sc, profile, 4)

    def distortion_map_frame(self, rgb: np.ndarray, planes, strides, sc=1.0, profile=2, block=16) -> np.ndarray:
        """distortion_frame's words per block of block x block luma pixels (16, 32 or 64): a (nby, nbx, 3, 4) uint64 array, in one
        launch; block_sample_counts gives the samples behind each entry"""
        return self._measure_frame(self.L.lumahip_distortion_map_frame_host, rgb, planes, strides, sc, profile, 4, distortion_map_dims,
                                   block)

    def moments_map_frame(self, rgb: np.ndarray, planes, strides, sc=1.0, profile=2, block=8) -> np.ndarray:
        """per block of block x block luma pixels (8, 16, 32 or 64) and plane the five sums {Se, Sg, See, Sgg, Seg} of the frame's
        codes e and the given samples g: a (nby, nbx, 3, 5) uint64 array, in one launch; moments_sample_counts gives the samples
        behind each entry and code_ssim the structural similarity"""
        return self._measure_frame(self.L.lumahip_moments_map_frame_host, rgb, planes, strides, sc, profile, 5, moments_map_dims, block)

    def transcode_distortion_frame(self, planes, strides, w, h, given_planes, given_strides, src_sc=1.0, src_profile=2, dst_sc=1.0,
                                   dst_profile=2) -> np.ndarray:
        """planes: code planes under the source quantizer; given_planes: code planes in the target's format, three (rows, stride)
        uint8 arrays each.  Returns a (3, 4) uint64 array: per plane {sse, sad, max_abs, n_differ} of the planes transcode_frame
        would write against the given ones, in one fused launch"""
        return self._measure_planes(self.L.lumahip_transcode_distortion_frame_host, planes, strides, w, h, given_planes, given_strides,
                                    src_sc, src_profile, dst_sc, dst_profile)

    def transcode_distortion_map_frame(self, planes, strides, w, h, given_planes, given_strides, src_sc=1.0, src_profile=2, dst_sc=1.0,
                                       dst_profile=2, block=16) -> np.ndarray:
        """transcode_distortion_frame's words per block of block x block luma pixels (16, 32 or 64) of the target: a
        (nby, nbx, 3, 4) uint64 array, in one launch; block_sample_counts(w, h, dst_profile, block) gives the samples behind each entry"""
        return self._measure_planes(self.L.lumahip_transcode_distortion_map_frame_host, planes, strides, w, h, given_planes, given_strides,
                                    src_sc, src_profile, dst_sc, dst_profile, distortion_map_dims, block)

    def transcode_moments_map_frame(self, planes, strides, w, h, given_planes, given_strides, src_sc=1.0, src_profile=2, dst_sc=1.0,
                                    dst_profile=2, block=8) -> np.ndarray:
        """moments_map_frame's five sums per block of block x block luma pixels (8, 16, 32 or 64) of the target, with e the codes
        transcode_frame would write for the source planes: a (nby, nbx, 3, 5) uint64 array, in one launch.  moments_map_dims,
        moments_sample_counts(w, h, dst_profile, block) and code_ssim apply unchanged"""
        return self._measure_planes(self.L.lumahip_transcode_moments_map_frame_host, planes, strides, w, h, given_planes, given_strides,
                                    src_sc, src_profile, dst_sc, dst_profile, moments_map_dims, block, words=5)

    def transcode_half_distortion_frame(self, planes, strides, w, h, given_planes, given_strides, src_sc=1.0, src_profile=2, dst_sc=1.0,
                                        dst_profile=2) -> np.ndarray:
        """planes: code planes of w x h under the source quantizer; given_planes: code planes of (w/2) x (h/2) in the target's format.
        Returns a (3, 4) uint64 array: per plane {sse, sad, max_abs, n_differ} of the planes transcode_half_frame would write against
        the given ones, in one fused launch; code_psnr applies unchanged"""
        return self._measure_planes(self.L.lumahip_transcode_half_distortion_frame_host, planes, strides, w, h, given_planes, given_strides,
                                    src_sc, src_profile, dst_sc, dst_profile, scale=2)

    def transcode_half_distortion_map_frame(self, planes, strides, w, h, given_planes, given_strides, src_sc=1.0, src_profile=2, dst_sc=1.0,
                                            dst_profile=2, block=16) -> np.ndarray:
        """transcode_half_distortion_frame's words per block of block x block luma pixels (16, 32 or 64) of the half-size target: a
        (nby, nbx, 3, 4) uint64 array with distortion_map_dims(w // 2, h // 2, block), in one launch"""
        return self._measure_planes(self.L.lumahip_transcode_half_distortion_map_frame_host, planes, strides, w, h, given_planes,
                                    given_strides, src_sc, src_profile, dst_sc, dst_profile, distortion_map_dims, block, scale=2)

    def planes_distortion_frame(self, a_planes, a_strides, w, h, b_planes, b_strides, profile=2) -> np.ndarray:
        """two sets of code planes of one profile, three (rows, stride) uint8 arrays each, compared as they are (no quantizer
        needed): a (3, 4) uint64 array, per plane {sse, sad, max_abs, n_differ} of A's samples e against B's samples g"""
        return self._measure_two_sets(self.L.lumahip_planes_distortion_frame_host, a_planes, a_strides, w, h, b_planes, b_strides, profile, 4)

    def planes_distortion_map_frame(self, a_planes, a_strides, w, h, b_planes, b_strides, profile=2, block=16) -> np.ndarray:
        """planes_distortion_frame's words per block of block x block luma pixels (16, 32 or 64): a (nby, nbx, 3, 4) uint64 array, in
        one launch; block_sample_counts gives the samples behind each entry"""
        return self._measure_two_sets(self.L.lumahip_planes_distortion_map_frame_host, a_planes, a_strides, w, h, b_planes, b_strides,
                                      profile, 4, distortion_map_dims, block)

    def planes_moments_map_frame(self, a_planes, a_strides, w, h, b_planes, b_strides, profile=2, block=8) -> np.ndarray:
        """per block of block x block luma pixels (8, 16, 32 or 64) and plane the five sums {Se, Sg, See, Sgg, Seg} of A's samples e
        and B's samples g: a (nby, nbx, 3, 5) uint64 array, in one launch; moments_map_dims, moments_sample_counts and code_ssim apply"""
        return self._measure_two_sets(self.L.lumahip_planes_moments_map_frame_host, a_planes, a_strides, w, h, b_planes, b_strides, profile,
                                      5, moments_map_dims, block)

    def light_level_frame(self, rgb: np.ndarray, scale=1.0) -> np.ndarray:
        """rgb: (3,h,w) float32.  Returns the frame's eight uint64 words {sum q(m), max q(m), over, NaN; the same of y}, m = max(R, G, B)
        and y the luminance after `* scale`, in units of 1/256 (include/lumahip_compare.h); content_light_level folds them.  No
        quantizer needed"""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        _, h, w = rgb.shape
        out = np.zeros(LIGHT_WORDS, dtype=np.uint64)
        self._chk(self.L.lumahip_light_level_frame_host(self.h, rgb.ctypes.data, w, h, scale, out.ctypes.data))
        return out

    def planes_light_level_frame(self, planes, strides, w, h, sc=1.0, profile=2, scale=1.0) -> np.ndarray:
        """light_level_frame of the frame decode_frame(planes, strides, w, h, sc, profile) would return, in one launch and without
        that frame: eight uint64 words"""
        planes = [np.ascontiguousarray(p) for p in planes]
        out = np.zeros(LIGHT_WORDS, dtype=np.uint64)
        self._chk(self.L.lumahip_planes_light_level_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                               _arr3(C.c_int, strides), w, h, profile, sc, scale, out.ctypes.data))
        return out

    def encode_frame_f16(self, rgb: np.ndarray, sc=1.0, profile=2, align=32, strides=None):
        """rgb: (3,h,w) np.float16 (LumaFrame layout of halves; 6 B per pixel cross to the device).  Returns (planes, strides,
        mean_lum), equal to encode_frame of the same frame widened to float32."""
        if np.asarray(rgb).dtype != np.float16:
            raise LumaHipError(ERR_ARG, "encode_frame_f16 takes np.float16 frames")
        rgb = np.ascontiguousarray(rgb)
        _, h, w = rgb.shape
        _, hs, st, _ = plane_geometry(w, h, profile, align)
        if strides is not None:
            st = tuple(strides)
        planes = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        mean = C.c_float(0)
        self._chk(self.L.lumahip_encode_frame_host_f16(self.h, rgb.ctypes.data, w, h, sc, profile,
                                                       _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                       _arr3(C.c_int, st), C.byref(mean)))
        return planes, st, float(mean.value)

    def decode_frame_f16(self, planes, strides, w, h, sc=1.0, profile=2) -> np.ndarray:
        """-> (3,h,w) np.float16: the decoded frame narrowed as ExrInterface::floatToHalf does (6 B per pixel come back)"""
        planes = [np.ascontiguousarray(p) for p in planes]
        out = np.empty((3, h, w), dtype=np.float16)
        self._chk(self.L.lumahip_decode_frame_host_f16(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                       _arr3(C.c_int, strides), w, h, profile, sc, out.ctypes.data))
        return out

    def encode_frames(self, frames, sc=1.0, profile=2, align=32):
        """pipelined batch form of encode_frame: frames = list of (3,h,w) float32 arrays.  Returns
        (list of plane triplets, strides, list of mean luminances)."""
        frames = [np.ascontiguousarray(f, dtype=np.float32) for f in frames]
        n = len(frames)
        _, h, w = frames[0].shape
        _, hs, st, _ = plane_geometry(w, h, profile, align)
        planes = [[np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)] for _ in range(n)]
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        pp = (C.c_void_p * (3 * n))(*[pl.ctypes.data for tri in planes for pl in tri])
        means = (C.c_float * n)()
        self._chk(self.L.lumahip_encode_frames_host(self.h, fp, n, w, h, sc, profile, pp, _arr3(C.c_int, st), means))
        return planes, st, [float(m) for m in means]

    def decode_frames(self, planes_list, strides, w, h, sc=1.0, profile=2):
        n = len(planes_list)
        planes_list = [[np.ascontiguousarray(p) for p in tri] for tri in planes_list]
        outs = [np.empty((3, h, w), dtype=np.float32) for _ in range(n)]
        pp = (C.c_void_p * (3 * n))(*[pl.ctypes.data for tri in planes_list for pl in tri])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        self._chk(self.L.lumahip_decode_frames_host(self.h, pp, _arr3(C.c_int, strides), n, w, h, profile, sc, op))
        return outs

    def pack_frame(self, transformed: np.ndarray, profile=2, align=32):
        """LumaEncoder::setChannels on its own: quantize + pack an already colour-transformed frame"""
        t = np.ascontiguousarray(transformed, dtype=np.float32)
        _, h, w = t.shape
        _, hs, st, _ = plane_geometry(w, h, profile, align)
        planes = [np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)]
        mean = C.c_float(0)
        self._chk(self.L.lumahip_pack_frame_host(self.h, t.ctypes.data, w, h, profile,
                                                 _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                 _arr3(C.c_int, st), C.byref(mean)))
        return planes, st, float(mean.value)

    def unpack_frame(self, planes, strides, w, h, profile=2) -> np.ndarray:
        """LumaDecoder::getVpxChannels on its own: unpack + dequantize, no inverse colour transform"""
        planes = [np.ascontiguousarray(p) for p in planes]
        out = np.empty((3, h, w), dtype=np.float32)
        self._chk(self.L.lumahip_unpack_frame_host(self.h, _arr3(C.c_void_p, [p.ctypes.data for p in planes]),
                                                   _arr3(C.c_int, strides), w, h, profile, out.ctypes.data))
        return out

    def transform_color_space(self, frame: np.ndarray, to_cs: bool, sc=1.0) -> np.ndarray:
        assert frame.dtype == np.float32 and frame.flags.c_contiguous and frame.shape[0] == 3
        self._chk(self.L.lumahip_transform_color_space_host(self.h, frame.ctypes.data, frame.shape[2], frame.shape[1],
                                                            int(bool(to_cs)), sc))
        return frame

    def quantize_array(self, a, ch=0) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        out = np.empty_like(a)
        self._chk(self.L.lumahip_quantize_array_host(self.h, a.ctypes.data, out.ctypes.data, a.size, ch))
        return out

    def dequantize_array(self, a, ch=0) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        out = np.empty_like(a)
        self._chk(self.L.lumahip_dequantize_array_host(self.h, a.ctypes.data, out.ctypes.data, a.size, ch))
        return out

    # ---- device entry points (raw device pointers, e.g. torch.Tensor.data_ptr())
    def encode_frames_device(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                             plane_frame_strides, stats_ptr=None):
        self._frame_fed(self.L.lumahip_encode_frames_device, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, stats_ptr)

    def transcode_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h,
                                dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr=None):
        self._two_sets(self.L.lumahip_transcode_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc,
                       nframes, w, h, dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr)

    # w, h: the SOURCE size; the destination planes hold (w/2) x (h/2) luma samples (the 2x2 box in linear light)
    def transcode_half_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h,
                                     dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr=None):
        self._two_sets(self.L.lumahip_transcode_half_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile,
                       src_sc, nframes, w, h, dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr)

    # w, h: the SOURCE size; the destination planes hold (w/4) x (h/4) luma samples (the 2x2 box twice, on floats; include/lumahip_rungs.h)
    def transcode_quarter_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h,
                                        dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr=None):
        self._two_sets(self.L.lumahip_transcode_quarter_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile,
                       src_sc, nframes, w, h, dst_plane_ptrs, dst_strides, dst_plane_frame_strides, dst_profile, dst_sc, stats_ptr)

    # distortion of given planes against the frames' own encode: out_ptr receives nframes x 3 planes x {sse, sad, max_abs, n_differ}
    # as uint64 (zeroed by the call); the arguments are those of the matching encode call
    def distortion_frames_device(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides, plane_frame_strides,
                                 out_ptr):
        self._frame_fed(self.L.lumahip_distortion_frames_device, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, out_ptr)

    def distortion_frames_device_planar(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                        plane_frame_strides, out_ptr):
        self._frame_fed(self.L.lumahip_distortion_frames_device_planar, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h, sc,
                        profile, plane_ptrs, strides, plane_frame_strides, out_ptr)

    def distortion_frames_device_f16(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                     plane_frame_strides, out_ptr):
        self._frame_fed(self.L.lumahip_distortion_frames_device_f16, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, out_ptr)

    def distortion_frames_device_planar_f16(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                            plane_frame_strides, out_ptr):
        self._frame_fed(self.L.lumahip_distortion_frames_device_planar_f16, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h,
                        sc, profile, plane_ptrs, strides, plane_frame_strides, out_ptr)

    # the same per block x block luma pixels (16, 32 or 64): map_ptr receives nframes x nby x nbx x 3 planes x {sse, sad, max_abs,
    # n_differ} as uint64, every word written by the launch (distortion_map_dims, block_sample_counts)
    def distortion_map_frames_device(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides, plane_frame_strides,
                                     block, map_ptr):
        self._frame_fed(self.L.lumahip_distortion_map_frames_device, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, block, map_ptr)

    def distortion_map_frames_device_planar(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                            plane_frame_strides, block, map_ptr):
        self._frame_fed(self.L.lumahip_distortion_map_frames_device_planar, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h,
                        sc, profile, plane_ptrs, strides, plane_frame_strides, block, map_ptr)

    def distortion_map_frames_device_f16(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                         plane_frame_strides, block, map_ptr):
        self._frame_fed(self.L.lumahip_distortion_map_frames_device_f16, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs,
                        strides, plane_frame_strides, block, map_ptr)

    def distortion_map_frames_device_planar_f16(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                                plane_frame_strides, block, map_ptr):
        self._frame_fed(self.L.lumahip_distortion_map_frames_device_planar_f16, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w,
                        h, sc, profile, plane_ptrs, strides, plane_frame_strides, block, map_ptr)

    # the moments of both signals per block x block luma pixels (8, 16, 32 or 64): mom_ptr receives nframes x nby x nbx x 3 planes x
    # {Se, Sg, See, Sgg, Seg} as uint64, every word written by the launch (moments_map_dims, moments_sample_counts, code_ssim)
    def moments_map_frames_device(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides, plane_frame_strides,
                                  block, mom_ptr):
        self._frame_fed(self.L.lumahip_moments_map_frames_device, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, block, mom_ptr)

    def moments_map_frames_device_planar(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                         plane_frame_strides, block, mom_ptr):
        self._frame_fed(self.L.lumahip_moments_map_frames_device_planar, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h, sc,
                        profile, plane_ptrs, strides, plane_frame_strides, block, mom_ptr)

    def moments_map_frames_device_f16(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                      plane_frame_strides, block, mom_ptr):
        self._frame_fed(self.L.lumahip_moments_map_frames_device_f16, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs,
                        strides, plane_frame_strides, block, mom_ptr)

    def moments_map_frames_device_planar_f16(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                             plane_frame_strides, block, mom_ptr):
        self._frame_fed(self.L.lumahip_moments_map_frames_device_planar_f16, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h,
                        sc, profile, plane_ptrs, strides, plane_frame_strides, block, mom_ptr)

    # distortion of given planes against the source planes' own transcode: the arguments are transcode_frames_device's, the
    # target-side planes are read, out_ptr receives nframes x 3 planes x {sse, sad, max_abs, n_differ} as uint64 (zeroed by the call)
    def transcode_distortion_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h,
                                           given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc, out_ptr):
        self._two_sets(self.L.lumahip_transcode_distortion_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile,
                       src_sc, nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc, out_ptr)

    # the same per block x block luma pixels of the target (16, 32 or 64): map_ptr receives nframes x nby x nbx x 3 planes x {sse, sad,
    # max_abs, n_differ} as uint64, every word written by the launch
    def transcode_distortion_map_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w,
                                               h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc, block,
                                               map_ptr):
        self._two_sets(self.L.lumahip_transcode_distortion_map_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides,
                       src_profile, src_sc, nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc,
                       block, map_ptr)

    # the moments of the source planes' transcode and the given planes per block x block luma pixels of the target (8, 16, 32 or 64):
    # mom_ptr receives nframes x nby x nbx x 3 planes x {Se, Sg, See, Sgg, Seg} as uint64, every word written by the launch
    # (moments_map_dims, moments_sample_counts(w, h, dst_profile, block) and code_ssim apply unchanged)
    def transcode_moments_map_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w, h,
                                            given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc, block,
                                            mom_ptr):
        self._two_sets(self.L.lumahip_transcode_moments_map_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides,
                       src_profile, src_sc, nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc,
                       block, mom_ptr)

    # given planes of (w/2) x (h/2) against the source planes' half-resolution transcode (include/lumahip_ladder.h): the arguments are
    # transcode_distortion_frames_device's, w x h the source's size; out_ptr receives nframes x 3 planes x 4 words (zeroed by the call)
    def transcode_half_distortion_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc, nframes, w,
                                                h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc, out_ptr):
        self._two_sets(self.L.lumahip_transcode_half_distortion_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides,
                       src_profile, src_sc, nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc,
                       out_ptr)

    # the same per block x block luma pixels of the half-size target (16, 32 or 64): map_ptr receives nframes x nby x nbx x 3 planes x 4
    # words with distortion_map_dims(w // 2, h // 2, block), every word written by the launch
    def transcode_half_distortion_map_frames_device(self, src_plane_ptrs, src_strides, src_plane_frame_strides, src_profile, src_sc,
                                                    nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile,
                                                    dst_sc, block, map_ptr):
        self._two_sets(self.L.lumahip_transcode_half_distortion_map_frames_device, src_plane_ptrs, src_strides, src_plane_frame_strides,
                       src_profile, src_sc, nframes, w, h, given_plane_ptrs, given_strides, given_plane_frame_strides, dst_profile, dst_sc,
                       block, map_ptr)

    # two sets of code planes of one profile compared as they are (include/lumahip_compare.h; no quantizer needed): out_ptr receives
    # nframes x 3 planes x {sse, sad, max_abs, n_differ} as uint64 (zeroed by the call), e from set A and g from set B
    def planes_distortion_frames_device(self, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h, b_plane_ptrs, b_strides,
                                        b_plane_frame_strides, profile, out_ptr):
        self._two_plane_sets(self.L.lumahip_planes_distortion_frames_device, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h,
                             b_plane_ptrs, b_strides, b_plane_frame_strides, profile, out_ptr)

    # the same per block x block luma pixels (16, 32 or 64): map_ptr receives nframes x nby x nbx x 3 planes x 4 words, every word
    # written by the launch
    def planes_distortion_map_frames_device(self, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h, b_plane_ptrs, b_strides,
                                            b_plane_frame_strides, profile, block, map_ptr):
        self._two_plane_sets(self.L.lumahip_planes_distortion_map_frames_device, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w,
                             h, b_plane_ptrs, b_strides, b_plane_frame_strides, profile, block, map_ptr)

    # the moments of both sets per block x block luma pixels (8, 16, 32 or 64): mom_ptr receives nframes x nby x nbx x 3 planes x
    # {Se, Sg, See, Sgg, Seg} as uint64, every word written by the launch
    def planes_moments_map_frames_device(self, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h, b_plane_ptrs, b_strides,
                                         b_plane_frame_strides, profile, block, mom_ptr):
        self._two_plane_sets(self.L.lumahip_planes_moments_map_frames_device, a_plane_ptrs, a_strides, a_plane_frame_strides, nframes, w, h,
                             b_plane_ptrs, b_strides, b_plane_frame_strides, profile, block, mom_ptr)

    # content light level (include/lumahip_compare.h): out_ptr receives nframes x 8 uint64 words (zeroed by the call); the frame
    # arguments are those of the matching encode call, no quantizer needed
    def light_level_frames_device(self, rgb_ptr, frame_stride, nframes, w, h, scale, out_ptr):
        self._chk(self.L.lumahip_light_level_frames_device(self.h, rgb_ptr, frame_stride, nframes, w, h, scale, out_ptr))

    def light_level_frames_device_planar(self, rgb_plane_ptrs, frame_stride, nframes, w, h, scale, out_ptr):
        self._chk(self.L.lumahip_light_level_frames_device_planar(self.h, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h,
                                                                  scale, out_ptr))

    def light_level_frames_device_f16(self, rgb_ptr, frame_stride, nframes, w, h, scale, out_ptr):
        self._chk(self.L.lumahip_light_level_frames_device_f16(self.h, rgb_ptr, frame_stride, nframes, w, h, scale, out_ptr))

    def light_level_frames_device_planar_f16(self, rgb_plane_ptrs, frame_stride, nframes, w, h, scale, out_ptr):
        self._chk(self.L.lumahip_light_level_frames_device_planar_f16(self.h, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w,
                                                                      h, scale, out_ptr))

    # the same of the frames decode_frames_device would write for these planes under the context's quantizer and sc, never written
    def planes_light_level_frames_device(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, scale, out_ptr):
        self._plane_fed(self.L.lumahip_planes_light_level_frames_device, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile,
                        sc, scale, out_ptr)

    def mean_luminance_reference_device(self, rgb_ptr, w, h, sc=1.0) -> float:
        """the reference's sequentially-summed mean of transformed channel 0 (exact; ~25 ms at 4K)"""
        m = C.c_float(0)
        self._chk(self.L.lumahip_mean_luminance_reference_device(self.h, rgb_ptr, w, h, sc, C.byref(m)))
        return float(m.value)

    def decode_frames_device(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, rgb_ptr,
                             frame_stride):
        self._plane_fed(self.L.lumahip_decode_frames_device, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, rgb_ptr,
                        frame_stride)

    def decode_display_frames_device(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, rgba_ptr,
                                     rgba_stride, rgba_frame_stride, exposure=1.0, gamma=2.2, do_tmo=False,
                                     ldr_sim=False, rgb_ptr=None, frame_stride=0):
        """decode fused with the player's display transform -> RGBA8"""
        self._plane_fed(self.L.lumahip_decode_display_frames_device, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc,
                        rgb_ptr, frame_stride, rgba_ptr, rgba_stride, rgba_frame_stride, exposure, gamma, int(bool(do_tmo)),
                        int(bool(ldr_sim)))

    def quantize_array_device(self, in_ptr, out_ptr, n, ch=0):
        self._chk(self.L.lumahip_quantize_array_device(self.h, in_ptr, out_ptr, n, ch))

    def dequantize_array_device(self, in_ptr, out_ptr, n, ch=0):
        self._chk(self.L.lumahip_dequantize_array_device(self.h, in_ptr, out_ptr, n, ch))

    def transform_frames_device(self, ptr, frame_stride, nframes, w, h, to_cs, sc):
        self._chk(self.L.lumahip_transform_color_space_device(self.h, ptr, frame_stride, nframes, w, h,
                                                              int(bool(to_cs)), sc))

    def synth_frames_device(self, ptr, frame_stride, nframes, w, h, seed=20250929, first_frame=0):
        self._chk(self.L.lumahip_synth_frames_device(self.h, ptr, frame_stride, nframes, w, h, seed, first_frame))

    def time_launches(self, direction, iters, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                      plane_frame_strides) -> float:
        """average milliseconds per launch, measured with hipEvents on the context's stream"""
        ms = C.c_float(0)
        self._chk(self.L.lumahip_time_launches(self.h, direction, iters, rgb_ptr, frame_stride, nframes, w, h, sc,
                                               profile, _arr3(C.c_void_p, plane_ptrs), _arr3(C.c_int, strides),
                                               _arr3(C.c_size_t, plane_frame_strides), C.byref(ms)))
        return float(ms.value)

    def device(self) -> int:
        return int(self.L.lumahip_device(self.h))

    def encode_frames_device_planar(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                    plane_frame_strides, stats_ptr=None):
        """float frames as three colour-plane base pointers (plane c of frame f at rgb_plane_ptrs[c] + f*frame_stride floats)"""
        self._frame_fed(self.L.lumahip_encode_frames_device_planar, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h, sc,
                        profile, plane_ptrs, strides, plane_frame_strides, stats_ptr)

    def decode_frames_device_rotating(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, base_ptrs, frame_stride):
        """packed frames over three buffers: frame f at base_ptrs[f % 3] + (f // 3) * frame_stride floats"""
        self._plane_fed(self.L.lumahip_decode_frames_device_rotating, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc,
                        _arr3(C.c_void_p, base_ptrs), frame_stride)

    def decode_frames_device_planar(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, rgb_plane_ptrs,
                                    frame_stride):
        self._plane_fed(self.L.lumahip_decode_frames_device_planar, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc,
                        _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride)

    # binary16 frames (raw device pointers to halves, e.g. a torch.float16 tensor's data_ptr(); strides count halves)
    def encode_frames_device_f16(self, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                 plane_frame_strides, stats_ptr=None):
        self._frame_fed(self.L.lumahip_encode_frames_device_f16, rgb_ptr, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                        plane_frame_strides, stats_ptr)

    def encode_frames_device_planar_f16(self, rgb_plane_ptrs, frame_stride, nframes, w, h, sc, profile, plane_ptrs, strides,
                                        plane_frame_strides, stats_ptr=None):
        self._frame_fed(self.L.lumahip_encode_frames_device_planar_f16, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, nframes, w, h, sc,
                        profile, plane_ptrs, strides, plane_frame_strides, stats_ptr)

    def decode_frames_device_f16(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc, rgb_ptr,
                                 frame_stride):
        self._plane_fed(self.L.lumahip_decode_frames_device_f16, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc,
                        rgb_ptr, frame_stride)

    def decode_frames_device_planar_f16(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile, sc,
                                        rgb_plane_ptrs, frame_stride):
        self._plane_fed(self.L.lumahip_decode_frames_device_planar_f16, plane_ptrs, strides, plane_frame_strides, nframes, w, h, profile,
                        sc, _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride)

    def f16_narrow_probe_device(self, out_ptr, first_bits, n):
        """uint16 binary16 bits the decode kernels store for the n consecutive fp32 bit patterns from first_bits"""
        self._chk(self.L.lumahip_f16_narrow_probe_device(self.h, out_ptr, first_bits, n))

    def begin_unordered(self, lanes: int = 0):
        """open an unordered section: the following _device encode / decode calls are independent of each other"""
        self._chk(self.L.lumahip_begin_unordered(self.h, lanes))

    def end_unordered(self):
        self._chk(self.L.lumahip_end_unordered(self.h))

    def probe_decode_traffic(self, plane_ptrs, strides, plane_frame_strides, nframes, w, h, rgb_plane_ptrs, frame_stride,
                             iters=1) -> float:
        """ms per launch of the decode kernel's loads + stores without arithmetic (overwrites the frames)"""
        ms = C.c_float(0)
        self._plane_fed(self.L.lumahip_probe_decode_traffic_device, plane_ptrs, strides, plane_frame_strides, nframes, w, h,
                        _arr3(C.c_void_p, rgb_plane_ptrs), frame_stride, iters, C.byref(ms))
        return float(ms.value)

    def probe_encode_traffic(self, rgb_ptr, frame_stride, nframes, w, h, plane_ptrs, strides, plane_frame_strides,
                             iters=1) -> float:
        """ms per launch of the encode kernel's loads + stores without arithmetic (overwrites the planes)"""
        ms = C.c_float(0)
        self._chk(self.L.lumahip_probe_encode_traffic_device(self.h, rgb_ptr, frame_stride, nframes, w, h,
                                                             _arr3(C.c_void_p, plane_ptrs), _arr3(C.c_int, strides),
                                                             _arr3(C.c_size_t, plane_frame_strides), iters, C.byref(ms)))
        return float(ms.value)

    def powf_probe_device(self, out_ptr, first_bits, n, y, regular=1):
        self._chk(self.L.lumahip_powf_probe_device(self.h, out_ptr, first_bits, n, y, int(regular)))

    def quantize_probe_device(self, out_ptr, first_bits, n, nonneg=False):
        """uint16 codes of the n consecutive fp32 bit patterns from first_bits, through quantize_lut<mode, 4, nonneg>"""
        self._chk(self.L.lumahip_quantize_probe_device(self.h, out_ptr, first_bits, n, int(bool(nonneg))))

    def ycbcr_luma_probe_device(self, out_ptr, first_bits, n, direct=False):
        """uint16 luminance codes of the n consecutive fp32 luma bit patterns from first_bits (YCbCr quantizers): through the
        composite records (direct=False) or through the reference's arithmetic on the device (direct=True)"""
        self._chk(self.L.lumahip_ycbcr_luma_probe_device(self.h, out_ptr, first_bits, n, int(bool(direct))))

    def host_register(self, arr: np.ndarray):
        """pin a numpy array's memory for PCIe-rate transfers by the host entry points"""
        self._chk(self.L.lumahip_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr: np.ndarray):
        self._chk(self.L.lumahip_host_unregister(self.h, arr.ctypes.data))

    # ---- raw device memory (hosts without torch)
    def malloc(self, nbytes) -> int:
        p = C.c_void_p()
        self._chk(self.L.lumahip_malloc(self.h, C.byref(p), nbytes))
        return p.value

    def free(self, ptr):
        self._chk(self.L.lumahip_free(self.h, ptr))

    def h2d(self, dst_ptr, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.lumahip_memcpy_h2d(self.h, dst_ptr, arr.ctypes.data, arr.nbytes))

    def d2h(self, arr: np.ndarray, src_ptr):
        assert arr.flags.c_contiguous
        self._chk(self.L.lumahip_memcpy_d2h(self.h, arr.ctypes.data, src_ptr, arr.nbytes))


class DecodedRing:
    """lumahip_decoded_ring: `nbatches` batches of up to `nframes` packed LumaFrames in buffers the LIBRARY allocates and places
    (the frames of a batch rotate over three buffers in three HBM region groups); include/lumahip.h"""

    def __init__(self, ctx: Context, nbatches, nframes, w, h):
        self.L, self.ctx = lib(), ctx
        h_ = C.c_void_p()
        rc = self.L.lumahip_decoded_ring_create(ctx.h, nbatches, nframes, w, h, C.byref(h_))
        if rc != OK:
            raise LumaHipError(rc, "lumahip_decoded_ring_create failed")
        self.h = h_
        a, fs = (C.c_int * 4)(), C.c_size_t(0)
        self.L.lumahip_decoded_ring_info(self.h, a, C.byref(fs))
        self.placed, self.nbatches, self.nframes, self.groups, self.frame_stride = bool(a[0]), a[1], a[2], a[3], fs.value

    def frame_ptr(self, batch, frame) -> int:
        p = self.L.lumahip_decoded_ring_frame(self.h, batch, frame)
        if not p:
            raise LumaHipError(ERR_ARG, "no frame %d of batch %d in this ring" % (frame, batch))
        return p

    def decode(self, plane_ptrs, strides, plane_frame_strides, nframes, profile, sc, batch):
        """lumahip_decode_frames_device_ring: nframes frames into batch slot `batch` (asynchronous)"""
        self.ctx._plane_fed(self.L.lumahip_decode_frames_device_ring, plane_ptrs, strides, plane_frame_strides, nframes, profile, sc, self.h,
                            batch)

    def close(self):
        if self.h:
            self.L.lumahip_decoded_ring_destroy(self.h)
            self.h = None


class Pool:
    """lumahip_pool: device memory in chunks, classified by HBM region group (include/lumahip.h)"""

    def __init__(self, ctx: Context, n_float, n_y, n_uv, n_striped=0, chunk_bytes=0, keep_free=0, max_chunks=0, iters=0, small=False):
        self.L = lib()
        h = C.c_void_p()
        if small:       # lumahip_pool_create_small: a dozen chunks probed for milliseconds instead of all free memory for seconds
            rc = self.L.lumahip_pool_create_small(ctx.h, n_float, n_y, n_uv, n_striped, C.byref(h))
        else:
            cfg = PoolConfig(chunk_bytes, n_float, n_y, n_uv, n_striped, keep_free, max_chunks, iters)
            rc = self.L.lumahip_pool_create(ctx.h, C.byref(cfg), C.byref(h))
        if rc != OK:
            raise LumaHipError(rc, "lumahip_pool_create failed")
        self.h = h
        self.chunk_bytes = chunk_bytes or (2 << 30)

    def stats(self) -> dict:
        import json
        return json.loads(self.L.lumahip_pool_stats_json(self.h).decode())

    def available(self, kind, group=-1) -> int:
        return int(self.L.lumahip_pool_available(self.h, kind, group))

    def alloc(self, kind, group=-1) -> int:
        p = C.c_void_p()
        rc = self.L.lumahip_pool_alloc(self.h, kind, group, C.byref(p))
        if rc != OK:
            raise LumaHipError(rc, "lumahip_pool_alloc: no chunk of kind %d / group %d left" % (kind, group))
        return p.value

    def release(self, ptr: int):
        rc = self.L.lumahip_pool_release(self.h, C.c_void_p(ptr))
        if rc != OK:
            raise LumaHipError(rc, "lumahip_pool_release: not a chunk of this pool")

    def group_of(self, ptr: int) -> int:
        return int(self.L.lumahip_pool_group_of(self.h, C.c_void_p(ptr)))

    def close(self):
        if getattr(self, "h", None):
            self.L.lumahip_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """lumahip_multi: one context per shard, block-sharded batches, quantizer broadcast over RCCL (include/lumahip.h)"""

    def __init__(self, devices=None, nshards=0):
        self.L = lib()
        h = C.c_void_p()
        if devices is None:
            rc = self.L.lumahip_multi_create(C.byref(h), None, nshards)
        else:
            arr = (C.c_int * len(devices))(*devices)
            rc = self.L.lumahip_multi_create(C.byref(h), arr, len(devices))
        if rc != OK:
            raise LumaHipError(rc, "lumahip_multi_create failed (there is no CPU fallback)")
        self.h = h

    def _chk(self, rc):
        if rc != OK:
            raise LumaHipError(rc, self.L.lumahip_multi_last_error(self.h).decode())

    @property
    def shards(self) -> int:
        return int(self.L.lumahip_multi_shards(self.h))

    def used_rccl(self) -> bool:
        return bool(self.L.lumahip_multi_used_rccl(self.h))

    def set_transport(self, mode: int):
        """0 auto (RCCL across several devices, host copies on one), 1 always RCCL, 2 always host copies"""
        self._chk(self.L.lumahip_multi_set_transport(self.h, mode))

    def transport_note(self) -> str:
        return self.L.lumahip_multi_transport_note(self.h).decode()

    def ctx(self, shard: int) -> Context:
        """the shard's context as a (non-owning) Context"""
        raw = self.L.lumahip_multi_ctx(self.h, shard)
        if not raw:
            raise LumaHipError(ERR_ARG, "no such shard")
        return _BorrowedContext(self.L, C.c_void_p(raw))

    def set_quantizer(self, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum, lut: np.ndarray):
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        self._chk(self.L.lumahip_multi_set_quantizer(self.h, ptf, bitdepth, cs, bitdepthC, max_lum, min_lum, lut.ctypes.data,
                                                     lut.size))

    def encode_frames(self, frames, sc=1.0, profile=2, align=32):
        frames = [np.ascontiguousarray(f, dtype=np.float32) for f in frames]
        n = len(frames)
        _, h, w = frames[0].shape
        _, hs, st, _ = plane_geometry(w, h, profile, align)
        planes = [[np.zeros((hs[p], st[p]), dtype=np.uint8) for p in range(3)] for _ in range(n)]
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        pp = (C.c_void_p * (3 * n))(*[pl.ctypes.data for tri in planes for pl in tri])
        means = (C.c_float * n)()
        self._chk(self.L.lumahip_multi_encode_frames_host(self.h, fp, n, w, h, sc, profile, pp, _arr3(C.c_int, st), means))
        return planes, st, [float(m) for m in means]

    def decode_frames(self, planes_list, strides, w, h, sc=1.0, profile=2):
        n = len(planes_list)
        planes_list = [[np.ascontiguousarray(p) for p in tri] for tri in planes_list]
        outs = [np.empty((3, h, w), dtype=np.float32) for _ in range(n)]
        pp = (C.c_void_p * (3 * n))(*[pl.ctypes.data for tri in planes_list for pl in tri])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        self._chk(self.L.lumahip_multi_decode_frames_host(self.h, pp, _arr3(C.c_int, strides), n, w, h, profile, sc, op))
        return outs

    def encode_frames_device(self, rgb_ptrs, frame_stride, counts, w, h, sc, profile, plane_ptrs, strides, plane_frame_strides):
        """rgb_ptrs[s], counts[s], plane_ptrs[s] = (Y, U, V) per shard"""
        ns = self.shards
        rp = (C.c_void_p * ns)(*rgb_ptrs)
        cn = (C.c_uint * ns)(*counts)
        pp = (C.c_void_p * (3 * ns))(*[p for tri in plane_ptrs for p in tri])
        self._chk(self.L.lumahip_multi_encode_frames_device(self.h, rp, frame_stride, cn, w, h, sc, profile, pp,
                                                            _arr3(C.c_int, strides), _arr3(C.c_size_t, plane_frame_strides)))

    def decode_frames_device(self, plane_ptrs, strides, plane_frame_strides, counts, w, h, profile, sc, rgb_ptrs, frame_stride):
        ns = self.shards
        rp = (C.c_void_p * ns)(*rgb_ptrs)
        cn = (C.c_uint * ns)(*counts)
        pp = (C.c_void_p * (3 * ns))(*[p for tri in plane_ptrs for p in tri])
        self._chk(self.L.lumahip_multi_decode_frames_device(self.h, pp, _arr3(C.c_int, strides),
                                                            _arr3(C.c_size_t, plane_frame_strides), cn, w, h, profile, sc, rp,
                                                            frame_stride))

    def sync(self):
        self._chk(self.L.lumahip_multi_sync(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.lumahip_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedContext(Context):
    """a Context view of a lumahip_ctx owned by someone else (a Multi): never destroyed from here"""

    def __init__(self, L, h):
        self.L = L
        self.h = h

    def close(self):
        self.h = None
