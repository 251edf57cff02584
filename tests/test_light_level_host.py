"""Content light level, what needs no GPU (include/lumahip_compare.h): the seven symbols are exported, declared in the open header as
lumahdrv_amd.capi's third table binds them, and wrapped by Context; the header compiles as C; content_light_level against hand-computed
cases; the numpy model the GPU test (tests/test_gpu_light_level.py) holds the kernels to against a scalar Python restatement; and the
frames that test builds (tests/support/light_level.py frames) cannot pass a wrong kernel:
  - in every frame the brightest pixel sits in another channel (R, G, B in turn) and in the bottom right corner, so in the last row and
    in the last column;
  - words 0, 1, 4 and 5 differ between all frames; words 2, 3, 6 and 7 are non-zero in frame 0 and zero in frames 1 and 2;
  - dropping a channel, the last row, the last column or the scale changes word 0 in every frame, and word 1 in every frame that has
    no pixel over (frames 1 and 2; a channel: in the frame whose corner it holds) -- frame 0, saturated by its planted pixels, loses a
    count of word 2 with its corner instead."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.light_level import (LL_DEVICE, LL_HEADER, LL_HOST, LL_METHODS, LL_SIZES, LL_SYMBOLS, NF, OVER, SCALES, WORDS, frames,
                                       inputs_cannot_pass, model, model_frames, planted, scalar_model)
from tests.support.tools import ROOT
from tests.support.transcode_moments import declarations

HEADER = os.path.join(ROOT, "include", LL_HEADER)


def test_the_seven_symbols_are_exported_declared_and_bound(L):
    from lumahdrv_amd import capi
    table = capi._ABI_COMPARE
    assert len(LL_SYMBOLS) == 7 and set(LL_SYMBOLS) <= set(table) and set(LL_SYMBOLS) <= set(capi.COMPARE_SYMBOLS)
    assert not set(LL_SYMBOLS) & (set(capi.SYMBOLS) | set(capi.MEASURE_SYMBOLS))
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    text = open(HEADER).read()
    decls = declarations(text)
    lib = capi.lib()
    for name in LL_SYMBOLS:
        assert (" T " + name + "\n") in exported, name
        restype, argtypes = table[name]
        assert name in decls and restype is C.c_int and len(argtypes) == len(decls[name]), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
    # the four frame-fed device forms share everything behind the frames; every call ends on (..., float scale, uint64_t *out)
    tails = {tuple(decls[n][2:]) for n in LL_DEVICE[:4]}
    assert len(tails) == 1
    for name in LL_SYMBOLS:
        assert decls[name][-2] == "float scale" and decls[name][-1].startswith("uint64_t") and table[name][1][-2] is C.c_float, name
    for name in LL_HOST:
        assert decls[name][-1] == "uint64_t out[8]", name
    assert "#define LUMAHIP_LIGHT_WORDS 8\n" in text and capi.LIGHT_WORDS == WORDS == 8
    # the closed header stands
    main = declarations(open(os.path.join(ROOT, "include", "lumahip.h")).read())
    assert not set(LL_SYMBOLS) & set(main) and len(capi.SYMBOLS) == 126 and capi.lib().lumahip_abi_version() == 5
    for method in LL_METHODS:
        assert callable(getattr(capi.Context, method, None)), method
    import lumahdrv_amd
    assert lumahdrv_amd.content_light_level is capi.content_light_level


def test_the_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler installed")
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(%s) + LUMAHIP_LIGHT_WORDS; }\n'
                   % (LL_HEADER, " + ".join("sizeof &" + n for n in LL_SYMBOLS)))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_content_light_level_against_hand_computed_cases():
    from lumahdrv_amd.capi import content_light_level as cll
    w, h = 4, 2
    row = lambda s, m: [s, m, 0, 0, 0, 0, 0, 0]   # noqa: E731
    # one frame: a peak of exactly 1000 cd/m2, every pixel at 100
    assert cll([row(100 * 256 * 8, 1000 * 256)], w, h) == (1000, 100)
    # one unit of 1/256 more rounds up, in both
    assert cll([row(100 * 256 * 8 + 1, 1000 * 256 + 1)], w, h) == (1001, 101)
    # the maxima are taken over the frames, each on its own: the peak from frame 1, the average from frame 0
    assert cll([row(300 * 256 * 8, 400 * 256), row(200 * 256 * 8, 4000 * 256)], w, h) == (4000, 300)
    # one frame's eight words without the outer list
    assert cll(np.array(row(8 * 256, 256), dtype=np.uint64), w, h) == (1, 1)
    # below one unit is still above zero
    assert cll([row(1, 1)], w, h) == (1, 1)
    # the cap of the 16-bit fields: a saturated pixel, and a frame of them (the sum of an 8K frame fits 64 bits)
    assert cll([row(OVER, OVER)], w, h) == (65535, 65535)
    px = 7680 * 4320
    assert px * OVER < 1 << 64 and cll([row(px * OVER, OVER)], 7680, 4320) == (65535, 65535)
    assert cll([row(65535 * 256 * 8, 65535 * 256)], w, h) == (65535, 65535)
    assert cll([row(65534 * 256 * 8 + 1, 65534 * 256 + 1)], w, h) == (65535, 65535)
    assert cll([row(65534 * 256 * 8, 65534 * 256)], w, h) == (65534, 65534)
    # an all-zero stream, and no frame at all
    assert cll(np.zeros((5, 8), dtype=np.uint64), w, h) == (0, 0) and cll(np.zeros((0, 8), dtype=np.uint64), w, h) == (0, 0)
    # Python integers come back
    assert all(type(v) is int for v in cll([row(3, 2)], w, h))
    # words beyond 2^63 are unsigned
    assert cll(np.array([row((1 << 64) - 1, 5)], dtype=np.uint64), 1 << 20, 1 << 20) == (1, 65535)


def test_the_model_against_a_scalar_restatement():
    fr = frames(6, 4)
    assert len(planted()) == 9
    for scale in SCALES:
        for f in range(NF):
            got, want = model(fr[f], scale), scalar_model(fr[f], scale)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (scale, f, got, want)
    # by hand: a 2 x 2 frame
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    f = np.array([[[1.5, nan], [-2.0, 16777216.0]], [[0.25, nan], [-1.0, 0.0]], [[0.0, nan], [inf, 0.0]]], dtype=np.float32)
    w = model(f, 1.0)
    # m = 1.5, NaN, inf, 16777216 -> q = 384, 0, over, over
    assert list(w[:4]) == [384 + 2 * OVER, OVER, 2, 1]
    # y = 0.212656 * 1.5 + 0.715158 * 0.25 = 0.4977735 -> 127; NaN; inf (finite + inf); 0.212656f * 2^24 * 256, exact: about 9.1335e8
    y3 = int(np.floor(np.float32(np.float32(0.212656) * np.float32(16777216.0)) * np.float32(256)))
    assert list(w[4:]) == [127 + OVER + y3, OVER, 1, 1] and 913350000 < y3 < 913351000
    # the scale is one rounded multiply in front of everything
    assert list(model(f, 0.5)[:4]) == [192 + OVER + (1 << 31), OVER, 1, 1]


def test_the_gpu_tests_inputs_cannot_pass_a_wrong_kernel():
    n = 0
    for (w, h) in LL_SIZES:
        for halves in (False, True):
            fr = frames(w, h, halves)
            assert fr.shape == (NF, 3, h, w) and fr.dtype == np.float32
            if halves:   # both calls are given binary16 values
                with np.errstate(over="ignore"):
                    assert np.array_equal(fr.astype(np.float16).astype(np.float32), fr, equal_nan=True)
            for scale in SCALES:
                words = inputs_cannot_pass(fr, scale, (w, h, halves, scale))
                assert np.array_equal(words, model_frames(fr, scale))
                n += 1
    assert n == 36
    # frame 0's planted pixels are all there: a NaN of one channel that m ignores and y does not
    w0 = model(frames(64, 32)[0], 1.0)
    assert w0[3] == 1 and w0[7] == 2 and w0[2] == 3 and w0[6] == 2 and w0[1] == OVER
