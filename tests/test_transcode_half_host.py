"""Half-resolution transcode, what needs no GPU (include/lumahip_compare.h lumahip_transcode_half_frames_device /
lumahip_transcode_half_frame_host): the two symbols are exported, declared in the open header and bound in capi._ABI_COMPARE; the
header compiles as C99; the matrix of tests/test_gpu_transcode_half.py names all 48 k_transcode_half<CSD, SUBD, CSE, SUBE, VW, LM>;
and the inputs of every row can fail: modelled with the oracle and numpy (tests/support/transcode_half.py), a kernel that takes the
top-left pixel, the horizontal pair or the vertical pair in the place of the 2x2 average writes another luma plane, and on the
Lu'v' -> Lu'v' rows at 264x72 and 268x76 so does one that adds in the order (a + c) + (b + d) or ((a + b) + c) + d.  The counts
are conditions on the inputs, asserted as lower bounds of 1 and printed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support import frame_kernels as fk
from tests.support import transcode_half as th
from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.tools import ROOT
from tests.support.transcode_moments import declarations

HEADER = "lumahip_compare.h"
DEVICE, HOST = "lumahip_transcode_half_frames_device", "lumahip_transcode_half_frame_host"
ROWS = th.half_matrix()


def test_the_two_symbols_are_exported_declared_and_bound(L):
    from lumahdrv_amd import capi
    table = capi._ABI_COMPARE
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    decls = declarations(open(os.path.join(ROOT, "include", HEADER)).read())
    lib = capi.lib()
    for name in (DEVICE, HOST):
        assert name in table and name in capi.COMPARE_SYMBOLS, name
        assert (" T " + name + "\n") in exported, name
        assert name in decls, name
        restype, argtypes = table[name]
        assert restype is C.c_int and len(argtypes) == len(decls[name]), (name, len(argtypes), len(decls[name]))
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
    # the transcode call's parameters, the device form with its statistics, the host form without a mean
    assert table[DEVICE] == capi._ABI["lumahip_transcode_frames_device"]
    assert table[HOST][1] == capi._ABI["lumahip_transcode_frame_host"][1][:-1]
    assert decls[DEVICE][-1].split()[-1] == "*stats_dev" and "mean_lum" not in " ".join(decls[HOST])
    # the closed header stands
    main = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    assert not {DEVICE, HOST} & set(declarations(main)) and len(capi.SYMBOLS) == 126
    assert "#define LUMAHIP_ABI_VERSION 5\n" in main and lib.lumahip_abi_version() == 5
    for method in ("transcode_half_frames_device", "transcode_half_frame"):
        assert callable(getattr(capi.Context, method, None)), method


def test_the_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler installed")
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(sizeof &%s + sizeof &%s) + LUMAHIP_ABI_VERSION; }\n' % (HEADER, DEVICE, HOST))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_matrix_names_all_48_kernels():
    want = {(csd, subd, cse, sube, vw, lm) for csd in (fk.LUV, fk.YCC) for subd in (True, False) for (cse, lm) in ((fk.LUV, 3), (fk.LUV, 7), (fk.YCC, 5))
            for sube in (True, False) for vw in (4, 2)}
    got = {th.kernel_of(r) for r in ROWS}
    assert len(want) == 48 and got == want, (sorted(want - got), sorted(got - want))
    assert len({r.id for r in ROWS}) == len(ROWS)
    # the sizes are the issue's, each with the vector width it is there for, and every target is even both ways
    assert th.SIZES == [(264, 72), (520, 12), (268, 76), (8, 4)]
    assert [4 if (w // 2) % 4 == 0 else 2 for (w, _) in th.SIZES] == [4, 4, 2, 4]
    assert all(w % 4 == 0 and h % 4 == 0 for (w, h) in th.SIZES)
    assert {(r.w, r.h) for r in ROWS} == set(th.SIZES)
    # a YCbCr source at preScaling 1, 20 and 3e5; the 8-bit profile pairs under 8-bit tables
    assert {r.src_sc for r in ROWS if r.csd == fk.YCC} == {1.0, 20.0, 3e5}
    eight = [r for r in ROWS if r.eight]
    assert {(r.sp, r.dp) for r in eight} == {pair for (pair, _) in th.EIGHT_BIT} and len(eight) == 16
    assert all((r.scfg[1] == 8) == (r.sp < 2) and (r.dcfg[1] == 8) == (r.dp < 2) for r in ROWS)
    assert sum(r.stats for r in ROWS) >= len(ROWS) // 2 - 2


def test_the_model_is_the_specified_average():
    """box() on values where the three orders differ by hand: fp32, ((a + b) + (c + d)) * 0.25"""
    d = np.array([[[1.0, 2.0 ** -24], [2.0 ** -24, 2.0 ** -24]]], dtype=np.float32)       # a = 1, the other three half an ulp of 1 each
    f32 = np.float32
    assert th.box(d)[0, 0, 0] == (f32(1.0) + f32(2.0 ** -23)) * f32(0.25)                  # (1 + e) -> 1; (e + e) = 2e; 1 + 2e exact
    assert th.box(d, "sequential")[0, 0, 0] == f32(0.25)                                   # every e is lost in turn
    assert th.box(d, "columns")[0, 0, 0] == th.box(d)[0, 0, 0]
    g = np.array([[[1.0, 3 * 2.0 ** -26], [1.0, 3 * 2.0 ** -25]]], dtype=np.float32)        # with e = 2^-24: b = 0.75 e, d = 1.5 e
    assert th.box(g)[0, 0, 0] == f32(0.5)                                                  # (1 + b) -> 1, (1 + d) -> 1 + 2e, 2 + 2e -> 2 (ties to even)
    assert th.box(g, "columns")[0, 0, 0] == (f32(2.0) + f32(2.0 ** -22)) * f32(0.25)       # 2 + 2.25 e -> 2 + 4e
    r = np.random.default_rng(5).standard_normal((3, 8, 12)).astype(np.float32)
    want = ((r[:, 0::2, 0::2].astype(np.float64) + r[:, 0::2, 1::2]) + (r[:, 1::2, 0::2].astype(np.float64) + r[:, 1::2, 1::2])) * 0.25
    assert th.box(r).shape == (3, 4, 6) and np.allclose(th.box(r), want, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_every_rows_inputs_tell_the_right_kernel_from_wrong_ones(oracle_mod, row):
    ex = th.expected_of(oracle_mod, row)
    tw, t_h = row.w // 2, row.h // 2
    assert ex.m.shape == (th.NF, 3, t_h, tw) and ex.m.dtype == np.float32
    for name in th.WRONG_KERNELS:
        n = th.luma_differences(oracle_mod, row, name)
        print("%s %s: %d of %d luma samples of frame 0 differ" % (row.id, name, n, tw * t_h))
        assert n >= 1, (row.id, name)
    if row.csd == fk.LUV and row.cse == fk.LUV and not row.eight and (row.w, row.h) in th.ORDER_SIZES:
        for name in th.WRONG_ORDERS:
            n = th.luma_differences(oracle_mod, row, name)
            print("%s order %s: %d luma samples of frame 0 differ" % (row.id, name, n))
            assert n >= 1, (row.id, name)
