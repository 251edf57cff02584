"""Quarter-resolution transcode, what needs no GPU (include/lumahip_rungs.h lumahip_transcode_quarter_frames_device /
lumahip_transcode_quarter_frame_host): the two symbols are exported, declared in the new header and only there, and bound in
capi._ABI_RUNGS with the half-resolution call's relation to the transcode call's types, apart from the four older tables; the header
compiles as C99; the matrix of tests/support/transcode_quarter.py names all 48 k_transcode_quarter<CSD, SUBD, CSE, SUBE, VW, LM>; the
model is the specified average; and the inputs of every row can fail: modelled with the oracle and numpy, a kernel that takes source
pixel (4X, 4Y) or the half-size mean at (2X, 2Y) alone writes another luma plane, and on the Lu'v' -> Lu'v' rows at 528x144 and
536x152 so does one that adds the sixteen in raster order or row by row.  The counts are conditions on the inputs, asserted as lower
bounds of 1 and printed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support import far_layouts
from tests.support import frame_kernels as fk
from tests.support import transcode_quarter as tq
from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.tools import ROOT
from tests.support.transcode_moments import declarations

HEADER = "lumahip_rungs.h"
DEVICE, HOST = "lumahip_transcode_quarter_frames_device", "lumahip_transcode_quarter_frame_host"
OLDER_HEADERS = ("lumahip.h", "lumahip_measure.h", "lumahip_compare.h", "lumahip_ladder.h")
ROWS = tq.quarter_matrix()


def test_the_two_symbols_are_exported_declared_and_bound(L):
    from lumahdrv_amd import capi
    table = capi._ABI_RUNGS
    assert tuple(table) == capi.RUNGS_SYMBOLS == (DEVICE, HOST)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    decls = declarations(open(os.path.join(ROOT, "include", HEADER)).read())
    assert set(decls) == set(table)
    lib = capi.lib()
    for name in (DEVICE, HOST):
        assert (" T " + name + "\n") in exported, name
        restype, argtypes = table[name]
        assert restype is C.c_int and len(argtypes) == len(decls[name]), (name, len(argtypes), len(decls[name]))
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
    # the transcode call's parameters, the device form with its statistics, the host form without a mean: the half call's relation
    assert table[DEVICE] == capi._ABI["lumahip_transcode_frames_device"] == capi._ABI_COMPARE["lumahip_transcode_half_frames_device"]
    assert table[HOST][1] == capi._ABI["lumahip_transcode_frame_host"][1][:-1] and table[HOST] == capi._ABI_COMPARE["lumahip_transcode_half_frame_host"]
    assert decls[DEVICE][-1].split()[-1] == "*stats_dev" and "mean_lum" not in " ".join(decls[HOST])
    half = declarations(open(os.path.join(ROOT, "include", "lumahip_compare.h")).read())
    for name, other in ((DEVICE, "lumahip_transcode_half_frames_device"), (HOST, "lumahip_transcode_half_frame_host")):
        assert [d.split()[0:-1] for d in decls[name]] == [d.split()[0:-1] for d in half[other]], name   # parameter for parameter, the same types
    # apart from the four other tables and their headers, which stand as they were
    others = set(capi._ABI) | set(capi._ABI_MEASURE) | set(capi._ABI_COMPARE) | set(capi._ABI_LADDER)
    assert not set(table) & others
    assert len(capi.SYMBOLS) == 126 and len(capi.MEASURE_SYMBOLS) == 2 and len(capi.LADDER_SYMBOLS) == 4
    for hdr in OLDER_HEADERS:
        assert not set(table) & set(declarations(open(os.path.join(ROOT, "include", hdr)).read())), hdr
    assert "#define LUMAHIP_ABI_VERSION 5\n" in open(os.path.join(ROOT, "include", "lumahip.h")).read() and lib.lumahip_abi_version() == 5
    assert not set(table) & set(far_layouts.strided_symbols(capi))
    for method in ("transcode_quarter_frames_device", "transcode_quarter_frame"):
        assert callable(getattr(capi.Context, method, None)), method


def test_the_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc")
    assert cc is not None, "no C compiler installed"
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(sizeof &%s + sizeof &%s) + LUMAHIP_ABI_VERSION; }\n' % (HEADER, DEVICE, HOST))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_matrix_names_all_48_kernels():
    want = {(csd, subd, cse, sube, vw, lm) for csd in (fk.LUV, fk.YCC) for subd in (True, False) for (cse, lm) in ((fk.LUV, 3), (fk.LUV, 7), (fk.YCC, 5))
            for sube in (True, False) for vw in (4, 2)}
    got = {tq.kernel_of(r) for r in ROWS}
    assert len(want) == 48 and got == want, (sorted(want - got), sorted(got - want))
    assert len({r.id for r in ROWS}) == len(ROWS)
    # the sizes are the issue's, each with the vector width it is there for; every source is a multiple of 8 and every target even both ways
    assert tq.SIZES == [(528, 144), (1040, 24), (536, 152), (16, 8), (8, 8)]
    assert [((w // 4, h // 4), 4 if (w // 4) % 4 == 0 else 2) for (w, h) in tq.SIZES] == [((132, 36), 4), ((260, 6), 4), ((134, 38), 2), ((4, 2), 4), ((2, 2), 2)]
    assert all(w % 8 == 0 and h % 8 == 0 for (w, h) in tq.SIZES)
    assert {(r.w, r.h) for r in ROWS} == set(tq.SIZES)
    # the half matrix row for row with the sources doubled, then the six rows of the smallest frame
    half = tq.th.half_matrix()
    assert [r._replace(id="", w=r.w // 2, h=r.h // 2) for r in ROWS[:len(half)]] == [r._replace(id="") for r in half]
    assert [(r.w, r.h) for r in ROWS[len(half):]] == [(8, 8)] * 6 and len({(r.csd, r.cse, r.lm) for r in ROWS[len(half):]}) == 6
    assert {r.src_sc for r in ROWS if r.csd == fk.YCC} == {1.0, 20.0, 3e5}
    eight = [r for r in ROWS if r.eight]
    assert {(r.sp, r.dp) for r in eight} == {pair for (pair, _) in tq.th.EIGHT_BIT} and len(eight) == 16
    assert all((r.scfg[1] == 8) == (r.sp < 2) and (r.dcfg[1] == 8) == (r.dp < 2) for r in ROWS)
    assert sum(r.stats for r in ROWS) >= len(ROWS) // 2 - 2


def test_the_model_is_the_specified_average():
    """box(box()) on a hand-made 8 x 8 frame whose sixteen values make the association visible: fp32,
    M = ((m00 + m01) + (m10 + m11)) * 0.25 of the 2x2 means m = ((a + b) + (c + d)) * 0.25"""
    f32 = np.float32
    e = 2.0 ** -24                                        # half an ulp of 1
    d = np.zeros((1, 8, 8), dtype=np.float32)
    # target pixel (0, 0): the top-left 2x2 block is 4, 0, 0, 0 -> m00 = 1; every other source pixel is 4e -> m01 = m10 = m11 = 4e.
    # spec: (1 + 4e) + (4e + 4e) = (1 + 4e) + 8e = 1 + 12e, exact; * 0.25.
    d[0, :4, :4] = 4 * e
    d[0, 0, 0], d[0, 0, 1], d[0, 1, 0], d[0, 1, 1] = 4.0, 0.0, 0.0, 0.0
    # target pixel (1, 0): 1 at (4, 0), e at (4, 1) and at (6, 1), zeros elsewhere
    d[0, 0, 4], d[0, 1, 4], d[0, 1, 6] = 1.0, e, e
    got = tq.box(tq.box(d))
    assert got.shape == (1, 2, 2) and got.dtype == np.float32
    assert got[0, 0, 0] == (f32(1.0) + f32(12 * e)) * f32(0.25)
    # m00 = ((1 + 0) + (e + 0)) / 4: 1 + e -> 1 (ties to even), m00 = 0.25; m01 = e / 4, half an ulp of 0.25: 0.25 + e/4 -> 0.25; M = 1/16
    assert got[0, 0, 1] == f32(0.0625)
    # row by row the two e meet each other before they meet the 1: (1 + 0) + (0 + 0) = 1, (e + 0) + (e + 0) = 2e, 1 + 2e is exact
    rows = tq.wrong_frame(d, "rows")[0, 0, 1]
    assert rows == (f32(1.0) + f32(2 * e)) * f32(0.0625) and rows != got[0, 0, 1]
    # pixel (0, 0) in raster order: 4 + 0, then + 4e again and again -- half an ulp of 4, ties to even: 4 every time
    assert tq.wrong_frame(d, "raster")[0, 0, 0] == f32(0.25) and tq.wrong_frame(d, "raster")[0, 0, 0] != got[0, 0, 0]
    assert tq.wrong_frame(d, "top_left")[0, 0, 0] == f32(4.0) and tq.wrong_frame(d, "top_left_2x2")[0, 0, 0] == f32(1.0)
    r = np.random.default_rng(5).standard_normal((3, 16, 24)).astype(np.float32)
    want = r.astype(np.float64).reshape(3, 4, 4, 6, 4).mean(axis=(2, 4))
    assert tq.box(tq.box(r)).shape == (3, 4, 6) and np.allclose(tq.box(tq.box(r)), want, rtol=1e-5, atol=1e-6)
    for name in tq.WRONG_ORDERS:
        assert np.allclose(tq.wrong_frame(r, name), want, rtol=1e-5, atol=1e-6), name
    assert np.array_equal(tq.wrong_frame(r, "top_left"), r[:, 0::4, 0::4])


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_every_rows_inputs_tell_the_right_kernel_from_wrong_ones(oracle_mod, row):
    ex = tq.expected_of(oracle_mod, row)
    tw, t_h = row.w // 4, row.h // 4
    assert ex.m.shape == (tq.NF, 3, t_h, tw) and ex.m.dtype == np.float32
    for name in tq.WRONG_KERNELS:
        n = tq.luma_differences(oracle_mod, row, name)
        print("%s %s: %d of %d luma samples of frame 0 differ" % (row.id, name, n, tw * t_h))
        assert n >= 1, (row.id, name)
    if row.csd == fk.LUV and row.cse == fk.LUV and not row.eight and (row.w, row.h) in tq.ORDER_SIZES:
        for name in tq.WRONG_ORDERS:
            n = tq.luma_differences(oracle_mod, row, name)
            print("%s order %s: %d luma samples of frame 0 differ" % (row.id, name, n))
            assert n >= 1, (row.id, name)
