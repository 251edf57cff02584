"""Half-resolution transcode distortion and its map, what needs no GPU (include/lumahip_ladder.h): the four symbols are exported,
declared in the new header and bound in capi._ABI_LADDER with their full-size counterparts' argument types, apart from the three older
tables, which stand as they were; the header compiles as C99; the two matrices of tests/support/transcode_half_measure.py name every
k_transcode_half_distortion / k_transcode_half_distortion_map that is instantiated; and the inputs of every row can fail.

The last are conditions on the inputs with a lower bound of 1, asserted and printed: every frame's given luma plane differs from the
model's e; for each wrong kernel of tests/support/transcode_half.py (top-left pixel, horizontal pair, vertical pair) at least one
word of the expected output differs from the words of that kernel's planes against the same g; and on the 16-bit Lu'v' -> Lu'v' rows
at 264x72, 268x76 and 264x140 the same for the two other orders of the sum."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support import far_layouts
from tests.support import frame_kernels as fk
from tests.support import transcode_half as th
from tests.support import transcode_half_measure as hm
from tests.support.device import L  # noqa: F401  (the module fixture)
from tests.support.tools import ROOT
from tests.support.transcode_moments import declarations

HEADER = "lumahip_ladder.h"
COUNTERPART = {"lumahip_transcode_half_distortion_frames_device": "lumahip_transcode_distortion_frames_device",
               "lumahip_transcode_half_distortion_map_frames_device": "lumahip_transcode_distortion_map_frames_device",
               "lumahip_transcode_half_distortion_frame_host": "lumahip_transcode_distortion_frame_host",
               "lumahip_transcode_half_distortion_map_frame_host": "lumahip_transcode_distortion_map_frame_host"}
ROWS = [r for family in hm.FAMILIES for r in hm.measure_matrix(family)]


def test_the_four_symbols_are_exported_declared_and_bound(L):
    from lumahdrv_amd import capi
    table = capi._ABI_LADDER
    assert tuple(table) == capi.LADDER_SYMBOLS == tuple(COUNTERPART)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    decls = declarations(open(os.path.join(ROOT, "include", HEADER)).read())
    main = declarations(open(os.path.join(ROOT, "include", "lumahip.h")).read())
    assert set(decls) == set(table)
    lib = capi.lib()
    for name, full in COUNTERPART.items():
        assert (" T " + name + "\n") in exported, name
        restype, argtypes = table[name]
        assert (restype, argtypes) == capi._ABI[full], name                # the counterpart's argument types ...
        assert len(decls[name]) == len(main[full]) == len(argtypes), name   # ... and as many parameters in the header
        assert [d.split()[0:-1] for d in decls[name]] == [d.split()[0:-1] for d in main[full]], name   # of the same types
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
    # apart from the three other tables, which stand as they were
    others = set(capi._ABI) | set(capi._ABI_MEASURE) | set(capi._ABI_COMPARE)
    assert not set(table) & others
    assert len(capi.SYMBOLS) == 126 and len(capi.MEASURE_SYMBOLS) == 2
    for hdr in ("lumahip.h", "lumahip_measure.h", "lumahip_compare.h"):
        assert not set(table) & set(declarations(open(os.path.join(ROOT, "include", hdr)).read())), hdr
    assert "#define LUMAHIP_ABI_VERSION 5\n" in open(os.path.join(ROOT, "include", "lumahip.h")).read() and lib.lumahip_abi_version() == 5
    # the far-layout matrix enumerates the three older tables: what it must name is what it named
    strided = far_layouts.strided_symbols(capi)
    assert not set(table) & set(strided)
    assert set(strided) <= others
    for method in ("transcode_half_distortion_frames_device", "transcode_half_distortion_map_frames_device",
                   "transcode_half_distortion_frame", "transcode_half_distortion_map_frame"):
        assert callable(getattr(capi.Context, method, None)), method


def test_the_header_compiles_as_c99(tmp_path):
    cc = shutil.which("cc")
    assert cc is not None, "no C compiler installed"
    src = tmp_path / "uses_header.c"
    src.write_text('#include "%s"\nint uses_header(void) { return (int)(%s) + LUMAHIP_ABI_VERSION; }\n'
                   % (HEADER, " + ".join("sizeof &%s" % n for n in COUNTERPART)))
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_matrices_name_every_instantiated_kernel():
    for family in hm.FAMILIES:
        rows = [r for r in ROWS if r.family == family]
        got, want = {hm.kernel_of(r) for r in rows}, hm.instantiated(family)
        assert got == want, (family, sorted(want - got), sorted(got - want))
        # 24 keys at VW 2; at VW 4 the twelve of a 4:2:0 source and the two Lu'v' 4:4:4 -> YCbCr ones
        assert len(want) == 38 and sum(k[5] == 4 for k in want) == 14, family
        assert len(rows) == len(th.half_matrix()) and len({r.id for r in rows}) == len(rows)
    assert len(ROWS) == 326
    dist, dmap = ([r for r in ROWS if r.family == f] for f in hm.FAMILIES)
    # the per-frame rows are th.half_matrix() as it stands; the map's differ in the sizes, position by position, and carry the blocks
    assert [tuple(r)[3:] for r in dist] == [tuple(r)[1:] for r in th.half_matrix()] and all(r.block is None for r in dist)
    assert hm.MAP_SIZES == [(264, 140), (520, 12), (268, 76), (8, 4)]
    assert [(r.w, r.h) for r in dmap] == [hm.MAP_SIZES[th.SIZES.index((d.w, d.h))] for d in dist]
    assert [r.block for r in dmap] == [(16, 32, 64)[n % 3] for n in range(len(dmap))]
    assert [r._replace(id="", family="", block=None, w=0, h=0) for r in dmap] == [r._replace(id="", family="", block=None, w=0, h=0) for r in dist]
    # 264x140: a 132x70 target, four pixels per thread, 9 x 5 blocks of 16 and 3 x 2 of 64 with a last block row 6 rows high
    assert (132 % 4, -(-132 // 16), -(-70 // 16), -(-132 // 64), -(-70 // 64), 70 - 64) == (0, 9, 5, 3, 2, 6)
    assert {b for r in dmap if (r.w, r.h) == (264, 140) for b in [r.block]} == {16, 32, 64}
    assert all(r.w % 4 == 0 and r.h % 4 == 0 for r in ROWS)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_every_rows_inputs_can_fail(oracle_mod, row):
    inp = hm.inputs_of(oracle_mod, row)
    tw, t_h = row.w // 2, row.h // 2
    assert inp.dist.shape == (hm.NF, 3, 4)
    if row.family == "distortion_map":
        assert inp.words.shape == (hm.NF, -(-t_h // row.block), -(-tw // row.block), 3, 4)
    for f in range(hm.NF):
        n = int(inp.dist[f, 0, 3])
        print("%s frame %d: %d of %d given luma samples differ from e" % (row.id, f, n, tw * t_h))
        assert n >= 1, (row.id, f)
    names = list(th.WRONG_KERNELS)
    if row.csd == fk.LUV and row.cse == fk.LUV and not row.eight and (row.w, row.h) in hm.ORDER_SIZES[row.family]:
        names += list(th.WRONG_ORDERS)
    for name in names:
        n = int(np.count_nonzero(hm.wrong_words(oracle_mod, row, name) != inp.words))
        print("%s %s: %d of %d expected words differ from the wrong kernel's" % (row.id, name, n, inp.words.size))
        assert n >= 1, (row.id, name)
