"""tests/support/far_layouts.py without a GPU: the layouts of tests/test_gpu_far_layouts.py are as far as they claim, a 32-bit address of
either kind stays inside their allocation and misses the true one, every row is one the library's host checks accept, the matrix names
every device entry point that takes a frame stride or plane frame strides, and the rows can fail: four wrong kernels, modelled on a
sparse picture of the allocation (regions over a sentinel background, never an array of its size), miss the oracle's expectation --
numpy's for the words -- on every row they apply to:
  a reader that narrows the frame term f * frame stride to 32 bits, unsigned or signed,
  a reader that narrows the row term row * stride,
  a writer that narrows either (its true destination then stays the sentinel),
  a host check that forms a span in 32 bits and so accepts what must be refused."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lumahdrv_amd import capi  # noqa: E402
from tests.support import far_layouts as fl  # noqa: E402
from tests.support.host import SENTINEL  # noqa: E402

ROWS = fl.matrix()
PLAIN = [r for r in ROWS if r.shape == "default"]
SYMBOLS = sorted(set(r.symbol for r in ROWS))
B31, B32 = 1 << 31, 1 << 32


def test_matrix_names_every_entry_point_with_a_stride():
    want = set(fl.strided_symbols(capi))
    for known in ("lumahip_encode_frames_device", "lumahip_decode_frames_device_rotating", "lumahip_transform_color_space_device",
                  "lumahip_synth_frames_device", "lumahip_light_level_frames_device_planar_f16", "lumahip_transcode_moments_map_frames_device",
                  "lumahip_planes_moments_map_frames_device", "lumahip_transcode_half_frames_device", "lumahip_time_launches"):
        assert known in want, known
    for other in ("lumahip_quantize_array_device", "lumahip_powf_probe_device", "lumahip_mean_luminance_reference_device", "lumahip_device"):
        assert other not in want, other
    named = set(SYMBOLS)
    assert not (named & set(fl.EXEMPT)), "exempt and in the matrix"
    assert want - named - set(fl.EXEMPT) == set(), "entry points with a stride that the matrix leaves out"
    assert (named | set(fl.EXEMPT)) - want == set(), "names that are no entry point with a stride"
    for name, why in fl.EXEMPT.items():
        assert name in ("lumahip_time_launches",) or "probe" in name or len(why) > 40, name
    assert len(set(r.id for r in ROWS)) == len(ROWS)
    # one row per entry point again in either launch shape
    for shape in ("two", "1024"):
        assert set(r.symbol for r in ROWS if r.shape == shape) == set(r.symbol for r in ROWS if r.group != "frames")


def test_matrix_covers_what_the_rows_are_asked_to():
    for sym in SYMBOLS:
        rows = [r for r in PLAIN if r.symbol == sym]
        if rows[0].group == "frames":
            continue
        assert set((r.w, r.h) for r in rows) >= set(fl.HALF_SIZES if rows[0].entry == "half" else fl.SIZES), sym
        if rows[0].entry not in ("light",):
            assert set(r.profile for r in rows) >= ({0, 2, 3}), sym
        if rows[0].entry not in ("light", "pdistortion", "pdistortion_map", "pmoments_map"):
            assert any(r.cs == "ycc" for r in rows), sym
    enc = [r for r in PLAIN if r.entry == "encode"]
    assert 0 < sum(r.stats for r in enc) < len(enc)
    for fam, blocks in (("distortion_map", {16, 32, 64}), ("moments_map", {8, 16, 32, 64})):
        for e in (fam, "t" + fam, "p" + fam):
            assert set(r.block for r in PLAIN if r.entry == e) == blocks, e
    assert all(r.nf == (4 if r.b == "rot" else 1 if "wide" in (r.a or "")[:4] or "wide" in (r.b or "")[:4] else 3) for r in ROWS)
    # one plane-to-plane row with A in the vector layout and B in the byte-wise one
    assert any(r.a == "far16" and r.b == "farodd" for r in PLAIN if r.entry.startswith("p") and r.entry != "plight")


def _vw(w):
    return 4 if w % 4 == 0 else 2


def _frame_facts(row, kind, w, h):
    esz = 2 if fl.halves_of(row) else 4
    n = w * h
    if kind == "planar3":
        # three allocations of PLANAR3_BYTES and more: two of them are at least that far apart, whatever the allocator does
        assert fl.PLANAR3_BYTES >= B32
        fs = n + fl.PAD
        for d in (fl.PLANAR3_BYTES + fl.LEAD, 3 * fl.PLANAR3_BYTES):
            assert fl.colour_planes_ok([0, d, 2 * d], esz, fs, row.nf, n)
        ok, _ = fl.frame_alignment([fl.LEAD] * 3, esz, fs, w)
        assert ok and fs % 2 == 0
        return
    lay = fl.frames_layout(kind, w, h, row.nf, esz)
    nb = len(lay.bases)
    terms = [(f // nb) * lay.fs for f in range(row.nf)]
    assert lay.fs % 2 == 0 and (w % 4 or lay.fs % 4 == 0)
    if kind == "far":
        assert row.nf == 3 and B31 <= terms[1] < B32 <= terms[2]
    else:
        assert row.nf == 4 and terms[3] >= B31 and terms[:3] == [0, 0, 0]
    assert lay.lead >= B31
    for f in range(row.nf):
        for narrow in ("u32", "s32"):
            at = fl.frame_offset(lay, f, narrow)
            for e in (at, at + lay.n3 - 1):
                assert 0 <= e < lay.alloc, (row.id, f, narrow, "outside the allocation")
            limit = B32 if narrow == "u32" else B31
            assert (at != fl.frame_offset(lay, f)) == (terms[f] >= limit), (row.id, f, narrow)
    ptrs = [lay.bases[0] * esz + k * n * esz for k in range(3)]
    ok, al4 = fl.frame_alignment(ptrs, esz, lay.fs, w)
    assert ok and al4 == (w % 4 == 0)
    assert fl.colour_planes_ok(ptrs, esz, lay.fs, row.nf, n)


def _plane_facts(row, kind, w, h):
    lay = fl.planes_layout(kind, w, h, row.profile, row.nf)
    assert fl.check_layout_ok(w, h, row.profile, row.nf, lay.st, lay.pfs), row.id
    assert lay.lead >= B31 and all(o >= lay.lead for o in lay.off)
    odd = kind in ("farodd", "wideodd")
    assert fl.planes_aligned(lay.off, lay.st, lay.pfs, row.profile, _vw(w)) == (not odd), (row.id, "the branch read_planes takes")
    if odd:
        assert all(o % 2 == 1 for o in lay.off)
    if kind in ("far16", "farodd"):
        assert row.nf == 3
        for p in range(3):
            assert B31 <= lay.pfs[p] < B32 <= 2 * lay.pfs[p]
            assert lay.pfs[p] % 2 == (1 if odd else 0) and (odd or lay.pfs[p] % 16 == 0)
    else:
        assert row.nf == 1 and all(s == lay.st[0] for s in lay.st)
        assert lay.st[0] % 2 == (1 if odd else 0) and lay.st[0] < B31
        luma = [r * lay.st[0] for r in range(lay.rows[0])]
        assert any(B31 <= t < B32 for t in luma) and luma[-1] >= B32
        if lay.rows[0] in (70, 72):
            assert luma[31] < B31 <= luma[32] and luma[63] < B32 <= luma[64]
        if row.profile == 3:
            assert lay.rows[1] == lay.rows[2] == lay.rows[0]
    for p in range(3):
        for f in range(row.nf):
            for r in range(lay.rows[p]):
                true = fl.row_offset(lay, p, f, r)
                for narrow in ("u32", "s32"):
                    at = fl.row_offset(lay, p, f, r, narrow, narrow)
                    assert 0 <= at and at + lay.rb[p] <= lay.alloc, (row.id, p, f, r, narrow, "outside the allocation")
                    limit = B32 if narrow == "u32" else B31
                    assert (at != true) == (f * lay.pfs[p] >= limit or r * lay.st[p] >= limit), (row.id, p, f, r, narrow)
    # no two sample regions share a byte
    spans = sorted((fl.row_offset(lay, p, f, r), lay.rb[p]) for p in range(3) for f in range(row.nf) for r in range(lay.rows[p]))
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])), row.id


def _disp_facts(row, kind, w, h):
    lay = fl.disp_layout(w, h, row.nf)
    assert row.nf == 3 and lay.lead >= B31 and lay.st < B31 and lay.st >= 4 * w and lay.dfs >= h * lay.st
    assert lay.dfs >= B32 and any(B31 <= r * lay.st < B32 for r in range(h)) and (h - 1) * lay.st >= B32
    for f in range(row.nf):
        for r in range(h):
            true = fl.disp_offset(lay, f, r)
            for narrow in ("u32", "s32"):
                limit = B32 if narrow == "u32" else B31
                for nf_, nr_ in ((narrow, None), (None, narrow), (narrow, narrow)):
                    at = fl.disp_offset(lay, f, r, nf_, nr_)
                    assert 0 <= at and at + 4 * w <= lay.alloc, (row.id, f, r, nf_, nr_, "outside the allocation")
                    assert (at != true) == ((nf_ and f * lay.dfs >= limit) or (nr_ and r * lay.st >= limit) or False), (row.id, f, r, nf_, nr_)


@pytest.mark.parametrize("group", sorted(set(r.group for r in ROWS)))
def test_layout_facts(group):
    for row in [r for r in ROWS if r.group == group]:
        ops = fl.operands(row)
        assert ops, (row.id, "a row without a far operand")
        for which, _, kind in ops:
            w, h = fl.dims_of(row, which)
            (_frame_facts if kind in fl.FRAME_KINDS else _disp_facts if kind == "fardisp" else _plane_facts)(row, kind, w, h)
        assert fl.live_bytes(row) <= fl.CAP, row.id


def test_sparse_picture():
    m = fl.Sparse(1 << 40)
    m.write((1 << 39) + 5, np.arange(10, dtype=np.uint8))
    got = m.read((1 << 39), 20)
    assert list(got[:5]) == [SENTINEL] * 5 and list(got[5:15]) == list(range(10)) and list(got[15:]) == [SENTINEL] * 5
    with pytest.raises(AssertionError):
        m.read((1 << 40) - 4, 8)
    with pytest.raises(AssertionError):
        m.write(-1, np.zeros(4, dtype=np.uint8))
    assert fl.s32(B31 + 8) == 8 - B31 and fl.u32(B32 + 8) == 8 and fl.s32(B32 + 8) == 8 and fl.u32(B31 + 8) == B31 + 8


def _distinct(arrays, tag):
    for i in range(len(arrays)):
        for j in range(i + 1, len(arrays)):
            assert not np.array_equal(arrays[i], arrays[j]), tag + (i, j, "two frames share a plane")


def _frames_dtype(row, role):
    if role == "in" or row.entry in ("transform", "synth"):
        return np.float16 if fl.halves_of(row) else np.float32
    return np.uint16 if fl.halves_of(row) else np.float32


def _wrong(o, row, inp, exp):
    """the (operand, role, model) names a row was shown to fail; asserts that it fails every model that applies to it"""
    shown = []
    for which, role, kind in fl.operands(row):
        if kind == "planar3":
            continue            # (three pointers, a compact stride: no term of these rows exceeds 32 bits; the facts above hold the rest)
        w, h = fl.dims_of(row, which)
        for narrow in ("u32", "s32"):
            tag = (row.id, which, role, narrow)
            if kind == "fardisp":
                lay = fl.disp_layout(w, h, row.nf)
                for term, (nf_, nr_) in (("frame", (narrow, None)), ("row", (None, narrow))):
                    m = fl.Sparse(lay.alloc)
                    for f in range(row.nf):
                        for r in range(h):
                            m.write(fl.disp_offset(lay, f, r, nf_, nr_), exp[f][r])
                    left = np.stack([np.stack([m.read(fl.disp_offset(lay, f, r), 4 * w) for r in range(h)]) for f in range(row.nf)])
                    assert not np.array_equal(left.reshape(exp.shape), exp), tag + ("passes a writer that narrows the %s term" % term,)
                    assert any(np.all(left[f][r] == SENTINEL) for f in range(row.nf) for r in range(h)), tag + (term, "no true destination stays the sentinel")
            elif kind in fl.FRAME_KINDS:
                dt = _frames_dtype(row, role)
                lay = fl.frames_layout(kind, w, h, row.nf, np.dtype(dt).itemsize)
                if all(fl.frame_offset(lay, f, narrow) == fl.frame_offset(lay, f) for f in range(row.nf)):
                    assert (kind, narrow) == ("rot", "u32"), tag
                    continue
                if role == "in":
                    seen = fl.get_frames(fl.put_frames(lay, inp.frames, dt), lay, w, h, dt, narrow).astype(np.float32)
                    assert not fl.same(fl.expectation(o, row, inp._replace(frames=seen)), exp), tag + ("passes a reader that narrows the frame term",)
                else:
                    left = fl.get_frames(fl.put_frames(lay, exp, dt, narrow), lay, w, h, dt)
                    assert not fl.same(left, np.asarray(exp, dtype=dt)), tag + ("passes a writer that narrows the frame term",)
                    bad = [f for f in range(row.nf) if np.all(left[f].view(np.uint8) == SENTINEL)]
                    assert bad, tag + ("no true destination stays the sentinel",)
            else:
                lay = fl.planes_layout(kind, w, h, row.profile, row.nf)
                term = "frame" if kind in ("far16", "farodd") else "row"
                nf_, nr_ = (narrow, None) if term == "frame" else (None, narrow)
                if role == "in":
                    seen = fl.get_planes(fl.put_planes(lay, getattr(inp, which)), lay, nf_, nr_)
                    assert not fl.same(fl.expectation(o, row, inp._replace(**{which: seen})), exp), tag + ("passes a reader that narrows the %s term" % term,)
                else:
                    left = fl.get_planes(fl.put_planes(lay, exp, nf_, nr_), lay)
                    assert not fl.same(left, exp), tag + ("passes a writer that narrows the %s term" % term,)
                    assert any(np.all(row_ == SENTINEL) for fr in left for p in fr for row_ in p), tag + ("no true destination stays the sentinel",)
            shown.append((which, role, kind, narrow))
    return shown


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_rows_fail_the_wrong_kernels(symbol, oracle_mod):
    o = oracle_mod
    shown = set()
    for row in [r for r in PLAIN if r.symbol == symbol]:
        inp = fl.true_inputs(o, row)
        exp = fl.expectation(o, row, inp)
        if inp.frames is not None and row.nf > 1:
            _distinct([f[c] for f in inp.frames for c in range(3)], (row.id, "frames"))
        for which in ("planes_a", "planes_b"):
            pl = getattr(inp, which)
            if pl is not None and row.nf > 1:
                for p in range(3):
                    _distinct([fr[p] for fr in pl], (row.id, which, p))
        assert fl.same(fl.expectation(o, row, inp), exp), (row.id, "the expectation is not a function of the inputs")
        shown |= set((kind, narrow, role) for (_, role, kind, narrow) in _wrong(o, row, inp, exp))
    # each model that applies to this entry point was shown on at least one of its rows
    kinds = set((kind, role) for r in PLAIN if r.symbol == symbol for (_, role, kind) in fl.operands(r) if kind != "planar3")
    for kind, role in kinds:
        for narrow in ("u32", "s32"):
            if (kind, narrow) != ("rot", "u32"):
                assert (kind, narrow, role) in shown, (symbol, kind, narrow, role)
    if not kinds:
        assert all(k == "planar3" for r in PLAIN if r.symbol == symbol for (_, _, k) in fl.operands(r))


@pytest.mark.parametrize("name", fl.REFUSALS)
def test_refusals_and_the_host_check_that_forms_its_span_in_32_bits(name):
    refused, inside = fl.refusal_facts(name)
    assert refused, "the library's check, restated, accepts this"
    assert inside, "an accepted call would leave the allocation"
    for narrow in ("u32", "s32"):
        wrong, _ = fl.refusal_facts(name, narrow)
        assert not wrong, (narrow, "a 32-bit span still refuses: the case would pass a narrowed check")
