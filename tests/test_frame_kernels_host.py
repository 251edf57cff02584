"""What tests/test_gpu_frame_kernels.py relies on, checked without a GPU: the encode matrix names the 68 k_encode instantiations its
docstring says, every call form meets every (colour space, search mode), the frames of a launch are distinct and their oracle planes
informative, and the comparison of a call's plane buffers with the oracle's planes (tests/support/frame_kernels.py planes_problem)
rejects each error planted into them -- as does the comparison of the statistics."""
import numpy as np
import pytest

from tests.support import frame_kernels as fk
from tests.support.host import GAP, SENTINEL, layout, plane_rows, planes_from_frames


def test_the_matrix_covers_what_the_docstring_says():
    """16 k_encode<CS, SUB, VW, LM> per colour space -- LM 3, 4, 7 by VW 4 and 2, LM 0 and 2 by VW 2, each 4:2:0 and 4:4:4 -- and the four
    LM 5 kernels of YCbCr: 68; each of the three further call forms on every (colour space, mode); statistics on both sides of every
    mode; the 8-bit profiles on every colour space"""
    rows = fk.encode_matrix()
    assert len({r[0] for r in rows}) == len(rows)
    kernels = {fk.kernel_of(cs, mode, profile, w, lm5) for (_, cs, mode, _, _, profile, w, _, _, _, _, lm5) in rows}
    assert len(kernels) == 68
    for cs in (fk.LUV, fk.RGB, fk.YCC, fk.XYZ):
        assert len({k for k in kernels if k[0] == cs and k[3] != 5}) == 16
    assert {k for k in kernels if k[3] == 5} == {(fk.YCC, sub, vw, 5) for sub in (True, False) for vw in (4, 2)}
    assert len({(r[1], r[2], r[10]) for r in rows}) == 4 * 5 * 3
    assert {(r[2], r[9]) for r in rows} == {(m, s) for m in fk.MODES for s in (True, False)}
    assert {(r[1], r[5]) for r in rows if r[5] < 2} == {(cs, p) for cs in fk.SPACES for p in (0, 1)}
    # the row's statistics decide the YCbCr kernel: LM 5 only without them
    assert all(not r[9] for r in rows if r[11]) and all(r[9] for r in rows if r[1] == fk.YCC and r[2] == 3 and not r[11])


def test_the_frames_of_a_launch_are_distinct_and_hold_the_special_values():
    for (w, h) in fk.SIZES:
        f = fk.frames(w, h)
        assert f.shape == (fk.NF, 3, h, w)
        for a in range(fk.NF):
            for b in range(a + 1, fk.NF):
                assert np.count_nonzero(f[a] != f[b]) > 0.9 * f[a].size * (0.5 if (w, h) == (64, 32) else 1.0)
        assert np.isnan(f).any() == ((w, h) == (64, 32)) and np.isinf(f).any() == ((w, h) == (64, 32))
        assert bool((f < 0).any()) == ((w, h) == (64, 32))
        h16 = fk.frames(w, h, halves=True)
        assert h16.dtype == np.float16 and np.array_equal(np.isnan(h16), np.isnan(f))


def _reference_keys():
    """every (configuration, profile, w, h, preScaling, halves) the GPU file asks the oracle for at 64x32 and 258x6"""
    keys = set()
    for (_, cs, mode, cfg, _, profile, w, h, sc, _, form, _) in fk.encode_matrix():
        keys.add((cfg, profile, w, h, sc, False))
        if "f16" in form:
            keys.add((cfg, profile, w, h, sc, True))
    for cs, (_, _, _, _, scs) in fk.SPACES.items():
        for profile in range(4):
            for (w, h) in fk.SIZES:
                keys.add((fk.config(cs, fk.PQ, 11) if profile > 1 else fk.pq8(cs), profile, w, h, scs[-1], False))
    return sorted(k for k in keys if (k[2], k[3]) != (6, 4))


def test_the_expected_planes_are_informative(oracle_mod):
    """at least 64 distinct sample values in every expected plane of every frame, U and V different; the smallest count is printed"""
    least = min(fk.informative(fk.expected(oracle_mod, cfg, profile, w, h, sc, halves)[1], w, h, profile, (cfg, profile, w, h, sc, halves))
                for (cfg, profile, w, h, sc, halves) in _reference_keys())
    print("the fewest distinct sample values of an expected plane: %d" % least)
    assert least >= fk.MIN_DISTINCT


# ---- planted errors
LAYOUTS = [pytest.param(2, 64, 32, "wide", 0, id="p2-64x32-wide"), pytest.param(3, 258, 6, "odd", 1, id="p3-258x6-odd-base1"),
           pytest.param(0, 64, 32, "wide", 4, id="p0-64x32-wide-base4"), pytest.param(1, 6, 4, "odd", 1, id="p1-6x4-odd-base1")]


def _built(o, profile, w, h, kind, base):
    cfg = fk.config(fk.LUV, fk.PQ, 11) if profile > 1 else fk.pq8(fk.LUV)
    _, exp, _ = fk.expected(o, cfg, profile, w, h, 1.0)
    st, gap = (fk.wide_layout(w, h, profile), GAP) if kind == "wide" else fk.odd_layout(w, h, profile)
    bufs = planes_from_frames(exp, w, h, profile, st, "sentinel", gap, base)
    return exp, st, gap, bufs


@pytest.mark.parametrize("profile,w,h,kind,base", LAYOUTS)
def test_the_plane_comparison_rejects_each_planted_error(oracle_mod, profile, w, h, kind, base):
    exp, st, gap, good = _built(oracle_mod, profile, w, h, kind, base)
    args = (exp, w, h, profile, st, gap, base)
    assert fk.planes_problem(good, *args) is None
    if kind == "odd":
        assert all(s % 2 == 1 for s in st) and all(x % 2 == 1 for x in layout(w, h, profile, st, gap)[2])
    hs, size, pfs = layout(w, h, profile, st, gap)
    bps = 2 if profile > 1 else 1
    nf = len(exp)

    def planted(change):
        bufs = [b.copy() for b in good]
        change(bufs)
        return fk.planes_problem(bufs, *args)

    # one sample off by one in the last row and column of the last frame, per plane
    for p in range(3):
        rb = plane_rows(w, h, profile, p)[1]
        at = base + (nf - 1) * pfs[p] + (hs[p] - 1) * st[p] + rb - bps

        def off_by_one(bufs, p=p, at=at):
            bufs[p][at] ^= 1
        assert "differ" in planted(off_by_one), p
        if bps == 2:
            def swapped(bufs, p=p, at=at):
                # (a sample whose bytes differ: the first such from the end of the last row)
                k = at
                while bufs[p][k] == bufs[p][k + 1]:
                    k -= 2
                bufs[p][k], bufs[p][k + 1] = bufs[p][k + 1], bufs[p][k]
            assert "differ" in planted(swapped), p

    def uv(bufs):
        bufs[1], bufs[2] = bufs[2], bufs[1]
    assert "differ" in planted(uv)

    def frames_exchanged(bufs):
        for p in range(3):
            a = bufs[p][base: base + size[p]].copy()
            bufs[p][base: base + size[p]] = bufs[p][base + 2 * pfs[p]: base + 2 * pfs[p] + size[p]]
            bufs[p][base + 2 * pfs[p]: base + 2 * pfs[p] + size[p]] = a
    assert "frame 0" in planted(frames_exchanged)

    # one byte outside the samples
    for p in range(3):
        rb = plane_rows(w, h, profile, p)[1]
        places = {"a row's padding": base + pfs[p] + (hs[p] - 1) * st[p] + rb, "the last byte of a row's padding": base + pfs[p] + st[p] - 1,
                  "a gap": base + size[p], "the last byte of a gap": base + pfs[p] - 1, "behind the last frame": base + (nf - 1) * pfs[p] + size[p],
                  "the last byte of the buffer": good[p].size - 1}
        if base:
            places["in front of the base"] = base - 1
            places["the first byte of the buffer"] = 0
        for what, at in places.items():
            def stray(bufs, p=p, at=at):
                assert bufs[p][at] == SENTINEL, (what, "is no padding byte")
                bufs[p][at] = 0
            assert "outside the samples" in planted(stray), (p, what)


def test_the_statistics_comparison_rejects_each_planted_error(oracle_mod):
    o = oracle_mod
    cfg = fk.config(fk.RGB, fk.PQ, 11)
    plain, special = fk.frames(258, 6)[0], fk.frames(64, 32)[0]
    want = fk.expected_stats(o, cfg, plain, 1.0)
    assert np.isfinite(want[0]) and want[1] > 0
    good = (np.float32(want[0]), want[1], want[2])
    assert fk.stats_problem(good, want) is None
    assert fk.stats_problem((np.float32(want[0] * (1 + 5e-5)), want[1], want[2]), want) is None
    assert "sum" in fk.stats_problem((np.float32(want[0] * (1 + 2e-4)), want[1], want[2]), want)
    assert "sum" in fk.stats_problem((np.float32("nan"), want[1], want[2]), want)
    assert "min" in fk.stats_problem((good[0], np.nextafter(want[1], np.float32(0)), want[2]), want)
    assert "min" in fk.stats_problem((good[0], want[1], np.nextafter(want[2], np.float32(np.inf))), want)
    # the frame with the special values: RGB's channel 0 holds NaN, +inf and -inf -- the sum is NaN, min and max pass over the NaN
    ws = fk.expected_stats(o, cfg, special, 1.0)
    assert np.isnan(ws[0]) and ws[1] == -np.inf and ws[2] == np.inf
    assert fk.stats_problem((np.float32("nan"), ws[1], ws[2]), ws) is None
    assert "sum" in fk.stats_problem((np.float32(1.0), ws[1], ws[2]), ws)
    assert "min" in fk.stats_problem((np.float32("nan"), np.float32("nan"), ws[2]), ws)
