"""The pure builders of tests/support/host.py, which every code-plane GPU test builds its device inputs with: the plane geometry
against figures written out by hand, the host byte buffers of from_frames in both padding modes, perturb's footprint, and the guard
check behind a map.  numpy only."""
import numpy as np
import pytest

from tests.support.host import GAP, GUARD, OUT_FILL, SENTINEL, layout, map_words, nwords, perturb, plane_rows, planes_from_frames

# profile -> ((rows, row bytes) of the luma plane, of a chroma plane)
GEOMETRY = {(34, 18): {0: ((18, 34), (9, 17)), 1: ((18, 34), (18, 34)), 2: ((18, 68), (9, 34)), 3: ((18, 68), (18, 68))},
            (6, 4): {0: ((4, 6), (2, 3)), 1: ((4, 6), (4, 6)), 2: ((4, 12), (2, 6)), 3: ((4, 12), (4, 12))}}


def test_plane_rows_are_the_hand_written_figures():
    for (w, h), by_profile in GEOMETRY.items():
        for profile, (luma, chroma) in by_profile.items():
            assert [plane_rows(w, h, profile, p) for p in range(3)] == [luma, chroma, chroma], (w, h, profile)
    assert plane_rows(5, 3, 2, 1) == (2, 6) and plane_rows(5, 3, 2, 0) == (3, 10)    # odd sizes round the chroma planes up
    hs, size, pfs = layout(6, 4, 2, (16, 8, 8))
    assert (hs, size, pfs) == ([4, 2, 2], [64, 16, 16], [64 + GAP, 16 + GAP, 16 + GAP])


@pytest.mark.parametrize("wider", [0, 3])
@pytest.mark.parametrize("padding", ["sentinel", "source"])
def test_from_frames_host_buffers(padding, wider):
    w, h, profile, st, nf = 6, 4, 2, (16, 8, 8), 2
    rows, rb = [4, 2, 2], [12, 6, 6]
    frames = []
    for f in range(nf):   # samples 1 .. 0x7F, row padding 0x80 + row: neither is the sentinel
        fr = []
        for p in range(3):
            a = np.empty((rows[p], st[p] + wider), dtype=np.uint8)
            a[:, :rb[p]] = 1 + (np.arange(rows[p] * rb[p]).reshape(rows[p], rb[p]) + 17 * f + 5 * p) % 0x7F
            a[:, rb[p]:] = 0x80 + np.arange(rows[p])[:, None]
            fr.append(a)
        frames.append(fr)
    bufs = planes_from_frames(frames, w, h, profile, st, padding)
    for p in range(3):
        assert bufs[p].dtype == np.uint8 and bufs[p].shape == (nf * (rows[p] * st[p] + GAP),)
        b = bufs[p].reshape(nf, rows[p] * st[p] + GAP)
        assert np.all(b[:, rows[p] * st[p]:] == SENTINEL), "the gap behind every frame's plane"
        for f in range(nf):
            got = b[f, :rows[p] * st[p]].reshape(rows[p], st[p])
            assert np.array_equal(got[:, :rb[p]], frames[f][p][:, :rb[p]])
            if padding == "sentinel":
                assert np.all(got[:, rb[p]:] == SENTINEL)
            else:
                assert np.array_equal(got[:, rb[p]:], frames[f][p][:, rb[p]:st[p]]) and np.all(got[:, rb[p]:] >= 0x80)


def test_from_frames_refuses_an_unknown_padding_and_short_source_rows():
    fr = [np.zeros((4, 16), np.uint8), np.zeros((2, 8), np.uint8), np.zeros((2, 8), np.uint8)]
    with pytest.raises(ValueError):
        planes_from_frames([fr], 6, 4, 2, (16, 8, 8), "zeros")
    with pytest.raises(ValueError):   # rows of 16 bytes cannot fill rows 19 bytes apart with their own padding
        planes_from_frames([fr], 6, 4, 2, (19, 11, 11), "source")
    assert len(planes_from_frames([fr], 6, 4, 2, (19, 11, 11), "sentinel")[0]) == 4 * 19 + GAP


@pytest.mark.parametrize("profile", [0, 1, 2, 3])
def test_perturb_leaves_every_byte_outside_the_row_bytes(profile):
    w, h = 34, 18
    rng = np.random.default_rng(profile)
    planes = []
    for p in range(3):
        rows, rb = plane_rows(w, h, profile, p)
        planes.append(rng.integers(0, 256, size=(rows, rb + 7), dtype=np.uint8))
    before = [a.copy() for a in planes]
    got = perturb(np.random.default_rng(1), planes, w, h, profile, frac=0.5)
    for p in range(3):
        rb = plane_rows(w, h, profile, p)[1]
        assert np.array_equal(planes[p], before[p]), "the argument itself is left alone"
        assert got[p].shape == before[p].shape and np.array_equal(got[p][:, rb:], before[p][:, rb:])
        assert not np.array_equal(got[p][:, :rb], before[p][:, :rb])


def test_map_words_checks_the_guard_words():
    nf, w, h, block = 2, 34, 18, 16
    n = nwords(nf, w, h, block)
    assert n == 2 * 3 * 2 * 12
    buf = np.full(n + GUARD, OUT_FILL, dtype=np.int64)
    buf[:n] = np.arange(n)
    m = map_words(buf, nf, w, h, block)
    assert m.shape == (2, 2, 3, 3, 4) and m.dtype == np.uint64 and m.ravel().tolist() == list(range(n))
    for k in (n, n + GUARD - 1):
        bad = buf.copy()
        bad[k] = 0
        with pytest.raises(AssertionError, match="guard words"):
            map_words(bad, nf, w, h, block)
