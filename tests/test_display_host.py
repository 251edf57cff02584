"""tests/support/display.py without a GPU: its float64 transform gives the oracle's bytes, check_rgba accepts what it should and
rejects what it must, and the derived EPS covers a numpy float32 evaluation of the kernel's formula on the display tests' own
inputs."""
import numpy as np
import pytest

from tests.golden.make_golden import extreme_frame, special_frame
from tests.support.display import (DISPLAY_SETS, EPS, ERR_T, MAX_EXEMPT, boundary_distance, check_rgba, display_bytes, display_fp32,
                                   display_frames, display_t, informative, reachable_codes)

W, H = 256, 192


def reference(k, seed=3):
    """(floats, t) of one frame under parameter set k, with the golden generator's special and extreme values in its first rows"""
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[k]
    f = display_frames(np.random.default_rng(seed + k), 1, W, H, exposure, gamma, do_tmo, ldr_sim, top=150.0)[0]
    f[:, :8, :16] = special_frame(8, 16)
    f[:, 8:12, :32] = extreme_frame(4, 32)
    return f, display_t(f, exposure, gamma, do_tmo, ldr_sim)


def test_eps_is_the_derived_figure():
    assert ERR_T == pytest.approx(1.75e-4, rel=0.01) and EPS == 4 * ERR_T and EPS < 1e-3 and MAX_EXEMPT == 0.01


@pytest.mark.parametrize("k", range(4))
def test_float64_transform_gives_the_oracles_bytes(oracle_mod, k):
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[k]
    f, t = reference(k)
    exp = oracle_mod.display_transform(f, exposure, gamma, do_tmo, ldr_sim)
    assert np.array_equal(display_bytes(t), exp)
    share, differ, far = check_rgba(exp, t, (k,))
    assert differ == 0 and far == 0.0 and share <= MAX_EXEMPT
    informative(t, exposure, gamma, do_tmo, ldr_sim, (k,))


def test_reachable_codes_under_the_ldr_simulation():
    assert reachable_codes(1.0, 2.2, 0, 0) == 256
    assert reachable_codes(1.0, 1.8, 0, 1) == 201 and reachable_codes(4.0, 2.4, 1, 1) == 87


@pytest.mark.parametrize("k", range(4))
def test_fp32_evaluation_disagrees_only_next_to_a_boundary(k):
    """the CPU check of the derivation: the kernel's formula in numpy float32 (correctly rounded log2 / exp2) differs from float64
    only within ERR_T of a rounding boundary, so it passes check_rgba with room; the figures are in check_rgba's docstring"""
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[k]
    worst = 0.0
    for seed in (3, 40, 77):
        f, t = reference(k, seed)
        got = display_fp32(f, exposure, gamma, do_tmo, ldr_sim)
        share, differ, far = check_rgba(got, t, (k, seed))
        worst = max(worst, far)
        print("set %d seed %d: exempt share %.4f, %d codes differ, farthest %.2e from a boundary (ERR_T %.2e, EPS %.2e)"
              % (k, seed, share, differ, far, ERR_T, EPS))
    assert worst < ERR_T


def test_check_rgba_has_teeth():
    do_tmo, ldr_sim, exposure, gamma = DISPLAY_SETS[1]
    f, t = reference(1)
    good = display_bytes(t)
    check_rgba(good, t)
    frac = t - np.floor(t)
    interior = (np.floor(t) >= 2) & (np.floor(t) <= 253)
    # +-1 on a pixel within EPS of its boundary, on the side of that boundary: accepted
    above = np.argwhere((frac < EPS) & interior)
    below = np.argwhere((1.0 - frac < EPS) & interior)
    far = np.argwhere((boundary_distance(t) > 0.25) & interior)
    assert len(above) and len(below) and len(far)
    for idx, step in ((above[0], -1), (below[0], +1)):
        img = good.copy()
        img[tuple(idx)] = int(good[tuple(idx)]) + step
        share, differ, dist = check_rgba(img, t)
        assert differ == 1 and 0.0 <= dist < EPS
        img[tuple(idx)] = int(good[tuple(idx)]) - step           # the other side of the same pixel: rejected
        with pytest.raises(AssertionError, match="codes off"):
            check_rgba(img, t)
    # +1 far from a boundary, +-2 anywhere (next to a boundary included)
    for idx, step in ((far[0], +1), (far[0], -1), (far[1], +2), (far[1], -2), (above[0], -2), (below[0], +2)):
        img = good.copy()
        img[tuple(idx)] = int(good[tuple(idx)]) + step
        with pytest.raises(AssertionError, match="codes off"):
            check_rgba(img, t)
    # two swapped channels, alpha 254 on one pixel
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(good[..., [1, 0, 2, 3]], t)
    img = good.copy()
    img[H - 1, W - 1, 3] = 254
    with pytest.raises(AssertionError, match="alpha"):
        check_rgba(img, t)
    # a slightly wrong exposure, the tone curve's constant without its power: both in float64 and in float32
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(display_bytes(display_t(f, exposure * (1 + 2.0 ** -10), gamma, do_tmo, ldr_sim)), t)
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(display_fp32(f, exposure * (1 + 2.0 ** -10), gamma, do_tmo, ldr_sim), t)
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(display_fp32(f, exposure, gamma, do_tmo, ldr_sim, tmo_const=0.8), t)
    # a wrong gamma, a missing tone curve
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(display_bytes(display_t(f, exposure, 2.4, do_tmo, ldr_sim)), t)
    with pytest.raises(AssertionError, match="codes off"):
        check_rgba(display_bytes(display_t(f, exposure, gamma, 0, ldr_sim)), t)


def test_check_rgba_refuses_inputs_that_judge_too_little():
    """an image whose values all sit on a rounding boundary is not a test"""
    t = np.full((8, 8, 3), 100.0 + EPS / 2)
    with pytest.raises(AssertionError, match="judge too little"):
        check_rgba(display_bytes(t), t)
    with pytest.raises(AssertionError, match="distinct codes"):
        informative(t, 1.0, 2.2, 0, 0)
    dark = np.full((8, 8, 3), 0.5) + np.arange(64).reshape(8, 8, 1) * 0.001
    with pytest.raises(AssertionError):
        informative(dark, 1.0, 2.2, 0, 0)
