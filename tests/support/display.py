"""The comparison the display-decode tests hold an RGBA image to, stated once and usable without a GPU: numpy alone.

display_t        the player's display transform (oracle/luma_oracle.c lo_display_transform) in float64, kept as t = 255 v + 0.5
                 BEFORE the floor; floor(t) is the oracle's byte
display_fp32     the same formula in numpy float32, operation by operation as the kernel's epilogue writes it (the CPU check of EPS)
check_rgba       what an image must satisfy against t (see its docstring, which also derives EPS); exempt_share: what it cannot judge
informative      the two conditions on a reference image: enough distinct codes, few saturated pixels
display_frames   input frames that meet them

Helpers here assert with an explicit message: pytest rewrites `assert` in test modules only."""
import numpy as np

# the four parameter sets (do_tmo, ldr_sim, exposure, gamma) of test_gpu_parity.py test_decode_display_transform
DISPLAY_SETS = [(0, 0, 1.0, 2.2), (1, 0, 0.02, 2.2), (0, 1, 1.0, 1.8), (1, 1, 4.0, 2.4)]

# ---- EPS: how far from a rounding boundary fp32 and float64 may disagree (derived in check_rgba's docstring)
U = 2.0 ** -24                      # one rounding of an fp32 operation, relative
_A = 6.0 * np.log(2.0)              # error of v per unit of |p|, in units of U: two chained powers, 3 ln2 each
_B = 2.0 + 7.53                     # the part that does not depend on p, in units of U (gamma >= 1)
_P = np.linspace(-60.0, 0.0, 60001)
ERR_T = 255.0 * float(np.max(2.0 ** _P * (_A * np.abs(_P) + _B))) * U + 512.0 * U     # bound on |t_fp32 - t_float64|
SAFETY = 4.0
EPS = SAFETY * ERR_T                # 7.0e-4
MAX_EXEMPT = 0.01                   # at most this share of a case's pixels may lie within EPS of a boundary


def display_t(rgb, exposure=1.0, gamma=2.2, do_tmo=0, ldr_sim=0):
    """(h, w, 3) float64: t = 255 v + 0.5 of lo_display_transform for decoded linear RGB (3, h, w) float32, every step in float64 and
    in lo_display_transform's order, with its comparisons (a NaN fails `v > 0`, `f < 256` and `f > 1`)"""
    v = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if ldr_sim:
            f = np.floor(256.0 * v)
            f = np.where(f < 256.0, f, 256.0)
            f = np.where(f > 1.0, f, 1.0)
            v = exposure * f / 256.0
        else:
            v = v * exposure
        if do_tmo:
            vn = np.power(np.where(v > 0.0, v, 0.0), 0.8)
            v = vn / (vn + np.power(0.8, 0.8))
        v = np.power(np.where(v > 0.0, v, 0.0), 1.0 / gamma)
        v = np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))
    return np.moveaxis(255.0 * v + 0.5, 0, -1)


def display_bytes(t):
    """(h, w, 4) uint8: the oracle's image from t"""
    out = np.full(t.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.floor(t).astype(np.uint8)
    return out


def display_fp32(rgb, exposure=1.0, gamma=2.2, do_tmo=0, ldr_sim=0, tmo_const=None):
    """(h, w, 4) uint8: the epilogue of dec_process (luma_kernels.hpp) in numpy float32 -- one fp32 rounding per operation, the
    powers as exp2(y * log2(x)) with log2 and exp2 rounded to fp32 from float64 (an ideal v_log_f32 / v_exp_f32).
    tmo_const: another tone-curve constant than pow(0.8, 0.8) (the host test's wrong image)"""
    f32 = np.float32

    def fpow(x, y):
        with np.errstate(all="ignore"):
            lg = np.log2(x.astype(np.float64)).astype(f32)
            return np.exp2((f32(y) * lg).astype(f32).astype(np.float64)).astype(f32)

    v = np.asarray(rgb, dtype=f32)
    with np.errstate(all="ignore"):
        if ldr_sim:
            v = f32(exposure) * np.fmax(f32(1), np.fmin(f32(256), np.floor(f32(256) * v))) * f32(1.0 / 256.0)
        else:
            v = v * f32(exposure)
        if do_tmo:
            vn = fpow(np.fmax(v, f32(0)), 0.8)
            v = vn / (vn + f32(0.83650957 if tmo_const is None else tmo_const))
        v = fpow(np.fmax(v, f32(0)), f32(1) / f32(gamma))
        v = np.fmin(np.fmax(v, f32(0)), f32(1))
        codes = (v * f32(255) + f32(0.5)).astype(np.uint32)
    out = np.full(codes.shape[1:] + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.moveaxis(codes, 0, -1)
    return out


def boundary_distance(t):
    """distance of t from the nearest integer: where floor(t) changes"""
    return np.abs(t - np.round(t))


def exempt_share(t):
    """the share of the pixels of t with a channel within EPS of a rounding boundary: what check_rgba cannot judge"""
    return float(np.mean((boundary_distance(np.asarray(t)) < EPS).any(axis=-1)))


def check_rgba(rgba, t, tag=()):
    """Holds an (h, w, 4) uint8 image to t = display_t(...) of the same pixels.  Asserts
      * alpha is 255 everywhere;
      * every code equals floor(t), or differs from it by one where t lies within EPS of an integer -- the rounding boundary -- and
        then towards that boundary: floor(t) - 1 just above it, floor(t) + 1 just below it;
      * at most MAX_EXEMPT of the pixels have a channel within EPS of a boundary (those the comparison cannot judge).
    Returns (that share, the number of codes that differ, the largest boundary distance at which one differs -- 0.0 without any).

    EPS.  The kernel evaluates in fp32 what t is in float64: x = v_in * exposure (or the LDR form: one rounded product, the floor
    and the division by 256 are exact), optionally s = vn / (vn + c) with vn = pow(x, 0.8), then v = pow(., 1 / gamma),
    t = v * 255 + 0.5.  Its pow is the fast one, exp2(y * log2(x)); take 1 ulp = 2 U for each of the two instructions and U = 2^-24
    for the rounding of every other operation.  With v = 2^p:
      one power   log2 x carries 2 U relative, the product with y U more, so the exponent is off by 3 U |p|, which exp2 turns into
                  3 ln2 |p| U relative in v; exp2 itself adds 2 U, the rounding of x adds U / gamma.
      two powers  the first one gives vn = 2^p1 with 3 ln2 |p1| U + 2 U + 0.8 U; s = vn / (vn + c) passes that on times
                  c / (vn + c) and adds 3 U (the sum, the quotient, c's own rounding).  |p1| c / (vn + c) <= |p| gamma + 0.35: for
                  vn < 1, s <= vn / c bounds |p1| by |p| gamma + 0.26, and for vn >= 1, p1 c / (2^p1 + c) <= 0.35.  Raised to
                  1 / gamma: 3 ln2 |p| U + (0.73 + 5.8) U / gamma on top of the one-power terms.
    For gamma >= 1 that is (6 ln2 |p| + 2 + 7.53) U relative in v, and 255 times it plus 2 * 256 U for the last product and sum in
    t.  2^p (A |p| + B) over p <= 0 has its maximum at p = 0 here (A / B < ln 2): ERR_T = 255 * 9.53 U + 512 U = 1.75e-4.  The
    instructions' accuracy is documented, not measured here, hence EPS = SAFETY * ERR_T = 4 * 1.75e-4 = 7.0e-4: 0.14 % of uniformly
    spread values of t, 0.42 % of pixels with three channels.

    Checked on the CPU (tests/test_display_host.py): display_fp32 against float64 on display_frames' values, 3 x 49152 pixels per
    parameter set, disagrees only within 1.08e-4 of a boundary with the tone curve (10 or 11 codes per frame) and within 5.9e-6
    without it (0 to 2 codes); under the LDR simulation not at all.  On the display tests' largest case (1280 x 720 through the
    YCbCr oracle, tone curve) 195 codes, the farthest 1.13e-4 from a boundary.  Under ERR_T, as it must be: its log2 and exp2 are
    correctly rounded, half of what is assumed above."""
    rgba, t = np.asarray(rgba), np.asarray(t)
    assert rgba.dtype == np.uint8 and rgba.shape == t.shape[:2] + (4,) and t.shape[2] == 3, tag + ("shapes", rgba.shape, t.shape)
    assert np.all(rgba[..., 3] == 255), tag + ("alpha is not 255 everywhere",)
    want = np.floor(t).astype(np.int64)
    d = rgba[..., :3].astype(np.int64) - want
    frac = t - np.floor(t)
    dist = np.minimum(frac, 1.0 - frac)
    ok = (d == 0) | ((d == -1) & (frac < EPS)) | ((d == 1) & (1.0 - frac < EPS))
    if not np.all(ok):
        y, x, c = (int(i[0]) for i in np.nonzero(~ok))
        raise AssertionError(tag + ("%d codes off" % np.count_nonzero(~ok), "first at row %d column %d channel %d" % (y, x, c),
                                    "got %d" % rgba[y, x, c], "t = %.6f" % t[y, x, c]))
    share = exempt_share(t)
    assert share <= MAX_EXEMPT, tag + ("%.4f of the pixels lie within EPS of a rounding boundary: these inputs judge too little" % share,)
    return share, int(np.count_nonzero(d)), float(dist[d != 0].max()) if np.any(d) else 0.0


def reachable_codes(exposure, gamma, do_tmo, ldr_sim, peak=np.inf):
    """how many codes the transform can produce from values in [0, peak]: the codes up to peak's own, or with the LDR simulation
    what its input levels 1 .. min(256, floor(256 peak)) map to"""
    if not ldr_sim:
        top = display_t(np.full((3, 1, 1), min(peak, 3e38), dtype=np.float32), exposure, gamma, do_tmo, 0)
        return int(np.floor(top[0, 0, 0])) + 1
    n = int(min(256.0, max(1.0, np.floor(256.0 * min(peak, 1.0)))))
    levels = (np.arange(1, n + 1, dtype=np.float64) / 256.0).astype(np.float32)   # floor(256 v) = 1 .. n
    t = display_t(np.broadcast_to(levels, (3, 1, n)), exposure, gamma, do_tmo, 1)
    return int(np.unique(np.floor(t[..., 0])).size)


def informative(t, exposure, gamma, do_tmo, ldr_sim, tag=(), levels=256):
    """the conditions on a reference image, from float64 alone: per channel at least 200 distinct codes and fewer than 20 % of the
    pixels at 0 or 255.  Where fewer codes than 250 can appear at all the first bound is 80 % of what can: under the LDR simulation
    only reachable_codes(...) codes exist (201 for the third parameter set, 87 for the fourth), and a caller passes in `levels`
    what else limits its case (how many distinct values the decoded channel holds, the codes below its quantizer's peak).
    Returns (fewest distinct codes of a channel, largest saturated share)."""
    codes = np.floor(t).astype(np.int64).reshape(-1, 3)
    can = min(int(levels), reachable_codes(exposure, gamma, do_tmo, ldr_sim))
    need = 200 if can >= 250 else int(0.8 * can)
    distinct = min(int(np.unique(codes[:, c]).size) for c in range(3))
    sat = max(float(np.mean((codes[:, c] == 0) | (codes[:, c] == 255))) for c in range(3))
    assert distinct >= need, tag + ("a channel shows %d distinct codes, fewer than %d" % (distinct, need),)
    assert sat < 0.20, tag + ("%.3f of a channel's pixels are at 0 or 255" % sat,)
    return distinct, sat


def display_frames(rng, nf, w, h, exposure, gamma=2.2, do_tmo=0, ldr_sim=0, peak=np.inf, top=1.04):
    """nf distinct (3, h, w) float32 frames (w, h even) whose display image spreads over the codes under the parameter set.  Colours
    are drawn per 2 x 2 block, so that a 4:2:0 stream's averaged chroma keeps their spread, and every pixel is moved by up to 2 %.
    Half the blocks are uniform in the display code -- the inverse of the transform, up to code 258 or to what the value `top` gives
    under the tone curve, which comes near 1 only far above 1 (code 253 at 150) --, half log-uniform over 2^-13 .. 1.04 before the
    exposure.  Under the LDR simulation, which cuts the values to 256 levels of [0, 1] before the exposure applies, the first half
    is uniform in [0, 1.04].  peak: the largest value the stream's quantizer holds after its preScaling; values above it are cut."""
    shape = (nf, 3, h // 2, w // 2)
    c = 0.8 ** 0.8
    if ldr_sim:
        x = rng.uniform(0.0, 1.04, size=shape)
    else:
        s = (rng.uniform(0.0, 258.0, size=shape) / 255.0) ** gamma
        if do_tmo:
            s = np.minimum(s, top ** 0.8 / (top ** 0.8 + c))
            x = (c * s / (1.0 - s)) ** 1.25
        else:
            x = s
    x = np.where(rng.random(size=shape) < 0.5, x, np.exp2(rng.uniform(-13.0, np.log2(1.04), size=shape)))
    x = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) * rng.uniform(0.98, 1.02, size=(nf, 3, h, w))
    return np.minimum(x if ldr_sim else x / exposure, peak).astype(np.float32)
