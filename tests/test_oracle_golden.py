"""The oracle against (a) the committed fixtures that tests/golden/make_golden.py generated from the real
reference -- LumaQuantizer (oracle/_ref/libluma_ref.so) and the plane loops LumaEncoder::setChannels /
LumaDecoder::getVpxChannels (oracle/_ref/ref_planes_tool), both compiled unmodified -- and (b), where those builds
are present, the reference itself, live; where they are not, its results on the same seeded inputs as recorded in
tests/golden/ref_live_*.npz.  CPU only; bit-exact everywhere (NaN == NaN)."""
import os

import numpy as np
import pytest

from tests.golden.make_golden import CONFIGS
from tests.support.device import table_for
from tests.support.host import plane_rows


def same(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the live-reference checks: the reference's results on their (seeded) inputs are recorded in
# ---- tests/golden/ref_live_<check>.npz (tests/golden/make_golden.py), so every check runs against the recording; where
# ---- oracle/_ref/ is built it runs live too

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def live_fixture(name):
    return os.path.join(GOLDEN, "ref_live_%s.npz" % name)


class Tape:
    """what the reference returned, call by call: recorded from the live reference (live=True) or replayed from the fixture"""

    def __init__(self, items=None):
        self.live = items is None
        self.items = [] if items is None else items
        self.pos = 0

    def take(self):
        assert self.pos < len(self.items), "more reference calls than the recording holds"
        self.pos += 1
        return self.items[self.pos - 1]

    def done(self):
        assert self.live or self.pos == len(self.items), "fewer reference calls than the recording holds"


def load_tape(name):
    calls = {}
    with np.load(live_fixture(name)) as z:
        for k in z.files:
            i, j = k.split("/")
            calls.setdefault(int(i), {})[int(j)] = z[k]
    return Tape([[c[j] for j in sorted(c)] for _, c in sorted(calls.items())])


def save_tape(name, tape, path=None):
    np.savez_compressed(path or live_fixture(name), **{"%04d/%d" % (i, j): a for i, call in enumerate(tape.items)
                                                       for j, a in enumerate(call)})


class RefQ:
    """o.RefQuantizer through a tape"""

    def __init__(self, o, tape, *cfg):
        self.t = tape
        self.r = o.RefQuantizer(*cfg) if tape.live else None

    def _rec(self, arrays):
        self.t.items.append([np.asarray(a) for a in arrays])

    @property
    def stale(self):
        return self.t.live and not hasattr(self.r.L, "ref_encode_frame")

    @property
    def mapping(self):
        if not self.t.live:
            return self.t.take()[0]
        m = self.r.mapping
        self._rec([m])
        return m

    def transform(self, frame, to_cs, sc=1.0):
        if not self.t.live:
            frame[...] = self.t.take()[0]
            return frame
        self.r.transform(frame, to_cs, sc)
        self._rec([frame.copy()])
        return frame

    def quantize_array(self, a, ch=0):
        if not self.t.live:
            return self.t.take()[0]
        q = self.r.quantize_array(a, ch)
        self._rec([q])
        return q

    def encode(self, frame, sc=1.0, profile=2):
        if not self.t.live:
            c = self.t.take()
            return list(c[:3]), [int(x) for x in c[3]], float(c[4][0])
        planes, st, avg = self.r.encode(frame, sc, profile)
        self._rec(list(planes) + [np.array(st, dtype=np.int32), np.array([avg], dtype=np.float64)])
        return planes, st, avg

    def encode_y_digest(self, frame, sc=1.0, profile=2):
        """the SURVEY digest of the Y plane the reference encodes (the plane itself is not recorded)"""
        if not self.t.live:
            return str(self.t.take()[0])
        from oracle import oracle_py as o
        planes, _, _ = self.r.encode(frame, sc, profile)
        d = o.survey_digest(o.packed_rows(planes[0], 2 * frame.shape[2]))
        self._rec([np.array(d)])
        return d


class RefP:
    """o.RefPlanes through a tape"""

    def __init__(self, o, tape, *cfg, lut_override=None):
        self.t = tape
        self.r = o.RefPlanes(*cfg, lut_override=lut_override) if tape.live else None

    def encode(self, frame, sc=1.0, profile=2, strides=None):
        if not self.t.live:
            c = self.t.take()
            return list(c[:3]), tuple(int(x) for x in c[3]), (float(c[4][0]) if c[4].size else None)
        planes, st, mean = self.r.encode(frame, sc, profile, strides=strides)
        self.t.items.append(list(planes) + [np.array(st, dtype=np.int32),
                                            np.array([] if mean is None else [mean], dtype=np.float64)])
        return planes, st, mean

    def decode(self, planes, strides, w, h, sc=1.0, profile=2, xform=True):
        if not self.t.live:
            return self.t.take()[0]
        d = self.r.decode(planes, strides, w, h, sc, profile, xform=xform)
        self.t.items.append([d])
        return d


def run_live_check(o, check, have_live):
    """the check against the recording, and against the live reference where it is built"""
    tape = load_tape(check.__name__)
    check(o, tape)
    tape.done()
    if have_live:
        check(o, Tape())


@pytest.fixture(scope="module")
def gold(golden_dir):
    return {k: np.load(os.path.join(golden_dir, "ref_%s.npz" % k)) for k in ("luts", "quantize", "transform")}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_lut_matches_reference(oracle_mod, gold, name):
    o = oracle_mod
    cfg = CONFIGS[name]
    m = o.Oracle(*cfg, table=table_for(o, cfg)).mapping
    assert same(m, gold["luts"][name])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_quantize_dequantize_match_reference(oracle_mod, gold, name):
    o = oracle_mod
    cfg = CONFIGS[name]
    qq = o.Oracle(*cfg, table=table_for(o, cfg))
    g = gold["quantize"]
    got0 = np.array([qq.quantize(float(v), 0) for v in g[name + "_in0"]])
    assert np.array_equal(got0.astype(np.uint16), g[name + "_q0"])
    got1 = np.array([qq.quantize(float(v), 1) for v in g[name + "_in1"]])
    assert np.array_equal(got1.astype(np.uint16), g[name + "_q1"])
    codes = np.arange(-2, 2 ** cfg[1] + 2, dtype=np.float32)
    assert same([qq.dequantize(float(c), 0) for c in codes], g[name + "_dq0"])
    ccodes = np.arange(0, 2 ** cfg[3], dtype=np.float32)
    assert same([qq.dequantize(float(c), 1) for c in ccodes], g[name + "_dq1"])


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("sc", [1.0, 20.0, 0.25])
def test_transform_matches_reference(oracle_mod, gold, name, sc):
    o = oracle_mod
    cfg = CONFIGS[name]
    qq = o.Oracle(*cfg, table=table_for(o, cfg))
    t = gold["transform"]
    f = t["input"].copy()
    qq.transform(f, True, sc)
    assert same(f, t["%s_fwd_sc%g" % (name, sc)])
    g = t["%s_inv_in_sc%g" % (name, sc)].copy()
    qq.transform(g, False, sc)
    assert same(g, t["%s_inv_sc%g" % (name, sc)])


def check_random_frames(o, tape):
    rng = np.random.default_rng(1234)
    for name, cfg in CONFIGS.items():
        qq = o.Oracle(*cfg, table=table_for(o, cfg))
        r = RefQ(o, tape, *cfg)
        assert same(qq.mapping, r.mapping)
        f = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), size=(3, 32, 64))).astype(np.float32)
        f[:, 0, :4] = [[0, np.nan, np.inf, -3], [1, 1, 1, 2], [2, 1, 1, 1]]
        for sc in (1.0, 3.5):
            a, b = f.copy(), f.copy()
            qq.transform(a, True, sc)
            r.transform(b, True, sc)
            assert same(a, b), (name, sc)
            vals = a[0].ravel()
            assert np.array_equal(np.array([qq.quantize(float(v), 0) for v in vals[:512]]), r.quantize_array(vals[:512], 0))
            assert np.array_equal(np.array([qq.quantize(float(v), 1) for v in a[1].ravel()[:512]]),
                                  r.quantize_array(a[1].ravel()[:512], 1))
            a2, b2 = np.abs(a).copy(), np.abs(a).copy()
            qq.transform(a2, False, sc)
            r.transform(b2, False, sc)
            assert same(a2, b2), (name, sc, "inv")


def test_live_reference_random_frames(oracle_mod):
    """oracle vs the reference .so on seeded random frames, all colour spaces, both directions"""
    run_live_check(oracle_mod, check_random_frames, oracle_mod.have_ref())


def check_extreme_inputs(o, tape):
    from tests.golden.make_golden import extreme_frame
    f = extreme_frame()
    for name, cfg in CONFIGS.items():
        qq = o.Oracle(*cfg, table=table_for(o, cfg))
        r = RefQ(o, tape, *cfg)
        for sc in (1.0, 20.0):
            a, b = f.copy(), f.copy()
            with np.errstate(all="ignore"):
                qq.transform(a, True, sc)
                r.transform(b, True, sc)
            assert same(a, b), (name, sc)
            for profile in (2, 3):
                pa, _, _ = qq.encode(f.copy(), sc, profile)
                pb, _, _ = r.encode(f.copy(), sc, profile)
                assert all(np.array_equal(x, y) for x, y in zip(pa, pb)), (name, sc, profile)


def test_live_reference_extreme_inputs(oracle_mod):
    """inf - inf patterns, +-FLT_MAX, NaNs of both signs in every position, -0, denormals: the oracle's forward transform
    and whole-frame encode against the REAL LumaQuantizer, every configuration, preScaling 1 and 20"""
    run_live_check(oracle_mod, check_extreme_inputs, oracle_mod.have_ref())


def test_roundtrip_decode_of_encode(oracle_mod):
    """encode -> decode through the plane layout reproduces the dequantized Lu'v' of every pixel"""
    o = oracle_mod
    qq = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    f = o.synth_frame(64, 32, frame=3)
    src = f.copy()
    for profile in (0, 1, 2, 3):
        qp = o.Oracle(o.PTF_PQ, 8 if profile < 2 else 11, o.CS_LUV, 8, 1e4, 0.005)
        g = src.copy()
        planes, strides, _ = qp.encode(g, 1.0, profile)
        out = qp.decode(planes, strides, 64, 32, 1.0, profile)
        assert out.shape == src.shape and np.all(np.isfinite(out))
        # luminance survives within one quantisation step of the PTF
        Y = 0.212656 * src[0] + 0.715158 * src[1] + 0.072186 * src[2]
        Yd = 0.212656 * out[0] + 0.715158 * out[1] + 0.072186 * out[2]
        assert np.median(np.abs(np.log2(Yd / Y))) < (0.2 if profile < 2 else 0.02)


def check_whole_frame_encode(o, tape):
    for name, cfg in CONFIGS.items():
        qq = o.Oracle(*cfg, table=table_for(o, cfg))
        r = RefQ(o, tape, *cfg)
        assert not r.stale, "oracle/_ref/libluma_ref.so predates ref_encode_frame: rebuild it"
        f = o.synth_frame(96, 40, frame=2)
        f[:, 0, :3] = [[np.nan, 0, -1], [1, 0, 5], [1, 0, 2]]
        for profile in (0, 1, 2, 3):
            a, _, avga = qq.encode(f.copy(), 1.0, profile)
            b, _, avgb = r.encode(f.copy(), 1.0, profile)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (name, profile)
            assert (np.isnan(avga) and np.isnan(avgb)) or avga == avgb
    r = RefQ(o, tape, o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    assert r.encode_y_digest(o.test_frame(1280, 720), 1.0, 2) == "e0ff09731298e8f6"


def test_live_reference_whole_frame_encode(oracle_mod):
    """the oracle's whole-frame encode against the REAL LumaQuantizer driven through the harness's plane loop
    (oracle/ref_harness.cpp: ref_encode_frame), every profile; PSI/HDR-VDP included (tables compiled into the
    reference).  Also reproduces the SURVEY Y-plane digest with the real quantizer."""
    run_live_check(oracle_mod, check_whole_frame_encode, oracle_mod.have_ref())


# ---- the plane loops: LumaEncoder::setChannels / setVpxChannel (src/luma_encoder.cpp:196-201,260-317) and
# ---- LumaDecoder::getVpxChannels (src/luma_decoder.cpp:205-240), pinned by the reference's own compiled code

def _plane_keys(gp):
    return sorted(k[:-3] for k in gp.files if k.endswith("_in"))


def test_plane_loops_match_reference_fixtures(oracle_mod, golden_dir):
    """lo_pack_plane / lo_unpack_plane (and the whole-frame drivers built on them) against what the reference's own
    setChannels / getVpxChannels produced: four configurations x the profiles their bit depth allows x two frame sizes,
    NaN / zero / negative / huge pixels, decoder-chosen odd strides, out-of-range codes."""
    o = oracle_mod
    gp = np.load(os.path.join(golden_dir, "ref_planes.npz"))
    keys = _plane_keys(gp)
    assert len(keys) == 16 and {int(k[-1]) for k in keys} == {0, 1, 2, 3}
    for key in keys:
        name, size, prof = key.rsplit("_", 2)
        cfg = CONFIGS[name]
        w, h = (int(x) for x in size.split("x"))
        profile = int(prof[1])
        sc = 20.0 if cfg[2] == o.CS_YCBCR else 1.0
        qq = o.Oracle(*cfg, table=table_for(o, cfg))
        planes, st, mean = qq.encode(gp[key + "_in"].copy(), sc, profile)
        assert tuple(st) == tuple(gp[key + "_stride"])
        rb = [plane_rows(w, h, profile, p)[1] for p in range(3)]
        for p in range(3):
            ref = gp[key + "_plane%d" % p]
            assert np.array_equal(planes[p][:, :rb[p]], ref[:, :rb[p]]), (key, p)
            assert np.all(ref[:, rb[p]:] == 0xA5)            # the reference writes the samples and nothing else
        printed = float(gp[key + "_mean"][0])
        if not np.isnan(printed):                             # the warning fired: avg <= 1 (src/luma_encoder.cpp:313-316)
            assert mean <= 1.0 and abs(mean - printed) <= 5e-7 * max(1.0, abs(printed))   # %f prints 6 decimals
        dst = tuple(int(x) for x in gp[key + "_dec_stride"])
        dpl = [gp[key + "_dec_plane%d" % p] for p in range(3)]
        assert same(qq.unpack(dpl, dst, w, h, profile), gp[key + "_unpacked"]), key
        assert same(qq.decode(dpl, dst, w, h, sc, profile), gp[key + "_decoded"]), key


def test_plane_digests_from_the_reference_loops(oracle_mod, golden_dir):
    """testFrame 1280x720 through encode -> decode: digests recorded from the reference's own loops, incl. the decode
    direction and the 4:4:4 profile that SURVEY.md 8(c) lacks; the profile-2 Y/U/V digests equal the survey's."""
    import json
    o = oracle_mod
    dig = json.load(open(os.path.join(golden_dir, "ref_plane_digests.json")))
    assert (dig["testframe_1280x720_p2"]["Y"], dig["testframe_1280x720_p2"]["U"], dig["testframe_1280x720_p2"]["V"]) == \
        ("e0ff09731298e8f6", "4c410839cf4228cc", "28868357f4a5e5e5")
    qq = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    for profile in (2, 3):
        d = dig["testframe_1280x720_p%d" % profile]
        planes, st, _ = qq.encode(o.test_frame(1280, 720), 1.0, profile)
        cb = 2560 if profile == 3 else 1280
        assert o.survey_digest(o.packed_rows(planes[0], 2560)) == d["Y"]
        assert o.survey_digest(o.packed_rows(planes[1], cb)) == d["U"]
        assert o.survey_digest(o.packed_rows(planes[2], cb)) == d["V"]
        assert o.survey_digest(qq.decode(planes, st, 1280, 720, 1.0, profile)) == d["decoded"]


def check_plane_loops(o, tape):
    rng = np.random.default_rng(77)
    for name, cfg in CONFIGS.items():
        qq = o.Oracle(*cfg, table=table_for(o, cfg))
        rp = RefP(o, tape, *cfg)
        sc = 20.0 if cfg[2] == o.CS_YCBCR else 1.0
        for (w, h) in ((6, 2), (50, 22)):
            f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(3, h, w))).astype(np.float32)
            f[:, 0, :3] = [[np.nan, 0, -2], [1, 0, 5], [1, 0, 2]]
            for profile in (0, 1, 2, 3):
                bps = 2 if profile > 1 else 1
                _, hs, st0, _ = o.plane_geometry(w, h, profile)
                st = tuple(s + 2 * p + 1 for p, s in enumerate(st0))             # odd, different per plane
                a, _, _ = qq.encode(f.copy(), sc, profile)
                b, _, _ = rp.encode(f.copy(), sc, profile, strides=st)
                rb = [plane_rows(w, h, profile, p)[1] for p in range(3)]
                for p in range(3):
                    assert np.array_equal(a[p][:, :rb[p]], b[p][:, :rb[p]]), (name, w, h, profile, p)
                    assert np.all(b[p][:, rb[p]:] == 0xA5)
                garbage = [np.where(rng.random(x.shape) < 0.02, rng.integers(0, 256, x.shape), x).astype(np.uint8) for x in b]
                assert same(qq.unpack(garbage, st, w, h, profile), rp.decode(garbage, st, w, h, sc, profile, xform=False)), (name, profile)
                assert same(qq.decode(garbage, st, w, h, sc, profile), rp.decode(garbage, st, w, h, sc, profile)), (name, profile)
    # dark frame: the reference prints its warning; its number is the sequential fp32 sum / (w*h)
    qq = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    rp = RefP(o, tape, o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    dark = (o.synth_frame(320, 180, frame=1) * np.float32(1e-5)).astype(np.float32)
    _, _, mo = qq.encode(dark.copy(), 1.0, 2)
    _, _, mr = rp.encode(dark.copy(), 1.0, 2)
    assert mr is not None and abs(mo - mr) <= 5e-7
    # table override (LumaDecoder::initialize, src/luma_decoder.cpp:121-122)
    lut = qq.mapping.copy()
    lut[100:110] *= np.float32(1.01)
    q2 = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    q2.overwrite_mapping(lut)
    rp2 = RefP(o, tape, o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005, lut_override=lut[:-1])   # getSize() = maxVal floats
    lut_eff = lut.copy()
    lut_eff[-1] = qq.mapping[-1]
    q2.overwrite_mapping(lut_eff)
    planes, st, _ = q2.encode(o.synth_frame(64, 32, frame=9), 1.0, 2)
    assert same(q2.decode(planes, st, 64, 32, 1.0, 2), rp2.decode(planes, st, 64, 32, 1.0, 2))


def test_live_reference_plane_loops(oracle_mod):
    """oracle vs the reference's compiled setChannels / getVpxChannels on seeded frames: every configuration, every
    profile, ragged sizes, odd strides, an attachment-434 style table override.  Also the mean luminance the reference
    prints in its warning (sequential fp32 sum) against the oracle's."""
    run_live_check(oracle_mod, check_plane_loops, oracle_mod.have_ref_planes())
