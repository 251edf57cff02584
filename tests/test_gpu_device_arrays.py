"""The device forms of the stand-alone calls, bit for bit against the oracle -- needs an MI355X.

lumahip_transform_color_space_device (Context.transform_frames_device): several frames per launch, a frame stride with a gap, both
directions, and a launch whose pixel pairs exceed the grid's threads, so that k_transform's grid-stride loop runs.
lumahip_quantize_array_device / lumahip_dequantize_array_device: channels 0, 1 and 2 -- the table for channel 0 and for every channel of
RGB / XYZ, the colour quantizer otherwise (lumahip_decode.hip array_launch) -- from one value to more than the grid's threads."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.golden.make_golden import CONFIGS, extreme_frame, special_frame  # noqa: E402
from tests.support.device import L, ctx, dev, table_for  # noqa: E402,F401  (L is the module fixture)
from tests.support.host import ERR_ARG, same_bits  # noqa: E402

NAN_BITS = 0x7FC0C3C3          # what the gaps and guards hold: a NaN no kernel here produces
GUARD = 16

_ctx, _orc = {}, {}


def context(L, name):
    if name not in _ctx:
        _ctx[name] = ctx(L, CONFIGS[name])
    return _ctx[name]


def oracle(o, L, name):
    if name not in _orc:
        cfg = CONFIGS[name]
        _orc[name] = o.Oracle(*cfg, table=table_for(o, cfg))
        assert same_bits(L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]), _orc[name].mapping), "the library's table is not the oracle's"
    return _orc[name]


def filled(n):
    """n floats on the device, every one the sentinel NaN"""
    import torch
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device=dev())


def bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- lumahip_transform_color_space_device
XF_CONFIGS = ["pq11_luv8", "pq12_rgb", "pq10_ycbcr10", "linear12_xyz"]
XW, XH, XNF, XGAP = 66, 34, 3, 6


def xf_frames(o, orc, golden_dir, name, sc, to_cs):
    """three (3, 34, 66) frames: forward, linear RGB with the golden generator's special and extreme values in frame 1; inverse, the
    oracle's forward output of those with the fixture's `*_inv_in_*` values (what getVpxChannels produces) in the corner of frame 1"""
    rng = np.random.default_rng(66 * 34)
    f = np.exp(rng.uniform(np.log(1e-4), np.log(3e4), size=(XNF, 3, XH, XW))).astype(np.float32)
    f[1, :, :8, :16] = special_frame(8, 16)
    f[1, :, 8:12, :32] = extreme_frame(4, 32)
    f[2] = o.synth_frame(XW, XH, frame=5)
    if to_cs:
        return f
    for k in range(XNF):
        orc.transform(f[k], True, sc)
    t = np.load(os.path.join(golden_dir, "ref_transform.npz"))
    f[1, :, 16:24, :16] = t["%s_inv_in_sc%g" % (name, sc)]
    return f


def on_device(frames, gap):
    """frames f at f * (3 w h + gap) floats of a buffer that holds the sentinel NaN elsewhere, and GUARD floats behind the last gap"""
    import torch
    nf, n3 = frames.shape[0], frames[0].size
    fs = n3 + gap
    host = np.full(nf * fs + GUARD, NAN_BITS, dtype=np.uint32)
    host[:nf * fs].reshape(nf, fs)[:, :n3] = frames.reshape(nf, n3).view(np.uint32)
    return torch.from_numpy(host.view(np.int32)).to(dev()), host, fs


def frames_of(buf, nf, fs, shape):
    """(the frames, whether every float outside them still is the sentinel)"""
    a = bits(buf)
    body = a[:nf * fs].reshape(nf, fs)
    n3 = int(np.prod(shape))
    intact = bool(np.all(body[:, n3:] == NAN_BITS) and np.all(a[nf * fs:] == NAN_BITS))
    return np.ascontiguousarray(body[:, :n3]).view(np.float32).reshape((nf,) + shape), intact


@pytest.mark.parametrize("sc", [1.0, 20.0, 0.25])
@pytest.mark.parametrize("to_cs", [True, False], ids=["forward", "inverse"])
@pytest.mark.parametrize("name", XF_CONFIGS)
def test_transform_frames_device(L, oracle_mod, golden_dir, name, to_cs, sc):
    import torch
    c, orc = context(L, name), oracle(oracle_mod, L, name)
    src = xf_frames(oracle_mod, orc, golden_dir, name, sc, to_cs)
    buf, _, fs = on_device(src, XGAP)
    assert fs == 3 * XW * XH + 6
    c.transform_frames_device(buf.data_ptr(), fs, XNF, XW, XH, to_cs, sc)
    torch.cuda.synchronize()
    got, intact = frames_of(buf, XNF, fs, (3, XH, XW))
    assert intact, (name, to_cs, sc, "the gaps between the frames or the floats behind the last one changed")
    for f in range(XNF):
        assert same_bits(got[f], orc.transform(src[f].copy(), to_cs, sc)), (name, to_cs, sc, f)
    assert same_bits(got[0], c.transform_color_space(src[0].copy(), to_cs, sc)), (name, to_cs, sc, "the one-frame host form")


@pytest.mark.parametrize("to_cs", [True, False], ids=["forward", "inverse"])
@pytest.mark.parametrize("name", XF_CONFIGS)
def test_transform_grid_stride_loop(L, oracle_mod, name, to_cs):
    """three frames of 1024 x 384: 589824 pixel pairs for at most num_cu * 8 workgroups of 256 threads -- 524288 threads on 256 CUs, the
    most an MI355X has -- so every launch goes round the loop; the first and the last frame against the oracle in full"""
    import torch
    o = oracle_mod
    c, orc = context(L, name), oracle(o, L, name)
    w, h, nf, sc = 1024, 384, 3, 20.0
    assert (w * h // 2) * nf > 256 * 8 * 256
    src = np.stack([o.synth_frame(w, h, frame=21 + k) for k in range(nf)])
    if not to_cs:
        for k in (0, nf - 1):
            orc.transform(src[k], True, sc)
    buf, _, fs = on_device(src, XGAP)
    c.transform_frames_device(buf.data_ptr(), fs, nf, w, h, to_cs, sc)
    torch.cuda.synchronize()
    got, intact = frames_of(buf, nf, fs, (3, h, w))
    assert intact, (name, to_cs)
    for f in (0, nf - 1):
        assert same_bits(got[f], orc.transform(src[f].copy(), to_cs, sc)), (name, to_cs, f)
    assert not same_bits(got[1], src[1]), (name, to_cs, "the middle frame was not transformed")


def test_transform_refused_calls_write_nothing(L, oracle_mod):
    import torch
    c = context(L, "pq11_luv8")
    src = np.ones((2, 3, 34, 66), dtype=np.float32)
    buf, host, fs = on_device(src, XGAP)
    for what, args in (("an odd pixel count", (buf.data_ptr(), fs, 2, 33, 17)), ("a pointer misaligned by 4", (buf.data_ptr() + 4, fs, 2, 66, 34)),
                       ("an odd frame stride", (buf.data_ptr(), fs + 1, 2, 66, 34)), ("no frames", (buf.data_ptr(), fs, 0, 66, 34)),
                       ("an empty frame", (buf.data_ptr(), fs, 2, 0, 34)), ("a null pointer", (None, fs, 2, 66, 34))):
        with pytest.raises(L.LumaHipError) as e:
            c.transform_frames_device(*args, True, 1.0)
        assert e.value.code == ERR_ARG, what
        torch.cuda.synchronize()
        assert np.array_equal(bits(buf), host), what


# ---- lumahip_quantize_array_device / lumahip_dequantize_array_device
ARRAY_CONFIGS = XF_CONFIGS + ["hdrvdp12_luv10"]
# num_cu is not exposed: 2^20 + 3 values are more than num_cu * 8 * 256 threads on any MI355X (256 CUs: 524288), so the grid-stride
# loop of both kernels runs, with a ragged end
MORE_THAN_THE_GRID = (1 << 20) + 3
NS = [1, 2, 255, 257, MORE_THAN_THE_GRID]
_expect = {}


def lut_channel(cfg, ch):
    return ch == 0 or cfg[2] in (1, 3)          # CS_RGB, CS_XYZ: the table for every channel


def quantize_inputs(orc, cfg, ch):
    rng = np.random.default_rng(31 + ch)
    edge = np.array([0.0, -0.0, -1.0, -1e-30, -3e38, 1e-45, 3e38, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)
    if lut_channel(cfg, ch):
        m = orc.mapping
        mids = ((m[:-1].astype(np.float64) + m[1:].astype(np.float64)) / 2).astype(np.float32)
        body = [m, np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf)), mids,
                np.nextafter(mids, np.float32(-np.inf)), np.nextafter(mids, np.float32(np.inf)),
                np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 2048)).astype(np.float32)]
    else:
        maxc = float((1 << cfg[3]) - 1)
        steps = (np.arange(-2, 2 * int(maxc) + 5, dtype=np.float64) / (2 * maxc)).astype(np.float32)     # the codes and the rounding points
        body = [steps, np.nextafter(steps, np.float32(-np.inf)), np.nextafter(steps, np.float32(np.inf)),
                rng.uniform(-0.2, 1.2, 2048).astype(np.float32)]
    return np.concatenate(body + [edge])


def dequantize_inputs(orc, cfg, ch):
    lut = lut_channel(cfg, ch)
    top = (1 << cfg[1]) - 1 if lut else (1 << cfg[3]) - 1
    v = np.concatenate([np.arange(-2, top + 3, dtype=np.float32),
                        np.array([0.5, 1.999, top - 0.5, top + 0.5, -0.5, 1e9, -1e9, np.inf, -np.inf], dtype=np.float32)])
    # (the reference indexes its table with (int)val: a NaN there is undefined in C, so only the colour quantizer is given one)
    return v if lut else np.concatenate([v, np.array([np.nan, -np.nan], dtype=np.float32)])


def expectation(o, L, name, ch, quant):
    """(inputs, the oracle's value for each), computed once per (configuration, channel, direction)"""
    key = (name, ch, quant)
    if key not in _expect:
        orc, cfg = oracle(o, L, name), CONFIGS[name]
        v = quantize_inputs(orc, cfg, ch) if quant else dequantize_inputs(orc, cfg, ch)
        fn = orc.quantize if quant else orc.dequantize
        _expect[key] = (v, np.array([fn(float(x), ch) for x in v], dtype=np.float32))
    return _expect[key]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("quant", [True, False], ids=["quantize", "dequantize"])
@pytest.mark.parametrize("name", ARRAY_CONFIGS)
def test_array_calls(L, oracle_mod, name, quant, n):
    import torch
    c = context(L, name)
    for ch in (0, 1, 2):
        base, exp_base = expectation(oracle_mod, L, name, ch, quant)
        # n values starting somewhere else for every n; the longest takes every input, over and over
        idx = (np.arange(n) + 7919 * n) % base.size
        assert n < base.size or np.unique(idx).size == base.size
        vals = base[idx]
        x = torch.from_numpy(vals).to(dev())
        out = filled(n + GUARD)
        if quant:
            c.quantize_array_device(x.data_ptr(), out.data_ptr(), n, ch)
        else:
            c.dequantize_array_device(x.data_ptr(), out.data_ptr(), n, ch)
        torch.cuda.synchronize()
        got = bits(out)
        assert np.all(got[n:] == NAN_BITS), (name, quant, ch, n, "the floats behind the output changed")
        assert np.array_equal(bits(x), vals.view(np.uint32)), (name, quant, ch, n, "the input changed")
        g, e = got[:n].view(np.float32), exp_base[idx]
        bad = np.nonzero(~((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))))[0]
        assert bad.size == 0, (name, "quantize" if quant else "dequantize", ch, n, "%d differ" % bad.size, "first: input %r got %r expected %r"
                               % (vals[bad[0]], g[bad[0]], e[bad[0]]))


def test_array_calls_refuse_null_pointers_and_accept_no_values(L, oracle_mod):
    import torch
    c = context(L, "pq11_luv8")
    out = filled(GUARD)
    for call in (c.quantize_array_device, c.dequantize_array_device):
        for args in ((None, out.data_ptr(), 4), (out.data_ptr(), None, 4)):
            with pytest.raises(L.LumaHipError) as e:
                call(*args, 0)
            assert e.value.code == ERR_ARG
        call(out.data_ptr(), out.data_ptr(), 0, 0)          # n == 0: nothing to do, no launch
    torch.cuda.synchronize()
    assert np.all(bits(out) == NAN_BITS)
