"""ExrInterface (include/exr_interface.h) without OpenEXR: the C++ reader / writer against an independent
restatement of the OpenEXR scan-line layout in numpy + zlib (tests/support/exr.py).  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.support.exr import attr, read_exr_py, write_exr_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lumahdrv_amd", "lib")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    import lumahdrv_amd
    lumahdrv_amd.build_library()
    exe = str(tmp_path_factory.mktemp("exr") / "exr_tool")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "exr_tool.cpp"), "-o", exe, "-L" + LIB, "-lluma_hip", "-llumahip",
                    "-Wl,-rpath," + LIB], check=True)
    return exe


def cpp_read(tool, path, tmp):
    outp = str(tmp / "out.f32")
    subprocess.run([tool, "read", path, outp], check=True)
    raw = open(outp, "rb").read()
    w, h = struct.unpack_from("<II", raw, 0)
    return np.frombuffer(raw, dtype="<f4", offset=8).reshape(3, h, w)


def eq(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_half_conversion_matches_ieee(tool):
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(20000).astype(np.float32) * 1e3,
                        np.exp(rng.uniform(-25, 12, 20000)).astype(np.float32),
                        np.array([0, -0.0, 65504, 65519.99, 65520, 1e9, -1e9, 6e-8, 5.9e-8, 2.98e-8, 2.99e-8, 6.1e-5, np.inf,
                                  -np.inf, np.nan, 1.0009765625, 1.00048828125, 1.00146484375], dtype=np.float32)])
    r = subprocess.run([tool, "half"], input=v.tobytes(), capture_output=True, check=True)
    got = np.frombuffer(r.stdout, dtype="<u2")
    with np.errstate(over="ignore"):
        exp = v.astype(np.float16).view(np.uint16)
    nan = np.isnan(v)
    assert np.array_equal(got[~nan], exp[~nan])
    assert np.all((got[nan] & 0x7C00) == 0x7C00) and np.all((got[nan] & 0x3FF) != 0)


@pytest.mark.parametrize("comp", [0, 2, 3])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_reader_against_python_writer(tool, tmp_path, comp, dtype):
    rng = np.random.default_rng(comp * 7 + len(dtype))
    h, w = 37, 50
    ch = {n: np.exp(rng.uniform(-8, 11.5, (h, w))).astype(dtype) for n in "RGBA"}
    path = str(tmp_path / "in.exr")
    write_exr_py(path, ch, comp, x0=-3, y0=5)
    got = cpp_read(tool, path, tmp_path)
    with np.errstate(over="ignore"):
        for i, n in enumerate("RGB"):
            assert eq(got[i], ch[n].astype(np.float16).astype(np.float32)), n   # Imf::Rgba: everything through half


def test_single_channel_replication_and_errors(tool, tmp_path):
    h, w = 8, 6
    g = np.linspace(0.1, 900, h * w).reshape(h, w).astype(np.float16)
    p = str(tmp_path / "g.exr")
    write_exr_py(p, {"G": g}, 3)
    got = cpp_read(tool, p, tmp_path)
    assert all(eq(got[i], g.astype(np.float32)) for i in range(3))     # WRITE_G: replicated to all three planes
    p2 = str(tmp_path / "y.exr")
    write_exr_py(p2, {"Y": g}, 0)
    r = subprocess.run([tool, "read", p2, str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 1 and "luminance only" in r.stderr             # src/exr_interface.cpp:145
    open(str(tmp_path / "junk.exr"), "wb").write(b"not an exr file at all")
    r = subprocess.run([tool, "read", str(tmp_path / "junk.exr"), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 1


@pytest.mark.parametrize("comp,as_float", [(0, 0), (2, 0), (3, 0), (3, 1)])
def test_writer_against_python_reader_and_roundtrip(tool, tmp_path, comp, as_float):
    rng = np.random.default_rng(11)
    h, w = 40, 33
    f = np.exp(rng.uniform(-6, 11, (3, h, w))).astype(np.float32)
    f[0, 0, :4] = [0, 70000, -2.5, 1e-9]
    src = str(tmp_path / "src.f32")
    open(src, "wb").write(struct.pack("<II", w, h) + f.tobytes())
    out = str(tmp_path / "w.exr")
    subprocess.run([tool, "write", src, out, str(comp), str(as_float)], check=True)
    chans, c = read_exr_py(out)
    assert c == comp and sorted(chans) == ["B", "G", "R"]
    with np.errstate(over="ignore"):
        exp = f if as_float else f.astype(np.float16).astype(np.float32)
        for i, n in enumerate("RGB"):
            assert eq(chans[n], exp[i])
        back = cpp_read(tool, out, tmp_path)
        assert eq(back, f.astype(np.float16).astype(np.float32))            # reading narrows to half either way


def test_reader_survives_corrupted_files_under_sanitizers(tmp_path):
    """mutation fuzzing (truncation, bit flips, stomped 32- and 64-bit fields, random spans) of valid files of every
    compression the reader implements (NONE, RLE, ZIPS, ZIP from the writer; PIZ and PXR24 from the Python encoders),
    reader built with ASan + UBSan: every attempt either decodes or raises LumaException"""
    exe = str(tmp_path / "exr_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "exr_fuzz.cpp"),
                    os.path.join(ROOT, "lumahdrv_amd", "csrc", "facade", "exr_interface.cpp"),
                    os.path.join(ROOT, "lumahdrv_amd", "csrc", "facade", "exr_codecs.cpp"), "-o", exe, "-lz"], check=True)
    # seeds for the compressions only the reader implements
    rng = np.random.default_rng(8)
    smooth = (np.add.outer(np.arange(40), np.arange(29)) // 5).astype(np.float16)
    seeds = []
    for comp, nm in ((4, "piz.exr"), (5, "pxr24.exr")):
        sp = str(tmp_path / nm)
        write_exr_py(sp, {"R": smooth, "G": rng.uniform(0, 9, smooth.shape).astype(np.float16) // 1, "B": (smooth * 3).astype(np.float16)}, comp)
        seeds.append(sp)
    r = subprocess.run([exe, str(tmp_path), "400"] + seeds, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok ")
    d, rj = [int(x.split("=")[1]) for x in r.stdout.split()[1:3]]
    assert d + rj == 2400 and rj > 300


def test_wrapping_chunk_offsets_and_empty_attributes_are_rejected(tmp_path):
    """Directed cases from the round-1 review, reader + CLI built with ASan + UBSan (no GPU library needed: exr_tool links
    the reader source directly): a 64-bit chunk offset that wraps `p + n` (0xFFFFFFFFFFFFFFFE), offsets at / past the end
    of the file, and a zero-size `compression` / `lineOrder` attribute as the last bytes of a truncated file."""
    exe = str(tmp_path / "exr_tool_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "exr_tool.cpp"),
                    os.path.join(ROOT, "lumahdrv_amd", "csrc", "facade", "exr_interface.cpp"),
                    os.path.join(ROOT, "lumahdrv_amd", "csrc", "facade", "exr_codecs.cpp"), "-o", exe, "-lz"], check=True)
    rng = np.random.default_rng(4)
    chans = {n: rng.uniform(0, 100, (18, 20)).astype(np.float16) for n in "RGB"}
    for comp in (0, 2, 3):
        good = str(tmp_path / ("good%d.exr" % comp))
        write_exr_py(good, chans, comp)
        d = bytearray(open(good, "rb").read())
        p = 8
        while d[p] != 0:                                  # walk the attributes to the offset table
            p = d.index(b"\0", p) + 1
            p = d.index(b"\0", p) + 1
            p += 4 + struct.unpack_from("<i", d, p)[0]
        table = p + 1
        r = subprocess.run([exe, "read", good, str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for v in (0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFF8, 0x8000000000000000, len(d), len(d) - 1, len(d) - 7, 1 << 32):
            m = bytearray(d)
            struct.pack_into("<Q", m, table, v)
            bad = str(tmp_path / "bad.exr")
            open(bad, "wb").write(m)
            r = subprocess.run([exe, "read", bad, str(tmp_path / "o.bin")], capture_output=True, text=True)
            assert r.returncode == 1 and "LumaException" in r.stderr, (comp, hex(v), r.returncode, r.stderr[-600:])
    # zero-size compression / lineOrder attribute at the very end of the data
    for name, typ in (("compression", "compression"), ("lineOrder", "lineOrder")):
        hdr = struct.pack("<ii", 20000630, 2) + attr(name, typ, b"")
        bad = str(tmp_path / "short.exr")
        open(bad, "wb").write(hdr)
        r = subprocess.run([exe, "read", bad, str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "LumaException" in r.stderr, (name, r.returncode, r.stderr[-600:])


@pytest.mark.parametrize("comp", [4, 5])
def test_reader_decodes_piz_and_pxr24(tool, tmp_path, comp):
    """PIZ (wavelet + LUT + Huffman) and PXR24 (24-bit byte-plane delta + zlib) chunks written by the Python encoders
    above: odd sizes across block boundaries, HALF and FLOAT channels, few distinct values (14-bit wavelet path and
    Huffman run-length codes) and noise (16-bit wavelet path), an alpha channel, a single-channel file, a data window
    that does not start at the origin."""
    rng = np.random.default_rng(comp)
    cases = []
    h, w = 45, 37                                            # two PIZ blocks (32 + 13), three PXR24 blocks
    smooth = (np.add.outer(np.arange(h), np.arange(w)) // 7).astype(np.float16)
    cases.append(({"R": smooth, "G": (smooth * 2).astype(np.float16), "B": np.zeros((h, w), np.float16)}, "smooth half"))
    noise = {n: rng.uniform(0, 6e4, (70, 300)).astype(np.float16) for n in "RGBA"}       # > 16384 distinct words per block
    cases.append((noise, "noise half + alpha"))
    # a ramp through > 16384 distinct half codes per block that still compresses: the 16-bit wavelet path of the decoder
    idx = np.arange(64 * 300, dtype=np.int64).reshape(64, 300) % (32 * 300)
    ramp = {"R": (3 * idx).astype(np.uint16).view(np.float16), "G": (3 * idx + 1).astype(np.uint16).view(np.float16),
            "B": (32768 + 3 * idx + 2).astype(np.uint16).view(np.float16)}
    assert all(np.isfinite(v.astype(np.float32)).all() for v in ramp.values())
    cases.append((ramp, "ramp, 16-bit wavelet"))
    f24 = {n: (rng.uniform(1e-3, 1e4, (h, w)).astype(np.float32).view(np.uint32) & 0xFFFFFF00).view(np.float32) for n in "RGB"}
    cases.append((f24, "float"))
    mixed = {"R": rng.uniform(0, 100, (33, 9)).astype(np.float16), "G": f24["G"][:33, :9].copy(), "B": rng.uniform(0, 5, (33, 9)).astype(np.float16)}
    cases.append((mixed, "mixed half / float"))
    cases.append(({"G": rng.uniform(0, 50, (5, 3)).astype(np.float16)}, "single channel, tiny"))
    for chans, what in cases:
        p = str(tmp_path / "c.exr")
        write_exr_py(p, chans, comp, x0=3, y0=-2)
        got = cpp_read(tool, p, tmp_path)
        names = [n for n in "RGB" if n in chans]
        src = names if len(names) == 3 else [names[0]] * 3
        with np.errstate(over="ignore"):
            for i, n in enumerate(src):
                assert eq(got[i], chans[n].astype(np.float16).astype(np.float32)), (comp, what, n)
    # the compressed path was really taken (not the stored-raw fallback) for the compressible cases
    write_exr_py(str(tmp_path / "s.exr"), cases[0][0], comp)
    assert os.path.getsize(str(tmp_path / "s.exr")) < 45 * 37 * 6 // 2
    if comp == 4:
        write_exr_py(str(tmp_path / "r.exr"), ramp, comp)
        assert os.path.getsize(str(tmp_path / "r.exr")) < 64 * 300 * 6 * 0.8
        assert len({int(x) for v in ramp.values() for x in v[:32].view(np.uint16).reshape(-1)}) > 16384


def test_reader_on_a_file_written_by_openexr(tool, tmp_path):
    """tests/golden/openexr_written_16x16_rgba_half.exr is a genuine OpenEXR-library file (CPython's test-suite sample
    `imghdrdata/python.exr`, 16x16 RGBA HALF, uncompressed, increasing-y) -- the one real-world EXR in the build image.
    The C++ reader and the Python restatement of the layout must agree on it."""
    path = os.path.join(ROOT, "tests", "golden", "openexr_written_16x16_rgba_half.exr")
    ch, comp = read_exr_py(path)
    assert comp == 0 and sorted(ch) == ["A", "B", "G", "R"] and ch["R"].shape == (16, 16)
    got = cpp_read(tool, path, tmp_path)
    for i, n in enumerate("RGB"):
        assert eq(got[i], ch[n])
    assert float(np.max(got)) > 0.0
