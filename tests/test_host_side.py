"""CPU-only checks of the product's host side: the C-ABI library loads and exports every symbol that
include/lumahip.h declares, the host LUT builder reproduces the reference's tables, the facade compiles and
links, and without a GPU every compute entry point fails loudly (no CPU fallback)."""
import os
import warnings
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


from tests.support.device import L  # noqa: E402,F401  (the module fixture)


def test_every_declared_symbol_is_exported(L):
    from lumahdrv_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lumahip.h")).read()
    declared = set(re.findall(r"\b(lumahip_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"lumahip_ctx"}
    lib = capi.lib()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert set(capi.SYMBOLS) == declared
    assert lib.lumahip_abi_version() == 5


def test_host_lut_builder_matches_reference_tables(L, golden_dir):
    from tests.golden.make_golden import CONFIGS
    g = np.load(os.path.join(golden_dir, "ref_luts.npz"))
    for name, cfg in CONFIGS.items():
        m = L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])
        assert np.array_equal(m.view(np.uint32), g[name].view(np.uint32)), name
    with pytest.raises(L.LumaHipError):
        L.build_lut(L.PTF_PSI, 13)      # the reference would read past its 12-bit table (quirk 3)


def test_no_gpu_means_loud_failure(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.LumaHipError):
        L.Context()
    with pytest.raises(L.LumaHipError):
        L.LumaQuantizer()


def test_facade_compiles_and_links(L, tmp_path):
    from tests.support.tools import build_facade_test
    exe = build_facade_test(str(tmp_path))
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lumahdrv_amd", "lib", "libluma_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    for sym in ("LumaEncoder", "LumaDecoder", "LumaQuantizer"):
        assert sym in out
    assert os.path.exists(exe)


def test_plane_geometry_matches_vpx_img_alloc():
    from lumahdrv_amd import plane_geometry
    # vpx_img_alloc(I42016, 3840, 2160, 32): stride 7680 / 3840, SURVEY.md 8(a) row a9
    assert plane_geometry(3840, 2160, 2)[2] == (7680, 3840, 3840)
    assert plane_geometry(1920, 1080, 2)[:2] == ((1920, 960, 960), (1080, 540, 540))
    assert plane_geometry(250, 100, 0)[2] == (256, 128, 128)
    assert plane_geometry(250, 100, 3)[2] == (512, 512, 512)


def _records_vs_oracle(capi, o, m, orc, rng):
    ix = capi.thresh_index(m)
    assert ix["ok"]
    mid = ((m[:-1].astype(np.float64) + m[1:]) / 2).astype(np.float32)
    zone = [mid]
    for _ in range(6):
        zone.append(np.nextafter(zone[-1], np.float32(np.inf)))
    dn = mid
    for _ in range(6):
        dn = np.nextafter(dn, np.float32(-np.inf))
        zone.append(dn)
    v = np.concatenate([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf))] + zone + [
        np.exp(rng.uniform(np.log(1e-8), np.log(1e9), 400000)).astype(np.float32),
        np.array([0.0, -0.0, -1.0, 1e-45, 1e-39, 3e38, np.inf, -np.inf, np.nan, -1e-30, 65504.0], dtype=np.float32)])
    v = np.where(np.isnan(v), np.float32(np.nan), v).astype(np.float32)     # numpy's nan is sign-clear
    v = np.concatenate([v, np.ones((-v.size) % 4, dtype=np.float32)])
    got = capi.thresh_lookup(ix, v)
    frame = np.stack([v.reshape(2, -1)] * 3).copy()
    planes, _, _ = orc.encode(frame, 1.0, 3)               # CS_RGB, profile 3: every value straight through the search
    exp = planes[0].view("<u2")[:, :frame.shape[2]].reshape(-1).astype(np.int64)
    assert np.array_equal(got, exp)
    return ix


def test_threshold_records_equal_the_reference_search(L, oracle_mod, golden_dir):
    """The threshold records the kernels search with (lut_index.hpp; one 4-byte gather per value) against the oracle's
    literal bisection + nearest-of-two (src/luma_quantizer.cpp:222-235) on the values where they could differ: every
    table entry and its neighbours, the rounding-tie zone around every midpoint, a dense log-uniform sample and the
    specials.  (The GPU suite repeats this for all 2^32 bit patterns through the kernels themselves.)"""
    from lumahdrv_amd import capi
    from tests.golden.make_golden import CONFIGS
    o = oracle_mod
    g = np.load(os.path.join(golden_dir, "ref_luts.npz"))
    rng = np.random.default_rng(1)
    for name, cfg in CONFIGS.items():
        m = g[name]
        orc = o.Oracle(cfg[0], cfg[1], o.CS_RGB, cfg[3], cfg[4], cfg[5], table=m if cfg[0] in (0, 3) else None)
        ix = _records_vs_oracle(capi, o, m, orc, rng)
        assert ix["nbuckets"] * 4 <= (72 << 10) or cfg[0] == L.PTF_LINEAR, name      # fits LDS (LINEAR: L2-resident)
    # duplicate entries are still a monotone step function
    dup = g["pq11_luv8"].copy()
    dup[5] = dup[4]
    orc = o.Oracle(o.PTF_PQ, 11, o.CS_RGB, 8, 1e4, 0.005)
    orc.overwrite_mapping(dup)
    _records_vs_oracle(capi, o, dup, orc, rng)
    dup[900:903] = dup[900]                       # a triple makes the code jump by two at one float: literal path
    assert not capi.thresh_index(dup)["ok"]
    # tables the records cannot represent: the kernels run the literal bisection
    bad = g["pq11_luv8"].copy()
    bad[100], bad[101] = bad[101], bad[100]
    assert not capi.thresh_index(bad)["ok"]
    nanlut = g["pq11_luv8"].copy()
    nanlut[7] = np.nan
    assert not capi.thresh_index(nanlut)["ok"]
    ix13 = capi.thresh_index(L.build_lut(L.PTF_PQ, 13))
    assert ix13["ok"] and ix13["nbuckets"] * 4 > (72 << 10)                         # global-memory records


def test_raw_stream_reader_rejects_crafted_headers(L, tmp_path):
    """LumaRawStreamReader::open (facade, upstream of LumaDecoder::decode) bounds the announced geometry by the file
    size and reports every malformed header as LumaException -- round-1 review: a 65536x65536 header made it allocate
    ~25 GB and die with std::bad_alloc.  CPU only (no context is created)."""
    lib = os.path.join(ROOT, "lumahdrv_amd", "lib")
    exe = str(tmp_path / "raw_stream_reject")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "raw_stream_reject.cpp"), "-o", exe, "-L" + lib, "-lluma_hip", "-llumahip",
                    "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_lumaenc_lumadec_option_handling(L):
    """tools/lumaenc.cpp / lumadec.cpp: the reference's option names, ranges, value sets and error situations
    (lumaenc.cpp:106-179, lumadec.cpp:71-90, its ArgParser): every rejected command line exits with status 1 and the
    reference's '<tool> input error:' prefix.  CPU only: nothing here reaches the GPU."""
    enc = os.path.join(ROOT, "lumahdrv_amd", "bin", "lumaenc")
    dec = os.path.join(ROOT, "lumahdrv_amd", "bin", "lumadec")
    assert os.path.exists(enc) and os.path.exists(dec)

    def run(exe, *a):
        r = subprocess.run([exe] + list(a), capture_output=True, text=True, timeout=60)
        return r.returncode, r.stderr

    rc, err = run(enc, "--help")
    assert rc == 1 and "--transfer-function <string>" in err and "-eb <int>," in err
    for flags, msg in (
            ((), "Missing required option '--output'"),
            (("-o", "x.lhs", "--bogus"), "The argument '--bogus' is not a valid input option"),
            (("-o",), "No value provided for input option '-o'"),
            (("-o", "x.mkv"), "Unsupported output format"),
            (("-o", "x.lhs", "-p", "4"), "Argument '-p' with value '4' is out of range. Valid range is [0, 3]"),
            (("-o", "x.lhs", "--quantizer-scaling", "64"), "Valid range is [0, 63]"),
            (("-o", "x.lhs", "-pb", "17"), "Valid range is [0, 16]"),
            (("-o", "x.lhs", "-ma", "50"), "Argument '-ma' with value '50' is out of range. Valid range is [100, 100000]"),
            (("-o", "x.lhs", "-mi", "100"), "out of range"),
            (("-o", "x.lhs", "-b", "10000"), "Valid range is [0, 9999]"),
            (("-o", "x.lhs", "-eb", "9"), "Input '9' for argument '-eb' is not valid. Valid values are: 8 10 12"),
            (("-o", "x.lhs", "-ptf", "pq"), "Input 'pq' for argument '-ptf' is not valid. Valid values are: PSI PQ LOG HDRVDP LINEAR"),
            (("-o", "x.lhs", "-cs", "YUV"), "Valid values are: LUV RGB YCBCR XYZ"),
            (("-o", "x.lhs", "-i", "__test__", "-f", "5"), "Unable to parse frame range from '5'. Valid format is startframe:step:endframe"),
            (("-o", "x.lhs", "-i", "__test__", "-f", "1:2:3:4"), "Unable to parse frame range"),
            (("-o", "x.lhs", "-i", "__test__", "-f", "a:3"), "Unable to parse frame range"),
            (("-o", "x.lhs", "-i", "__test__", "-f", "9:1:3"), "Invalid frame range '9:1:3'. End frame should be >= start frame")):
        rc, err = run(enc, *flags)
        assert rc == 1 and "lumaenc input error: " in err and msg in err, (flags, err)
    rc, err = run(enc, "-o", "x.lhs")                       # no input: the reference needs pfstools for stdin streams
    assert rc == 1 and "lumaenc encoding error: Compiled without pfstools support" in err
    rc, err = run(dec)
    assert rc == 1 and "lumadec input error: Missing required option '--input'" in err
    rc, err = run(dec, "-i", "/nonexistent/stream.lhs")
    assert rc == 1 and "lumadec decoding error: " in err


def test_drop_in_links_against_the_real_downstream(tmp_path):
    """INTEGRATION.md's two ways in, LINKED against the reference's real downstream (build container only): `make -C oracle
    ref_full` builds the vendored libvpx (generic-gnu), libebml and libmatroska and links
    A. this repo's facade + tools/integration/vpx_mkv_{sink,source}.h + the reference's MkvInterface (sink_encode_hipA,
       source_decode_hipA);
    B. the reference's own lumaenc.cpp / lumadec.cpp with tools/integration/apply_patch_b.py applied to its encoder / decoder
       classes (lumaenc_hipB, lumadec_hipB);
    and the complete unmodified reference applications beside them (lumaenc_ref, lumadec_ref).  Here: every link succeeded, no
    vpx_* / Kax* / Ebml* symbol is left undefined, the C-ABI symbols resolve in liblumahip.so, and the reference pair runs on
    the CPU (encode -> decode of two test frames).  tests/test_gpu_dropin.py runs the GPU-backed ones against it."""
    ref = "/root/reference"
    if not os.path.isdir(os.path.join(ref, "src")):
        pytest.skip("needs /root/reference")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref_full"], check=True)
    full = os.path.join(ROOT, "oracle", "_ref", "full")
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lumahdrv_amd", "lib", "liblumahip.so")],
                              capture_output=True, text=True, check=True).stdout
    facade = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lumahdrv_amd", "lib", "libluma_hip.so")],
                            capture_output=True, text=True, check=True).stdout
    for tool in ("lumaenc_ref", "lumadec_ref", "lumaenc_hipB", "lumadec_hipB", "sink_encode_hipA", "source_decode_hipA",
                 os.path.join("..", "ref_planes_tool")):
        und = subprocess.run(["nm", "-u", os.path.join(full, tool)], capture_output=True, text=True, check=True).stdout
        names = [l.split()[-1] for l in und.splitlines() if l.strip()]
        bad = [n for n in names if n.startswith("vpx_") or "Kax" in n or "Ebml" in n or "MkvInterface" in n]
        assert not bad, (tool, bad[:5])
        hip = [n for n in names if n.startswith("lumahip_")]
        if "_hipB" in tool:
            assert hip, tool                          # the hot path really is the C ABI's
            for n in hip:
                assert (" T " + n + "\n") in exported, (tool, n)
        elif "_hipA" in tool:                         # the facade's classes, which libluma_hip.so implements over the C ABI
            cls = [n for n in names if n.startswith(("_ZN11LumaEncoder", "_ZN11LumaDecoder"))]
            assert cls, tool
            for n in cls:
                assert (" T " + n + "\n") in facade, (tool, n)
        else:
            assert not hip, (tool, hip)               # the reference binaries do not touch it
    # the patched classes keep every other line of the reference: the edits are the C-ABI calls
    for f in ("luma_encoder.h", "luma_decoder.h", "luma_encoder.cpp", "luma_decoder.cpp"):
        assert "lumahip_" in open(os.path.join(full, "patch_b", f)).read()
    # the complete reference, run: two test frames through VP9 + Matroska and back
    subprocess.run([os.path.join(full, "lumaenc_ref"), "-i", "__test__", "-f", "1:1:2", "-o", "r.mkv"], cwd=tmp_path, check=True,
                   capture_output=True)
    subprocess.run([os.path.join(full, "lumadec_ref"), "-i", "r.mkv", "-o", "r_%05d.exr"], cwd=tmp_path, check=True, capture_output=True)
    assert os.path.getsize(tmp_path / "r_00002.exr") > 10000
    # without a GPU the patched application fails loudly, through the reference's own error path
    r = subprocess.run([os.path.join(full, "lumaenc_hipB"), "-i", "__test__", "-f", "1:1:1", "-o", "h.mkv"], cwd=tmp_path,
                       capture_output=True, text=True)
    import torch
    if not torch.cuda.is_available():
        assert r.returncode == 1 and "No usable HIP device" in r.stderr


def test_decoder_base_class_usage_compiles_against_both_trees():
    """tests/cpp/decoder_base_usage.cpp holds a LumaDecoderBase* and uses only what the reference documents on the base class
    (constructor (inputFile, verbose), seekToTime, getQuantizer, getReader, getFrame, initialized; LumaDecoderParams::stride as
    int *): it must compile unchanged against include/luma/ of this repo and -- in the build container -- against the
    reference's headers (include/luma/luma_decoder.h:81-120 there)."""
    src = os.path.join(ROOT, "tests", "cpp", "decoder_base_usage.cpp")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "luma"), src], check=True)
    ref = "/root/reference"
    vpx = os.path.join(ROOT, "oracle", "_ref", "full", "libvpx")
    if not os.path.isdir(os.path.join(ref, "src")):
        return
    if not os.path.isdir(os.path.join(vpx, "vpx")):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref_planes"], check=True)
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-w", "-I" + os.path.join(ref, "include", "luma"), "-I" + os.path.join(ref, "lib", "ebml"),
                    "-I" + os.path.join(ref, "lib", "matroska"), "-I" + os.path.join(vpx, "vpx"), "-I" + vpx, src], check=True)


def argparser_lines():
    """the command lines of the option-handling check: fixed ones, then random numeric options with values around their limits"""
    rng = np.random.default_rng(12)
    lines = [
        ["-o", "a.lhs"], ["--output", "a.lhs", "-i", "__test__", "-f", "1:2:9"], ["-o", "a.lhs", "-p", "0", "-q", "63", "-sc", "2.5e3"],
        ["-o", "a.lhs", "-pb", "16", "-cb", "0", "-ptf", "HDRVDP", "-cs", "XYZ", "-ma", "100", "-mi", "99.99"],
        ["-o", "a.lhs", "-b", "9999", "-k", "9999", "-eb", "8", "-l", "-v", "-fps", "59.94"],
        ["-o", "a.lhs", "-p", "3", "-p", "1"], ["-o", "a.lhs", "-p", "-1"], ["-o", "a.lhs", "-p", "abc"], ["-o", "a.lhs", "-p", "2.9"],
        ["-o", "a.lhs", "-sc", "-1"], ["-o", "a.lhs", "-sc", "1e21"], ["-o", "a.lhs", "-ma", "99.9"], ["-o", "a.lhs", "-mi", "0"],
        ["-o", "a.lhs", "-eb", "11"], ["-o", "a.lhs", "-ptf", "PQ "], ["-o", "a.lhs", "-cs", "luv"], ["-o", "a.lhs", "-q"],
        ["-o", "a.lhs", "--lossless", "--verbose", "--bogus"], ["-i", "x"], [], ["-o", "a.lhs", "-h"], ["--help"], ["-o", "a.lhs", "-l", "1"],
    ]
    names = [("-p", "--profile"), ("-q", "--quantizer-scaling"), ("-pb", "--ptf-bitdepth"), ("-cb", "--color-bitdepth"), ("-b", "--bitrate"),
             ("-k", "--keyframe-interval"), ("-eb", "--encoding-bitdepth"), ("-sc", "--pre-scaling"), ("-ma", "--max-luminance"),
             ("-mi", "--min-luminance"), ("-fps", "--framerate")]
    for _ in range(150):
        args = ["-o", "r.lhs"]
        for _ in range(int(rng.integers(1, 5))):
            short, long_ = names[int(rng.integers(0, len(names)))]
            v = rng.choice(["0", "1", "3", "4", "8", "9", "10", "12", "16", "17", "63", "64", "99", "100", "9999", "10000", "1e-10", "1e-11",
                            "99.99", "100.5", "1e5", "100001", "0.5", "-3", "x"])
            args += [short if rng.random() < 0.5 else long_, str(v)]
        lines.append(args)
    return lines


def test_lumaenc_option_handling_equals_the_reference_parser(tmp_path):
    """tools/lumaenc's option handling (tools/luma_cli.h) against the reference's own ArgParser (src/arg_parser.cpp compiled
    unmodified behind lumaenc's option table: oracle/_ref/ref_argparser_tool) on the same command lines: same accept / reject
    decision, same message, same parsed values -- atoi / atof conversions, range and value-set checks, repeated options,
    missing values, help.  The parser's answers are recorded in tests/golden/ref_argparser.json (tests/golden/make_golden.py);
    where oracle/_ref/ is built the parser also runs live and must give the recorded answers."""
    import json
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_argparser.json")))
    assert [a for a, _ in rec] == argparser_lines()
    tool = os.path.join(ROOT, "oracle", "_ref", "ref_argparser_tool")
    live = os.path.exists(tool)
    enc = os.path.join(ROOT, "lumahdrv_amd", "bin", "lumaenc")
    for args, ref in rec:
        if live:
            assert subprocess.run([tool] + args, capture_output=True, text=True, timeout=30).stdout.strip() == ref, args
        r = subprocess.run([enc] + args, capture_output=True, text=True, timeout=30, env=dict(os.environ, LUMAENC_PRINT_ARGS="1"))
        if ref.startswith("OK "):
            assert r.returncode == 0 and r.stdout.strip() == ref, (args, ref, r.stdout, r.stderr)
        elif ref == "HELP":
            assert r.returncode == 1 and "Available options:" in r.stderr, (args, r.stderr)
        else:
            assert ref.startswith("ERR ")
            assert r.returncode == 1 and ("lumaenc input error: " + ref[4:]) in r.stderr, (args, ref, r.stderr)


def test_bench_reports_counter_figures_only_for_matching_kernel_sources(tmp_path):
    """bench.py's roofline.traffic / VALU mix come from committed rocprofv3 captures; they must be dropped (null) when the
    capture was made from other kernel sources or for another launch size -- never reported stale."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    from lumahdrv_amd import capi
    sha = capi.kernel_source_sha()
    p = tmp_path / "t.json"
    json.dump({"pq11_luv": {"workload": "pq11_luv", "kernel_source_sha": sha, "pixels_per_launch": 100.0, "hbm_bytes_per_launch": 1500.0}}, open(p, "w"))
    assert b.load_profile(str(p), "pq11_luv", 100.0, sha)["hbm_bytes_per_launch"] == 1500.0
    assert b.load_profile(str(p), "pq11_luv", 100.0, "0" * 12) is None          # other sources
    assert b.load_profile(str(p), "log12_luv", 100.0, sha) is None              # other workload
    assert b.load_profile(str(tmp_path / "missing.json"), "pq11_luv", 100.0, sha) is None
    # the committed captures belong to the committed sources
    for f in ("traffic_latest.json", "valu_mix_latest.json"):
        d = json.load(open(os.path.join(ROOT, "profiles", f)))
        assert set(d) == {"pq11_luv", "pq10_ycbcr", "log12_luv"}
        # a capture from other kernel sources is legal in the tree (between a kernel change and the next tools/profile_round.sh
        # run) -- what must hold is that bench.py then reports null instead of the stale figure
        for wl, v in d.items():
            got = b.load_profile(os.path.join(ROOT, "profiles", f), wl, v["pixels_per_launch"], sha)
            if v["kernel_source_sha"] == sha:
                assert got is not None
            else:
                assert got is None
                warnings.warn("profiles/%s[%s] was captured from other kernel sources: bench.py reports null until "
                              "tools/profile_round.sh + summarize_profile.py are re-run" % (f, wl))


def test_threshold_records_on_random_monotone_tables(L, oracle_mod):
    """A decoder may be handed ANY attachment-434 table.  Random non-decreasing tables (log-uniform over 60 decades,
    linear, with zeros, denormals, duplicates, huge last entries; 2 ... 4096 entries): wherever the record builder
    accepts a table, its records must equal the oracle's literal search on the table's neighbourhoods and on a random
    sample; tables it refuses (codes jumping by two at one float) simply take the literal kernels."""
    from lumahdrv_amd import capi
    o = oracle_mod
    rng = np.random.default_rng(2024)
    accepted = refused = 0
    for trial in range(60):
        bits = int(rng.choice([1, 2, 3, 6, 10, 12]))
        n = 1 << bits
        kind = trial % 4
        if kind == 0:
            m = np.sort(np.exp(rng.uniform(np.log(1e-30), np.log(1e30), n))).astype(np.float32)
        elif kind == 1:
            m = np.sort(rng.uniform(0, 1e4, n)).astype(np.float32)
        elif kind == 2:
            m = np.sort(np.exp(rng.uniform(np.log(1e-44), np.log(1e-30), n))).astype(np.float32)      # denormals and tiny values
            m[0] = 0.0
        else:
            m = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(1e5), n))).astype(np.float32)
            k = int(rng.integers(0, n - 1))
            m[k + 1] = m[k]                                                                            # one duplicate
        ix = capi.thresh_index(m)
        if not ix["ok"]:
            refused += 1
            continue
        accepted += 1
        orc = o.Oracle(o.PTF_PQ, bits, o.CS_RGB, 8, 1e4, 0.005)
        orc.overwrite_mapping(m)
        mids = ((m[:-1].astype(np.float64) + m[1:]) / 2).astype(np.float32)
        v = np.concatenate([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf)), mids,
                            np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
                            np.exp(rng.uniform(np.log(1e-45), np.log(3e38), 20000)).astype(np.float32),
                            np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38], dtype=np.float32)])
        v = np.concatenate([v, np.ones((-v.size) % 2, dtype=np.float32)])
        got = capi.thresh_lookup(ix, v)
        frame = np.stack([v.reshape(2, -1)] * 3).copy()
        planes, _, _ = orc.encode(frame, 1.0, 3 if bits > 8 else 1)
        w = frame.shape[2]
        exp = (planes[0].view("<u2")[:, :w] if bits > 8 else planes[0][:, :w]).reshape(-1).astype(np.int64)
        assert np.array_equal(got & (0xFFFF if bits > 8 else 0xFF), exp), (trial, bits, kind)
    assert accepted >= 40 and accepted + refused == 60


def test_value_keyed_records_of_evenly_spaced_tables(L, oracle_mod):
    """PTF_LINEAR tables (src/luma_quantizer.cpp:200-203) and other evenly spaced ones: their float-bit records miss LDS from 12
    bits (229 KiB), the VALUE-keyed records (lut_index.hpp LinIndex; search mode 7) hold about one bucket per code.  Wherever
    the builder accepts a table its records must equal the oracle's literal search around every table entry and midpoint, on a
    random sample of values and of bit patterns, and on the special values; PQ / LOG tables (thresholds crowd near zero) and
    tables with duplicates must be refused."""
    from lumahdrv_amd import capi
    o = oracle_mod
    rng = np.random.default_rng(7)
    cases = [(capi.build_lut(capi.PTF_LINEAR, b, mx, 0.005), b) for b, mx in ((12, 1e4), (8, 1e4), (10, 1000.0), (13, 1e4), (14, 1e4), (11, 0.37), (4, 3e38))]
    jit = (np.arange(4096) * 2.5 + rng.uniform(-0.3, 0.3, 4096)).astype(np.float32)          # evenly spaced with jitter
    jit[0] = 0.0
    cases.append((np.sort(jit), 12))
    for m, bits in cases:
        ix = capi.lin_index(m)
        # PTF_LINEAR: one bucket per code (+ 0.2 % + the two ends); the jittered table: its smallest gap sets the bucket width
        assert ix["ok"] and ix["nbuckets"] <= (1.5 if m is cases[-1][0] else 1.02) * m.size + 8, (bits, ix["nbuckets"])
        orc = o.Oracle(o.PTF_PQ, bits, o.CS_RGB, 8, 1e4, 0.005)
        orc.overwrite_mapping(m)
        mids = ((m[:-1].astype(np.float64) + m[1:]) / 2).astype(np.float32)
        v = np.concatenate([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf)), mids,
                            np.nextafter(mids, np.float32(np.inf)), np.nextafter(mids, np.float32(-np.inf)),
                            rng.uniform(-0.01 * float(m[-1]), min(1.2 * float(m[-1]), 3.4e38), 20000).astype(np.float32),
                            rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                            np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32),
                            np.array([0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff], dtype=np.uint32).view(np.float32)])
        v = np.concatenate([v, np.ones((-v.size) % 2, dtype=np.float32)])
        got = capi.lin_lookup(ix, v)
        frame = np.stack([v.reshape(2, -1)] * 3).copy()
        with np.errstate(all="ignore"):
            planes, _, _ = orc.encode(frame, 1.0, 3 if bits > 8 else 1)
        w = frame.shape[2]
        exp = (planes[0].view("<u2")[:, :w] if bits > 8 else planes[0][:, :w]).reshape(-1).astype(np.int64)
        assert np.array_equal(got & (0xFFFF if bits > 8 else 0xFF), exp), bits
    for ptf, bits in ((capi.PTF_PQ, 11), (capi.PTF_LOG, 12), (capi.PTF_PQ, 8)):
        assert not capi.lin_index(capi.build_lut(ptf, bits, 1e4, 0.005))["ok"]
    dup = capi.build_lut(capi.PTF_LINEAR, 10, 1e4, 0.005)
    dup[500] = dup[499] = dup[498]
    assert not capi.lin_index(dup)["ok"]


def test_ycbcr_stream_tables_equal_the_reference_arithmetic(L, oracle_mod):
    """The two per-stream tables of the YCbCr kernels, built on the host with libm (host_lut.cpp): (1) the composite
    "t = 219 y + 16 -> luminance code" threshold records against the oracle's PQdec(t / 255) + literal search
    (src/luma_quantizer.cpp:337, 496-500, 222-235) around every threshold and on a dense sample; (2) the y table against
    (255 PQenc(lut[i]) - 16) / 219 (src/luma_quantizer.cpp:447-448).  (The GPU suite sweeps every float >= 16 through the kernels' own
    lookup.)"""
    import ctypes as C
    from lumahdrv_amd import capi
    o = oracle_mod
    lo = o.lib()
    lo.lo_transform_pq.restype = C.c_float
    lo.lo_transform_pq.argtypes = [C.c_float, C.c_float, C.c_int]
    rng = np.random.default_rng(5)
    for ptf, bits, mx in ((L.PTF_PQ, 10, 1000.0), (L.PTF_PQ, 11, 1e4), (L.PTF_LOG, 12, 1e4), (L.PTF_PQ, 8, 1e4)):
        lut = L.build_lut(ptf, bits, mx, 0.005)
        ix = capi.ycbcr_luma_index(lut, mx)
        assert ix["ok"] and ix["nbuckets"] * 4 <= (64 << 10)
        orc = o.Oracle(ptf, bits, o.CS_YCBCR, 10, mx, 0.005)

        def want(t):
            return np.array([int(orc.quantize(lo.lo_transform_pq(mx, float(x) / np.float32(255.0), 0), 0)) for x in (t / np.float32(255.0))])

        # every bucket edge and both neighbours, a dense sample of [16, 600], the specials
        k = np.arange(ix["kmin"], ix["kmin"] + ix["nbuckets"], dtype=np.int64)
        edges = np.concatenate([(k << ix["shift"]), (k << ix["shift"]) - 1, ((k + 1) << ix["shift"]) - 1])
        edges = edges[(edges >= 0x41800000) & (edges <= 0x7f800000)].astype(np.uint32).view(np.float32)
        t = np.concatenate([edges[::7], rng.uniform(16, 600, 30000).astype(np.float32),
                            np.array([16.0, 255.0, 507.9, 508.5, 1e30, np.inf], dtype=np.float32)])
        v = t / np.float32(255.0)
        exp = np.array([int(orc.quantize(lo.lo_transform_pq(mx, float(x), 0), 0)) for x in v])
        assert np.array_equal(capi.thresh_lookup(ix, t), exp), (ptf, bits)
        yt = capi.ycbcr_ytab(lut, mx)
        e = np.array([(np.float32(255) * np.float32(lo.lo_transform_pq(mx, float(x), 1)) - np.float32(16)) / np.float32(219) for x in lut],
                     dtype=np.float32)
        assert np.array_equal(yt.view(np.uint32), e.view(np.uint32)), (ptf, bits)
    # a table the composite cannot be built for (LINEAR-12: too many records) simply has none
    assert not capi.ycbcr_luma_index(L.build_lut(L.PTF_LINEAR, 12, 1e4, 0.005), 1e4)["ok"]


def test_half_input_table_equals_the_reference_arithmetic(L, oracle_mod):
    """The half-input table of the YCbCr encode kernels (host_lut.cpp ycbcr_half_table_host): entry i against the oracle's
    PQenc(std::max(x * sc, 1e-10f)) (src/luma_quantizer.cpp:331-333, 491-494) for EVERY half x in +0 ... +inf, for the
    preScalings / peaks the GPU suite encodes with; and the pairs it must refuse."""
    from lumahdrv_amd import capi
    lo = oracle_mod.lib()
    halves = np.arange(capi.HALF_TABLE_LEN, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert halves[0] == 0.0 and np.isinf(halves[-1]) and np.all(np.isfinite(halves[:-1]))
    for sc in (1.0, 20.0, 0.25, 3.0e30):
        for mx in (1000.0, 1e4):
            t = capi.ycbcr_half_table(sc, mx)
            assert t is not None and t.size == capi.HALF_TABLE_LEN
            with np.errstate(over="ignore"):
                arg = np.maximum(halves * np.float32(sc), np.float32(1e-10))
            exp = np.array([lo.lo_transform_pq(mx, float(v), 1) for v in arg], dtype=np.float32)
            same = (t.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(t) & np.isnan(exp))
            assert bool(np.all(same)), (sc, mx, int(np.argmin(same)))
            ok = np.isnan(t) | ((t >= np.float32(7e-7)) & (t <= np.float32(2.0)))
            assert bool(np.all(ok)) and np.isnan(t[-1])          # PQenc(inf) = NaN, everything else in the licensed range
    for sc, mx in ((0.0, 1e4), (-1.0, 1e4), (float("inf"), 1e4), (float("nan"), 1e4), (1.0, 0.0), (1.0, -5.0), (1.0, float("nan")),
                   (1.0, 1e-30)):
        assert capi.ycbcr_half_table(sc, mx) is None, (sc, mx)


def test_scalar_quantize_dequantize_equal_the_reference_fixture(L, golden_dir):
    """LumaQuantizer::quantize / dequantize for one value on the host (lumahip_quantize_value_host, what the C++ facade's
    per-value members call): every value of tests/golden/ref_quantize.npz -- produced by the reference's own compiled
    LumaQuantizer (src/luma_quantizer.cpp:215-264), NaN / +-inf / -0 / denormals and out-of-range codes included -- for all
    eight configurations, both channels.  No GPU."""
    from lumahdrv_amd import capi
    from tests.golden.make_golden import CONFIGS
    g = np.load(os.path.join(golden_dir, "ref_quantize.npz"))
    luts = np.load(os.path.join(golden_dir, "ref_luts.npz"))
    for name, cfg in CONFIGS.items():
        ptf, bits, cs, bitsC, mx, mn = cfg
        lut = luts[name] if name in luts else L.build_lut(ptf, bits, mx, mn)
        assert lut.size == 1 << bits
        for ch in (0, 1):
            vin = g["%s_in%d" % (name, ch)]
            got = np.array([capi.quantize_value(lut, cs, bitsC, float(v), ch) for v in vin], dtype=np.float32)
            assert np.array_equal(got.astype(np.uint16), g["%s_q%d" % (name, ch)]) and np.all(got == np.floor(got)), (name, ch)
        codes = np.arange(-2, 2 ** bits + 2, dtype=np.float32)
        dq0 = np.array([capi.quantize_value(lut, cs, bitsC, float(v), 0, dequantize=True) for v in codes], dtype=np.float32)
        assert np.array_equal(dq0.view(np.uint32), g[name + "_dq0"].view(np.uint32)), name
        dq1 = np.array([capi.quantize_value(lut, cs, bitsC, float(v), 1, dequantize=True) for v in range(2 ** bitsC)], dtype=np.float32)
        assert np.array_equal(dq1.view(np.uint32), g[name + "_dq1"].view(np.uint32)), name
    # bad arguments are refused, not read
    import ctypes as C
    out = C.c_float(0)
    assert capi.lib().lumahip_quantize_value_host(None, 8, 0, 8, 1.0, 0, C.byref(out)) == capi.ERR_ARG
    assert capi.lib().lumahip_dequantize_value_host(lut.ctypes.data, 1, 0, 8, 1.0, 0, C.byref(out)) == capi.ERR_ARG


def test_numa_plan_from_a_fabricated_sysfs_tree(tmp_path):
    """lumahip_numa_plan_host: which NUMA node and which CPUs the host side of a context is placed on, derived from a sysfs
    tree shaped like the GPU boxes' (two sockets, 64 cores x 2 threads each, GPUs on both) -- no GPU, no /sys of this machine."""
    from lumahdrv_amd import capi
    root = tmp_path / "sys"
    for node, cl in ((0, "0-63,128-191\n"), (1, "64-127,192-255\n")):
        d = root / "devices" / "system" / "node" / ("node%d" % node)
        d.mkdir(parents=True)
        (d / "cpulist").write_text(cl)
    for bus, node in (("0000:05:00.0", "0\n"), ("0000:85:00.0", "1\n"), ("0000:c5:00.0", "-1\n"), ("0001:0a:00.0", "7\n")):
        d = root / "bus" / "pci" / "devices" / bus
        d.mkdir(parents=True)
        (d / "numa_node").write_text(node)
    r = str(root)
    n0 = list(range(0, 64)) + list(range(128, 192))
    n1 = list(range(64, 128)) + list(range(192, 256))
    assert capi.numa_plan(r, "0000:05:00.0") == (0, n0)
    assert capi.numa_plan(r, "0000:85:00.0") == (1, n1)
    assert capi.numa_plan(r, "0000:85:00.0".upper()) == (1, n1) and capi.numa_plan(r, "85:00.0") == (1, n1)   # as hipDeviceGetPCIBusId may print it
    assert capi.numa_plan(r, "0000:85:00.0", "0-7,64-71,200") == (1, list(range(64, 72)) + [200])              # a cpuset: only what the process may use
    assert capi.numa_plan(r, "0000:85:00.0", "0-7") == (1, [])                                               # the cpuset excludes the node: no pinning
    assert capi.numa_plan(r, "0000:c5:00.0") == (-1, [])                                                     # the kernel does not know: nothing
    assert capi.numa_plan(r, "0000:ff:00.0") == (-1, [])                                                     # no such device
    assert capi.numa_plan(r, "0001:0a:00.0") == (7, [])                                                      # a node without a cpulist
    with pytest.raises(capi.LumaHipError):
        capi.numa_plan(r, "0000:85:00.0", "3-1")
    with pytest.raises(capi.LumaHipError):
        capi.numa_plan(r, "0000:85:00.0", "a,b")
