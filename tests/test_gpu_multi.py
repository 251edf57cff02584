"""The N>1 path on real devices.  `ShardedStream` (lumahdrv_amd/sharding.py) driving a real lumahdrv_amd.Context per
rank over the "nccl" (= RCCL) backend: 2 ranks when the box has >= 2 GPUs, 1 rank otherwise (the 1-GPU boxes still
exercise RCCL init, the quantizer broadcast on device tensors and the digest gather).  And bench.py's own contract:
one JSON line, the world size RCCL reports, the config-5 stream mode, and the refusal to mislabel a run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.support.tools import ROOT, bench


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, nframes, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import lumahdrv_amd as L
    from lumahdrv_amd.sharding import ShardedStream
    from oracle import oracle_py as o          # only the synthetic frame generator and the digest function (test plumbing)
    cfg = lut = None
    if rank == 0:   # only rank 0 knows the configuration and builds the table
        cfg = (L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005, 1.0, 2)
        lut = L.build_lut(L.PTF_PQ, 11, 1e4, 0.005)
    st = ShardedStream(nframes, dev, cfg, lut)

    def make_worker(cfg, lut):
        ctx = L.Context(rank)                  # the product: HIP kernels on this rank's GPU
        ctx.set_quantizer(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], lut)   # the BROADCAST table
        return ctx

    def process(ctx, f):
        planes, _, _ = ctx.encode_frame(o.synth_frame(64, 32, frame=f), st.cfg[6], st.cfg[7])
        return o.fnv1a64(np.concatenate([p.ravel() for p in planes]))

    digests = st.run(make_worker, process)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(digests, dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_stream_drives_real_contexts_over_rccl(tmp_path, oracle_mod):
    import torch
    import torch.multiprocessing as mp
    o = oracle_mod
    world = 2 if torch.cuda.device_count() >= 2 else 1
    nframes = 7
    mp.spawn(_worker, args=(world, _free_port(), nframes, str(tmp_path)), nprocs=world, join=True)
    orc = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    expect = []
    for f in range(nframes):
        planes, _, _ = orc.encode(o.synth_frame(64, 32, frame=f), 1.0, 2)
        expect.append(o.fnv1a64(np.concatenate([p.ravel() for p in planes])) & 0x7FFFFFFFFFFFFFFF)
    for r in range(world):
        assert np.load(tmp_path / ("rank%d.npy" % r)).tolist() == expect     # every rank holds the in-order digests


@pytest.mark.gpu
def test_bench_contract_single_gpu():
    p = bench("--full", "--steps", "3", "--warmup", "1", "--min-seconds", "0.05", "--no-cpu-baseline", "--no-other-workloads",
              "--no-facade-hostfed")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Mpixels/s" and r["value"] > 0 and r["full"] is True
    assert r["repeats"] >= 1 and r["ms_per_step_min"] <= r["ms_per_step"] <= r["ms_per_step_max"]
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1 and abs(rf["achieved"] / rf["peak"] - rf["frac"]) < 1e-3
    assert rf["traffic"] is None or abs(rf["traffic"] / rf["algorithmic_bytes_per_launch"] - 1) < 0.05
    # round 3: decode has its own roofline block (own traffic-only probe), the ordered figures sit beside the overlapped ones,
    # the plain-allocation rate beside the placed one, and the drop-in call on host frames is part of the line
    dr = r["decode_roofline"]
    assert dr["bound"] == "hbm" and 0 < dr["frac"] < 1 and dr["traffic_only_ms"] > 0 and dr["kernel_ms"] > 0
    assert dr["traffic"] is None or abs(dr["traffic"] / dr["algorithmic_bytes_per_launch"] - 1) < 0.05
    assert rf["kernel_ms_ordered"] > 0 and r["value_ordered"] > 0 and r["lanes"] == 2
    assert r["ms_per_step_over_ranks"]["min"] <= r["ms_per_step_over_ranks"]["max"]
    # round 4: roofline.frac is the ORDERED figure (one launch's own duration, what a rocprofv3 kernel trace of --lanes 0 gives);
    # the window of the overlapped launches is reported beside it
    bytes_ = rf["algorithmic_bytes_per_launch"]
    assert abs(bytes_ / (rf["kernel_ms_ordered"] * 1e-3) / 1e9 / rf["peak"] - rf["frac"]) < 2e-3 and rf["frac_overlapped"] > 0
    assert abs(bytes_ / (dr["kernel_ms_ordered"] * 1e-3) / 1e9 / dr["peak"] - dr["frac"]) < 2e-3
    # round 6: the configuration is the arguments' (configs[1]: 500 frames resident, never fewer silently); the HBM-read wording of
    # north_star beside the 15 B/pixel figures; the small pool and the plain allocations with their own ordered fractions
    c = r["config"]
    assert c["resident_frames"] == 500 and c["stream_frames"] == 500 and c["resident_frames_per_rank"] == [500] and r["config_degraded"] is False
    ro, dro = rf["read_only"], dr["read_only"]
    assert ro["bytes_per_launch"] == 12.0 * 20 * 3840 * 2160 and dro["bytes_per_launch"] == 3.0 * 20 * 3840 * 2160
    assert abs(ro["frac"] / rf["frac"] - 0.8) < 1e-3 and abs(dro["frac"] / dr["frac"] - 0.2) < 1e-3
    if "small_pool" in r:      # (absent only when a dozen chunks cannot be had)
        sp = r["small_pool"]
        assert sp["resident_frames"] == 40 and sp["value"] == r["value_small_pool"] > 0 and 0 < sp["frac_ordered"] < 1 and sp["pool_GB_kept"] < 10
    if r["placement"].get("grouped"):
        assert r["value_placement_off"] > 0 and r["placement_off"]["resident_frames"] == 160 and 0 < r["placement_off"]["frac_ordered"] < 1
        # the reference's decoder returns the packed LumaFrame: that layout's decode rate, pool-placed and plainly allocated
        pk = r["decode_packed_layout"]
        # (a box with little free HBM gives the pool too few chunks for some of these legs: they are then absent, never wrong)
        assert "caller_buffer" in pk and "library_ring" in pk      # one caller-owned buffer / buffers the library allocates and places
        assert r["decode_packed_mpix_s"] == pk["library_ring"]["value"] and r["decode_packed_frac"] == pk["library_ring"]["frac_ordered"]
        for how in ("pool_placed", "pool_rotating", "frame_rotating", "library_ring", "caller_buffer"):
            if how in pk:
                assert pk[how]["value"] > 0 and 0 < pk[how]["frac_ordered"] < 1 and pk[how]["kernel_ms_ordered"] > 0, pk
    assert "facade_hostfed" not in r                      # (--no-facade-hostfed: that leg has its own test below)


@pytest.mark.gpu
def test_bench_plain_run_times_exactly_k_steps_and_dumps_what_they_computed(tmp_path, oracle_mod):
    """The plain line is the headline alone: ONE region of exactly --steps steps (ms_per_step = its time / K), none of the --full
    legs.  --dump-outputs writes the planes the last timed step encoded (step W + K - 1: batch 3 of the 25-batch stream here,
    frames 60..79) as seeded float32 samples: they must be the oracle's codes of those frames at the same positions."""
    from lumahdrv_amd.benchlib import outputs as bo
    o = oracle_mod
    d = tmp_path / "out"
    _wait_for_hbm()
    p = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    if p.returncode == 3:
        pytest.skip("the 500-frame resident stream does not fit this GPU's free HBM right now (bench.py exit code 3, by design): "
                    + p.stderr[-300:])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["repeats"] == 1 and r["full"] is False and r["higher_is_better"] is True
    assert r["unit"] == "Mpixels/s" and r["dtype"] == "f32" and r["ms_per_step"] > 0
    w, h, B = 3840, 2160, 20
    assert abs(B * w * h / (r["ms_per_step"] * 1e-3) / 1e6 / r["value"] - 1) < 2e-3
    for k in ("roofline", "decode_mpix_s", "value_ordered", "other_workloads", "facade_hostfed", "cpu_baseline", "placement_off"):
        assert k not in r, k
    files = sorted(os.listdir(d))
    assert files == ["u_plane_sample.npy", "v_plane_sample.npy", "y_plane_sample.npy"]
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    got = {f[0]: np.load(d / f) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    _, hs, st, _ = o.plane_geometry(w, h, 2)
    ws = (w, w // 2, w // 2)
    pos = [bo.sample_positions(B * hs[p] * ws[p], bo.SAMPLE_CAP[p], p) for p in range(3)]
    assert [got[c].size for c in "yuv"] == [len(x) for x in pos]
    orc = o.Oracle(o.PTF_PQ, 11, o.CS_LUV, 8, 1e4, 0.005)
    first = ((1 + 3 - 1) % 25) * B
    for f in range(B):
        planes, _, _ = orc.encode(o.synth_frame(w, h, bo.SEED, first + f), 1.0, 2, threads=16)
        for p, c in enumerate("yuv"):
            codes = np.ascontiguousarray(planes[p]).view("<u2")[:, :ws[p]].reshape(-1)
            sel = (pos[p] // (hs[p] * ws[p])) == f
            assert np.array_equal(got[c][sel], codes[pos[p][sel] % (hs[p] * ws[p])].astype(np.float32)), (f, c)


@pytest.mark.gpu
def test_hostfed_leg_schema_and_half_upload_counters():
    """The host-fed leg of the bench line (tools/facade_hostfed.cpp: the drop-in calls on HOST frames).  Schema and deterministic
    evidence only -- the rates are PCIe- and host-CPU-bound on shared hosts, so nothing here compares one rate with another:
    that binary16-valued frames crossed PCIe as halves is read from lumahip_half_upload_info's counters."""
    exe = os.path.join(ROOT, "lumahdrv_amd", "bin", "facade_hostfed")
    p = subprocess.run([exe, "1280", "720", "6"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    hf = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("LumaEncoder_encode_pageable_frame", "LumaEncoder_pipelined_encode_pageable_frame", "LumaEncoder_encode_registered_frame",
              "LumaEncoder_encode_pageable_half_valued_frame", "LumaEncoder_pipelined_encode_pageable_half_valued_frame",
              "lumahip_encode_frames_host_pinned", "lumahip_encode_frames_host_pageable", "lumahip_encode_frames_host_pageable_half_valued",
              "decode_frame_host_pageable", "decode_stream_pageable", "lumahip_decode_frames_host_pageable",
              "LumaQuantizer_quantize_ns_per_call", "LumaQuantizer_dequantize_ns_per_call"):
        assert hf[k] > 0, k
    up = hf["half_upload_info"]                  # {uploaded as halves, found to hold other values, left as floats by policy}
    if "no F16C" not in p.stderr:
        assert up[0] >= 6 and up[1] == 0, up      # the batched call's frames all went up as halves, none was found to hold floats


@pytest.mark.gpu
def test_bench_rccl_path_and_stream_mode():
    """the RCCL code path with the devices this box has (forced with one rank), in the 2000-frame-stream mode scaled down"""
    import torch
    n = 2 if torch.cuda.device_count() >= 2 else 1
    p = bench("--gpus", str(n), "--stream-frames", "37", "--frames-per-step", "8", "--width", "1280", "--height", "720",
              "--min-seconds", "0.05", env={"LUMAHIP_BENCH_FORCE_DIST": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
    assert r["n_gpus"] == n and r["scaling"] == "strong"
    assert r["digests"]["gathered_in_stream_order"] == 37 and r["digests"]["spot_checked_by_rank0"] == 2 * n
    # the stream digest does not depend on how many ranks produced it
    q = bench("--gpus", "1", "--stream-frames", "37", "--frames-per-step", "5", "--width", "1280", "--height", "720",
              "--min-seconds", "0.05")
    assert q.returncode == 0, q.stderr[-2000:]
    assert json.loads(q.stdout.splitlines()[-1])["digests"]["stream_digest"] == r["digests"]["stream_digest"]


def _wait_for_hbm(min_free_frac=0.9, settle_s=2.0, timeout_s=90.0):
    """A process that has just exited may not have handed its HBM back to the driver yet (profiles/r03_settle.txt): wait until the
    free figure is high and has stopped moving before the next bench process is started.  Returns the free bytes seen."""
    import time

    import torch
    t0, last, since = time.time(), -1, time.time()
    while True:
        free, total = torch.cuda.mem_get_info(0)
        if abs(free - last) > (256 << 20):
            last, since = free, time.time()
        if (free >= min_free_frac * total and time.time() - since >= settle_s) or time.time() - t0 > timeout_s:
            return free
        time.sleep(0.25)


@pytest.mark.gpu
def test_bench_under_the_launcher_at_n1_is_the_plain_run():
    """The driver's scaling curve starts with N = 1 in the LAUNCHER form (python -m torch.distributed.run --nnodes=1
    --nproc-per-node 1 ... bench.py --gpus 1): one rank with WORLD_SIZE=1 in its environment.  It must be the plain `python
    bench.py` run -- same configuration, same fields, no process group -- so that the N = 1 point of the curve and the round's
    BENCH line are one measurement.  `config` is a function of the arguments (benchlib/plan.py), so it is compared WHOLE, with
    each other and with what `--plan-only` prints without a GPU; where the buffers ended up (`placement`) and the rates depend on
    the box and the moment and are only printed (round 5 asserted them and failed on the driver's lease)."""
    import torch
    torch.cuda.empty_cache()
    flags = ["--gpus", "1", "--steps", "10", "--warmup", "2", "--min-seconds", "0.3", "--no-cpu-baseline", "--no-other-workloads",
             "--no-facade-hostfed", "--no-placement-off"]
    planned = bench(*(flags + ["--plan-only", "--hbm-free-gb", "280"]))
    assert planned.returncode == 0, planned.stderr[-2000:]
    plan = json.loads(planned.stdout.strip().splitlines()[-1])
    _wait_for_hbm()
    plain = bench(*flags)
    if plain.returncode == 3:
        pytest.skip("the 500-frame resident stream does not fit this GPU's free HBM right now (bench.py exit code 3, by design): "
                    + plain.stderr[-300:])
    assert plain.returncode == 0, plain.stderr[-2000:]
    _wait_for_hbm()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + flags
    e = dict(os.environ)
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    launched = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=900)
    assert launched.returncode == 0, launched.stderr[-2000:]
    a = json.loads([l for l in plain.stdout.splitlines() if l.startswith("{")][-1])
    b = json.loads([l for l in launched.stdout.splitlines() if l.startswith("{")][-1])
    assert len([l for l in launched.stdout.splitlines() if l.startswith("{")]) == 1        # ONE JSON line under the launcher too
    assert set(a) == set(b) and (a["n_gpus"], b["n_gpus"]) == (1, 1) and a["scaling"] == b["scaling"] == "weak"
    assert a["config"] == b["config"] and not a["config_degraded"] and not b["config_degraded"]
    want = dict(plan["config"], world_size_reported_by="single process")
    assert a["config"] == want, (a["config"], want)
    assert a["config"]["resident_frames"] == 500 and a["config"]["stream_frames"] == 500      # BASELINE configs[1]
    assert a["rccl_ranks_seen"] is None and b["rccl_ranks_seen"] is None                     # no process group at N = 1 either way
    for r in (a, b):
        rs = r["placement"]["resident_stream"]
        assert rs["batches"] == 25 and rs["batches_in_pool_chunks"] + rs["batches_in_plain_allocations"] == 25
    print("plain %.0f Mpixel/s (%d of 25 batches placed), under torch.distributed.run %.0f (%d placed), ratio %.3f"
          % (a["value"], a["placement"]["resident_stream"]["batches_in_pool_chunks"], b["value"],
             b["placement"]["resident_stream"]["batches_in_pool_chunks"], b["value"] / a["value"]))


@pytest.mark.gpu
def test_bench_fails_loudly_when_the_stream_does_not_fit(tmp_path):
    """Short memory never shrinks the workload (round 5: 480 instead of 500 frames, silently).  With most of the HBM held by
    this process, `bench.py` exits with code 3 and no JSON line; `--allow-short-stream` runs a shorter stream and says so."""
    import torch
    _wait_for_hbm()
    free, total = torch.cuda.mem_get_info(0)
    hold_bytes = max(0, free - (40 << 30))                    # leave ~40 GB: the 500-frame stream needs 112 GB
    hold = [torch.empty(min(8 << 30, hold_bytes - k), dtype=torch.uint8, device="cuda:0") for k in range(0, hold_bytes, 8 << 30)]
    try:
        flags = ["--steps", "3", "--warmup", "1", "--min-seconds", "0.05", "--no-cpu-baseline", "--no-other-workloads",
                 "--no-facade-hostfed", "--no-placement-off"]
        p = bench(*flags)
        assert p.returncode == 3 and "does not fit" in p.stderr and not [l for l in p.stdout.splitlines() if l.startswith("{")], p.stderr[-1500:]
        q = bench(*(flags + ["--allow-short-stream"]))
        assert q.returncode == 0, q.stderr[-2000:]
        r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
        assert r["config_degraded"] is True and 20 <= r["config"]["resident_frames"] < 500 and r["config"]["resident_frames"] % 20 == 0
        assert "%d-frame resident stream" % r["config"]["resident_frames"] in r["config"]["workload"]
    finally:
        del hold
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_bench_refuses_more_gpus_than_visible():
    import torch
    n = torch.cuda.device_count() + 1
    p = bench("--gpus", str(n), "--steps", "1")
    assert p.returncode != 0 and "visible" in (p.stderr + p.stdout)


def test_bench_never_mislabels_world_size():
    """CPU-checkable halves of the contract: --gpus 2 with WORLD_SIZE=1 in the environment must fail (round 1 silently ran
    one rank and printed n_gpus: 1), and --gpus 2 without devices must fail instead of reporting fewer GPUs."""
    p = bench("--gpus", "2", "--steps", "1", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)
    import torch
    if not torch.cuda.is_available():
        q = bench("--gpus", "2", "--steps", "1")
        assert q.returncode != 0 and "visible" in (q.stderr + q.stdout)


@pytest.mark.gpu
def test_bench_config3_encode_is_hbm_bound():
    """BASELINE configs[2] (HDR10 recipe, 4K): the synthetic stream holds binary16 values, as every EXR frame of the reference
    does, so the encode launches run on the half-input table and the line prices them against HBM; decode stays VALU-bound."""
    p = bench("--full", "--steps", "3", "--warmup", "1", "--min-seconds", "0.05", "--no-cpu-baseline", "--no-other-workloads",
              "--no-facade-hostfed", "--no-placement-off", "--workload", "pq10_ycbcr")
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1 and r["value"] > 0
    assert rf["half_input_table"]["table_launches"] > 0 and rf["half_input_table"]["backoff_launches"] == 0
    dr = r["decode_roofline"]
    assert dr["bound"] == "valu" and 0 < dr["hbm"]["frac"] < 1
    assert dr["frac"] is None or dr["frac"] > 0               # (VALU roofline from the committed instruction mix, when it matches the sources)
    # the other input class of this configuration: the same stream with full-precision mantissas (what the reference's PFS pipe
    # delivers, src/pfs_interface.cpp:57-113) through the DEFAULT policy -- VALU-bound, and the launches of each kind are exactly
    # what the policy's model says for a stream of that many float launches (a function of the data, not of timing)
    from tests.support.host import _half_policy_model
    fi = r["float_inputs"]
    assert fi["value"] > 0 and fi["roofline"]["bound"] == "valu" and 0 < fi["hbm_frac"] < 1
    n = fi["table_launches"] + fi["backoff_launches"]
    assert n >= 8 and _half_policy_model([True] * n)[-1] == (fi["table_launches"], fi["backoff_launches"]), fi
    # decode of a picture-like stream (the red / blue tables are read) next to the synthetic stream's (they are not: its launches
    # report no local wave and the policy -- the same model, pause capped at 64 -- sends the rest to the plain kernels)
    dc = r["decode_coherent"]
    assert dc["value"] > 0 and dc["backoff_launches"] == 0 and dc["table_launches"] >= 8 and dc["rb_table_bytes"] == 8 << 20, dc
    dp = r["decode_random_rb_policy"]
    n = dp["table_launches"] + dp["backoff_launches"]
    assert _half_policy_model([True] * n, longest=64)[-1] == (dp["table_launches"], dp["backoff_launches"]), dp
    mi = r["mixed_inputs_1e-3"]
    assert mi["value"] > 0 and mi["backoff_launches"] == 0 and mi["table_launches"] >= 8, mi   # 1e-3 of the pixels: stays on the table
