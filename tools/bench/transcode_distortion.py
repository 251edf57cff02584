#!/usr/bin/env python3
"""tools/bench/transcode_distortion.py [--rounds R] [--min-s S] [--out FILE] -- the fused transcode distortion launch against what
it replaces.

Workloads: PQ-11 Lu'v' planes -> LOG-12 Lu'v' and -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20); profile 2 on both
sides, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process on one box, four distinct
batches.  The given planes are the source planes' own transcode under a target preScaling 2 % off (small differences nearly
everywhere, as a lossy decode leaves them).  Legs, interleaved round by round:
  `fused`     = lumahip_transcode_distortion_frames_device;
  `replaced`  = lumahip_transcode_frames_device into scratch planes, then the torch reduction that yields the same twelve
                integers per frame (difference, square, sum, max, count per plane);
  `transcode` = that transcode launch alone (the kernel the fused one shares its front end with).
Per leg and round: hipEvent time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
The two legs' integers are compared once before anything is timed.
-> profiles/transcode_distortion.jsonl: every run APPENDS one JSON line with, per workload, ms and Mpixel/s of each leg, fused over
replaced, the fused and the transcode kernel's fraction of 8 TB/s at 6 B/pixel, and the spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402
from tools.bench.distortion import torch_reduction  # noqa: E402

HBM = 8e12
BPP = 6
SRC = ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0)
TARGETS = {"log12_luv8": ((L.PTF_LOG, 12, L.CS_LUV, 8, 1e4, 0.005), 1.0),
           "pq10_ycbcr10": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_distortion.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="one target, e.g. pq10_ycbcr10 (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="fused, replaced or transcode: that leg only, one round, nothing written")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    s = torch.cuda.current_stream()
    scfg, src_sc = SRC

    def at(t, b):
        return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

    # the archive: nb batches of B frames as PQ-11 Lu'v' planes (the float frames exist only to make them)
    src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
    cs = L.Context(0)
    cs.set_stream(s.cuda_stream)
    cs.set_quantizer(*scfg, L.build_lut(scfg[0], scfg[1], scfg[4], scfg[5]))
    f32 = torch.empty(B * n3, dtype=torch.float32, device=dev)
    for b in range(nb):
        cs.synth_frames_device(f32.data_ptr(), n3, B, w, h)
        f32 *= 1.0 + 0.25 * b   # (distinct batches)
        cs.encode_frames_device(f32.data_ptr(), n3, B, w, h, src_sc, profile, at(src, b), st, psz)
    torch.cuda.synchronize()
    cs.close()
    del f32
    torch.cuda.empty_cache()

    rows = []
    for name, (cfg, dst_sc) in TARGETS.items():
        if a.only and a.only != name:
            continue
        tag = "pq11_luv8->" + name
        c = L.Context(0)
        c.set_stream(s.cuda_stream)
        c.set_quantizer(*cfg, L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5]))
        c.set_source_quantizer(*scfg, L.build_lut(scfg[0], scfg[1], scfg[4], scfg[5]))
        given = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        scratch = [torch.zeros(B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        out_f = torch.zeros(nb, B, 3, 4, dtype=torch.int64, device=dev)
        out_r = torch.zeros(nb, B, 3, 4, dtype=torch.int64, device=dev)
        for b in range(nb):
            c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile, dst_sc * 1.02)

        def launch(leg, b):
            if leg == "fused":
                c.transcode_distortion_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, at(given, b), st, psz, profile, dst_sc,
                                                     out_f[b].data_ptr())
                return
            c.transcode_frames_device(at(src, b), st, psz, profile, src_sc, B, w, h, [t.data_ptr() for t in scratch], st, psz, profile, dst_sc)
            if leg == "replaced":
                torch_reduction(scratch, [given[p][b * B * psz[p]:(b + 1) * B * psz[p]] for p in range(3)], B, out_r[b])

        for b in range(nb):   # the two legs compute the same integers
            launch("fused", b)
            launch("replaced", b)
        torch.cuda.synchronize()
        if not torch.equal(out_f, out_r):
            raise SystemExit("%s: the fused launch and the replaced method disagree" % tag)
        differing = float(out_f[..., 3].sum()) / (nb * B * 1.5 * n)

        def timed(leg, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        legs = [a.leg] if a.leg else ["fused", "replaced", "transcode"]
        iters = {}
        for leg in legs:   # warm-up, and how many launches make --min-s of device time
            timed(leg, 4)
            iters[leg] = max(4, int(a.min_s * 1e3 / timed(leg, 8)) + 1)
        res = {leg: [] for leg in legs}
        for r in range(1 if a.leg else a.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                res[leg].append(timed(leg, iters[leg]))
        if a.leg:
            print("%s  %s: %.4f ms per launch" % (tag, a.leg, res[a.leg][0]))
        else:
            med = {leg: sorted(v)[len(v) // 2] for leg, v in res.items()}
            mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
            rows.append(dict(workload=tag, frames_per_launch=B, w=w, h=h, profile=profile, src_sc=src_sc, dst_sc=dst_sc,
                             samples_differing=round(differing, 3), ms={leg: round(med[leg], 4) for leg in legs},
                             mpixel_s={leg: round(mpx[leg], 1) for leg in legs},
                             fused_over_replaced=round(mpx["fused"] / mpx["replaced"], 3), bytes_per_pixel=BPP,
                             fused_hbm_fraction_8tbs=round(mpx["fused"] * 1e6 * BPP / HBM, 3),
                             transcode_hbm_fraction_8tbs=round(mpx["transcode"] * 1e6 * BPP / HBM, 3),
                             spread={leg: round(max(v) / min(v) - 1, 4) for leg, v in res.items()}, launches_per_round=iters))
        c.close()
        del given, scratch, out_f, out_r
        torch.cuda.empty_cache()
    for r in rows:
        print("%-26s fused %8.4f ms | replaced %8.4f ms | transcode alone %8.4f ms | fused x%.3f of replaced | of 8 TB/s at %d B/px: "
              "fused %.3f, transcode %.3f | spread %s" % (r["workload"], r["ms"]["fused"], r["ms"]["replaced"], r["ms"]["transcode"],
                                                        r["fused_over_replaced"], r["bytes_per_pixel"], r["fused_hbm_fraction_8tbs"],
                                                        r["transcode_hbm_fraction_8tbs"], r["spread"]))
    if a.out and rows:
        line = dict(rounds=a.rounds, min_s=a.min_s, kernel_source_sha=capi.kernel_source_sha(), device=torch.cuda.get_device_name(0),
                    workloads=rows)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
