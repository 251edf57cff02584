#!/usr/bin/env python3
"""tools/bench/transcode.py [--rounds R] [--min-s S] [--out FILE] -- the fused transcode launch against the two launches it replaces.

Pairs: PQ-11 Lu'v' -> LOG-12 Lu'v' and PQ-11 Lu'v' -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20), profile 2 on both
sides, 8 frames of 3840x2160 per launch, ordered launches on one stream, plain allocations, one process on one box.  The source
planes are real code planes (synthetic frames encoded under the source quantizer), four distinct batches.  Legs, interleaved
round by round: `fused` = lumahip_transcode_frames_device; `pair` = lumahip_decode_frames_device into a float buffer followed
by lumahip_encode_frames_device from it (the existing kernels, which this tool does not change).  Per leg and round: hipEvent
time of back-to-back launches, at least --min-s seconds of device time; the median round is reported.
-> profiles/transcode.jsonl: one JSON line per pair with Mpixel/s of each leg, their ratio, the fused leg's fraction of 8 TB/s at
its 6 B/pixel, and the spread of the rounds (max / min - 1 per leg: what the box does to repeated identical runs)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402

HBM = 8e12
CFG = {"pq11_luv8": ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "log12_luv8": ((L.PTF_LOG, 12, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "pq10_ycbcr10": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}
PAIRS = [("pq11_luv8", "log12_luv8"), ("pq11_luv8", "pq10_ycbcr10")]


def lut(cfg):
    return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="SRC:DST, one pair (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="fused or pair: that leg only, one round, nothing written (for rocprofv3 captures)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    s = torch.cuda.current_stream()
    rows = []
    for sname, dname in PAIRS:
        if a.only and a.only != "%s:%s" % (sname, dname):
            continue
        (scfg, ssc), (dcfg, dsc) = CFG[sname], CFG[dname]
        cs, ct = L.Context(0), L.Context(0)   # cs: the source as a quantizer (encodes the inputs, decodes in the pair leg)
        for c in (cs, ct):
            c.set_stream(s.cuda_stream)
        cs.set_quantizer(*scfg, lut(scfg))
        ct.set_quantizer(*dcfg, lut(dcfg))
        ct.set_source_quantizer(*scfg, lut(scfg))
        frames = torch.empty(B * n3, dtype=torch.float32, device=dev)   # the pair leg's intermediate, and the inputs' staging
        src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        dst = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]

        def at(t, b):
            return [t[p].data_ptr() + b * B * psz[p] for p in range(3)]

        for b in range(nb):
            cs.synth_frames_device(frames.data_ptr(), n3, B, w, h, first_frame=b * B)
            cs.encode_frames_device(frames.data_ptr(), n3, B, w, h, ssc, profile, at(src, b), st, psz)

        def launch(leg, b):
            if leg == "fused":
                ct.transcode_frames_device(at(src, b), st, psz, profile, ssc, B, w, h, at(dst, b), st, psz, profile, dsc)
            else:
                cs.decode_frames_device(at(src, b), st, psz, B, w, h, profile, ssc, frames.data_ptr(), n3)
                ct.encode_frames_device(frames.data_ptr(), n3, B, w, h, dsc, profile, at(dst, b), st, psz)

        def timed(leg, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        legs = [a.leg] if a.leg else ["fused", "pair"]
        iters = {}
        for leg in legs:   # warm-up, and how many launches make --min-s of device time
            timed(leg, 4)
            iters[leg] = max(4, int(a.min_s * 1e3 / timed(leg, 8)) + 1)
        res = {leg: [] for leg in legs}
        for r in range(1 if a.leg else a.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                res[leg].append(timed(leg, iters[leg]))
        if a.leg:
            print("%s -> %s  %s: %.4f ms per launch" % (sname, dname, a.leg, res[a.leg][0]))
            continue
        med = {leg: sorted(v)[len(v) // 2] for leg, v in res.items()}
        mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
        rows.append(dict(pair="%s->%s" % (sname, dname), frames_per_launch=B, w=w, h=h, profile=profile,
                         fused_ms=round(med["fused"], 4), pair_ms=round(med["pair"], 4),
                         fused_mpixel_s=round(mpx["fused"], 1), pair_mpixel_s=round(mpx["pair"], 1),
                         fused_over_pair=round(mpx["fused"] / mpx["pair"], 3),
                         fused_hbm_fraction_8tbs_at_6B=round(mpx["fused"] * 1e6 * 6 / HBM, 3),
                         spread={leg: round(max(v) / min(v) - 1, 4) for leg, v in res.items()},
                         rounds=a.rounds, launches_per_round=iters, kernel_source_sha=capi.kernel_source_sha(),
                         device=torch.cuda.get_device_name(0)))
        for c in (cs, ct):
            c.close()
        del frames, src, dst
        torch.cuda.empty_cache()
    for r in rows:
        print("%-28s fused %8.4f ms %9.1f Mpx/s | pair %8.4f ms %9.1f Mpx/s | x%.3f | %.3f of 8 TB/s at 6 B/px | spread %s" %
              (r["pair"], r["fused_ms"], r["fused_mpixel_s"], r["pair_ms"], r["pair_mpixel_s"], r["fused_over_pair"],
               r["fused_hbm_fraction_8tbs_at_6B"], r["spread"]))
    if a.out and rows:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
