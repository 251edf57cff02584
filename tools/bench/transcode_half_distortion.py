#!/usr/bin/env python3
"""tools/bench/transcode_half_distortion.py [--rounds R] [--min-s S] [--out FILE] [--vw2] -- the half-resolution transcode distortion
launches (include/lumahip_ladder.h) against the method they replace and against the half-resolution transcode launch alone.

Pairs: PQ-11 Lu'v' -> LOG-12 Lu'v' and PQ-11 Lu'v' -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20), profile 2 on both
sides, 8 source frames of 3840x2160 per launch (given planes of 1920x1080), ordered launches on one stream, plain allocations, one
process on one box.  The source planes are real code planes (synthetic frames encoded under the source quantizer), four distinct
batches; the given planes are their half-resolution transcode with every 97th byte changed.
Calls: the per-frame words, and the map at blocks of 16 and of 64.  Legs, interleaved round by round:
  fused     lumahip_transcode_half_distortion_frames_device / lumahip_transcode_half_distortion_map_frames_device;
  replaced  lumahip_transcode_half_frames_device into scratch planes, then lumahip_planes_distortion_frames_device /
            lumahip_planes_distortion_map_frames_device on them;
  half      lumahip_transcode_half_frames_device alone: what the fused launch computes, without the comparison;
  vw2       (--vw2 only) the fused launch on copies of both plane sets 4 bytes off their 8-byte alignment, which makes the plan take
            two pixels per thread: the A/B of a family's vector width.
Once, before anything is timed: fused, replaced (and vw2) give the same integers.  Per leg and round: hipEvent time of back-to-back
launches, at least --min-s seconds of device time; the median round is reported.
-> profiles/transcode_half_distortion.jsonl: one JSON line per pair and call APPENDED, with ms and source Mpixel/s of each leg, fused
over replaced (the gate: <= 1 + the larger spread of the two legs' rounds), fused over half, and the spread of the rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lumahdrv_amd as L  # noqa: E402
from lumahdrv_amd import capi  # noqa: E402

CFG = {"pq11_luv8": ((L.PTF_PQ, 11, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "log12_luv8": ((L.PTF_LOG, 12, L.CS_LUV, 8, 1e4, 0.005), 1.0),
       "pq10_ycbcr10": ((L.PTF_PQ, 10, L.CS_YCBCR, 10, 1000.0, 0.01), 20.0)}
PAIRS = [("pq11_luv8", "log12_luv8"), ("pq11_luv8", "pq10_ycbcr10")]
CALLS = [("words", None), ("map16", 16), ("map64", 64)]
OFF = 4   # bytes the vw2 leg's planes lie off their alignment


def lut(cfg):
    return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_half_distortion.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="SRC:DST, one pair")
    ap.add_argument("--vw2", action="store_true", help="add the vw2 leg")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    tw, th = w // 2, h // 2
    n, n3 = w * h, 3 * w * h
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    _, ths, tst, _ = L.plane_geometry(tw, th, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    tpsz = [ths[p] * tst[p] for p in range(3)]
    s = torch.cuda.current_stream()
    legs = ["fused", "replaced", "half"] + (["vw2"] if a.vw2 else [])
    rows = []
    for sname, dname in PAIRS:
        if a.only and a.only != "%s:%s" % (sname, dname):
            continue
        (scfg, ssc), (dcfg, dsc) = CFG[sname], CFG[dname]
        cs, ct = L.Context(0), L.Context(0)   # cs: the source as a quantizer (encodes the inputs)
        for c in (cs, ct):
            c.set_stream(s.cuda_stream)
        cs.set_quantizer(*scfg, lut(scfg))
        ct.set_quantizer(*dcfg, lut(dcfg))
        ct.set_source_quantizer(*scfg, lut(scfg))
        frames = torch.empty(B * n3, dtype=torch.float32, device=dev)
        src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        given = [torch.zeros(nb * B * tpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        scratch = [torch.zeros(B * tpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]

        def at(t, b, sz, off=0):
            return [t[p].data_ptr() + off + b * B * sz[p] for p in range(3)]

        for b in range(nb):
            cs.synth_frames_device(frames.data_ptr(), n3, B, w, h, first_frame=b * B)
            cs.encode_frames_device(frames.data_ptr(), n3, B, w, h, ssc, profile, at(src, b, psz), st, psz)
            ct.transcode_half_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, at(given, b, tpsz), tst, tpsz, profile, dsc)
        torch.cuda.synchronize()
        del frames
        for t in given:
            t[::97] ^= 1
        src2 = given2 = None
        if a.vw2:   # the same bytes OFF bytes into buffers of their own
            src2 = [torch.cat([torch.zeros(OFF, dtype=torch.uint8, device=dev), t]) for t in src]
            given2 = [torch.cat([torch.zeros(OFF, dtype=torch.uint8, device=dev), t]) for t in given]

        for call, block in CALLS:
            nbx, nby = (1, 1) if block is None else L.distortion_map_dims(tw, th, block)
            out = {leg: torch.zeros(B * nbx * nby * 12, dtype=torch.int64, device=dev) for leg in legs}

            def launch(leg, b):
                o = out[leg].data_ptr()
                if leg in ("fused", "vw2"):
                    sp, gp = (at(src, b, psz), at(given, b, tpsz)) if leg == "fused" else (at(src2, b, psz, OFF), at(given2, b, tpsz, OFF))
                    args = (sp, st, psz, profile, ssc, B, w, h, gp, tst, tpsz, profile, dsc)
                    if block is None:
                        ct.transcode_half_distortion_frames_device(*args, o)
                    else:
                        ct.transcode_half_distortion_map_frames_device(*args, block, o)
                    return
                sc_ptrs = [t.data_ptr() for t in scratch]
                ct.transcode_half_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, sc_ptrs, tst, tpsz, profile, dsc)
                if leg == "replaced":
                    args = (sc_ptrs, tst, tpsz, B, tw, th, at(given, b, tpsz), tst, tpsz, profile)
                    if block is None:
                        ct.planes_distortion_frames_device(*args, o)
                    else:
                        ct.planes_distortion_map_frames_device(*args, block, o)

            # once: the methods give the same integers, and they are not all zero
            same = True
            for b in range(nb):
                for leg in legs:
                    launch(leg, b)
                torch.cuda.synchronize()
                same = same and all(bool(torch.equal(out["fused"], out[leg])) for leg in legs if leg not in ("fused", "half"))
                same = same and bool(out["fused"].any())
            if not same:
                raise SystemExit("%s -> %s %s: the fused launch and the replaced method give different words" % (sname, dname, call))

            def timed(leg, iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for i in range(iters):
                    launch(leg, i % nb)
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1) / iters

            iters = {}
            for leg in legs:   # warm-up, and how many launches make --min-s of device time
                timed(leg, 4)
                iters[leg] = max(4, int(a.min_s * 1e3 / timed(leg, 8)) + 1)
            res = {leg: [] for leg in legs}
            for r in range(a.rounds):
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    res[leg].append(timed(leg, iters[leg]))
            rows.append(result_row(a, sname, dname, call, block, B, n, w, h, profile, same, legs, res, iters))
            print(line_of(rows[-1]), flush=True)
        for c in (cs, ct):
            c.close()
        del src, given, scratch, src2, given2
        torch.cuda.empty_cache()
    if a.out and rows:
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


def line_of(r):
    vw2 = " | vw2 %8.4f ms (vw2 / fused %.3f)" % (r["vw2_ms"], r["vw2_over_fused"]) if "vw2_ms" in r else ""
    return ("%-28s %-6s fused %8.4f ms | replaced %8.4f ms (fused / replaced %.3f, gate %s) | half alone %8.4f ms (fused / half %.3f)%s | spread %s" %
            (r["pair"], r["call"], r["fused_ms"], r["replaced_ms"], r["fused_over_replaced"], "passed" if r["gate_passed"] else "MISSED",
             r["half_ms"], r["fused_over_half"], vw2, r["spread"]))


def result_row(a, sname, dname, call, block, B, n, w, h, profile, same, legs, res, iters):
    """the JSON line of one pair and call: the median round of every leg, the ratios, the gate and the spread of the rounds"""
    med = {leg: sorted(x)[len(x) // 2] for leg, x in res.items()}
    mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
    spread = {leg: round(max(x) / min(x) - 1, 4) for leg, x in res.items()}
    margin = max(spread["fused"], spread["replaced"])
    row = dict(pair="%s->%s" % (sname, dname), call=call, block=block, frames_per_launch=B, w=w, h=h, profile=profile, words_equal=same,
               fused_ms=round(med["fused"], 4), replaced_ms=round(med["replaced"], 4), half_ms=round(med["half"], 4),
               fused_source_mpixel_s=round(mpx["fused"], 1), replaced_source_mpixel_s=round(mpx["replaced"], 1),
               half_source_mpixel_s=round(mpx["half"], 1),
               fused_over_replaced=round(med["fused"] / med["replaced"], 3), gate_margin=margin,
               gate_passed=bool(med["fused"] <= med["replaced"] * (1 + margin)),
               fused_over_half=round(med["fused"] / med["half"], 3))
    if "vw2" in med:
        row.update(vw2_ms=round(med["vw2"], 4), vw2_over_fused=round(med["vw2"] / med["fused"], 3))
    row.update(spread=spread, rounds=a.rounds, launches_per_round=iters, kernel_source_sha=capi.kernel_source_sha(),
               device=torch.cuda.get_device_name(0))
    return row


if __name__ == "__main__":
    main()
