#!/usr/bin/env python3
"""tools/bench/transcode_half.py [--rounds R] [--min-s S] [--out FILE] -- the half-resolution transcode launch against the method it
replaces and against the full-resolution transcode launch on the same source.

Pairs: PQ-11 Lu'v' -> LOG-12 Lu'v' and PQ-11 Lu'v' -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20), profile 2 on both
sides, 8 source frames of 3840x2160 per launch (1920x1080 out), ordered launches on one stream, plain allocations, one process on
one box.  The source planes are real code planes (synthetic frames encoded under the source quantizer), four distinct batches.
Legs, interleaved round by round:
  fused     lumahip_transcode_half_frames_device;
  replaced  lumahip_decode_frames_device into a float buffer, torch's ((a + b) + (c + d)) * 0.25 on strided views of it into a
            half-size float buffer (four launches), lumahip_encode_frames_device from that;
  parent    lumahip_transcode_frames_device on the same source planes: the full-resolution launch, which reads the same bytes and
            does four times the encode work.
Once, before anything is timed: fused and replaced give the same planes, byte for byte.  Per leg and round: hipEvent time of
back-to-back launches, at least --min-s seconds of device time; the median round is reported.
-> profiles/transcode_half.jsonl: one JSON line per pair APPENDED, with ms and source Mpixel/s of each leg, fused over replaced (the
gate: <= 1 + the larger spread of the two legs' rounds), fused over parent, and the spread of the rounds (max / min - 1 per leg)."""
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
LEGS = ["fused", "replaced", "parent"]


def lut(cfg):
    return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_half.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="SRC:DST, one pair (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="fused, replaced or parent: that leg only, one round, nothing written (for rocprofv3 captures)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    tw, th = w // 2, h // 2
    n, n3, tn3 = w * h, 3 * w * h, 3 * tw * th
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    _, ths, tst, _ = L.plane_geometry(tw, th, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    tpsz = [ths[p] * tst[p] for p in range(3)]
    s = torch.cuda.current_stream()
    rows = []
    for sname, dname in PAIRS:
        if a.only and a.only != "%s:%s" % (sname, dname):
            continue
        (scfg, ssc), (dcfg, dsc) = CFG[sname], CFG[dname]
        cs, ct = L.Context(0), L.Context(0)   # cs: the source as a quantizer (encodes the inputs, decodes in the replaced leg)
        for c in (cs, ct):
            c.set_stream(s.cuda_stream)
        cs.set_quantizer(*scfg, lut(scfg))
        ct.set_quantizer(*dcfg, lut(dcfg))
        ct.set_source_quantizer(*scfg, lut(scfg))
        frames = torch.empty(B * n3, dtype=torch.float32, device=dev)   # the replaced leg's decoded frames, and the inputs' staging
        small = torch.empty(B * tn3, dtype=torch.float32, device=dev)   # ... and its averaged frames
        tmp = torch.empty(B * tn3, dtype=torch.float32, device=dev)
        v = frames.view(B, 3, h, w)
        v00, v01, v10, v11 = v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]
        sm, tm = small.view(B, 3, th, tw), tmp.view(B, 3, th, tw)
        src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        half = [torch.zeros(nb * B * tpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        full = [torch.zeros(B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]   # the parent leg's destination

        def at(t, b, sz):
            return [t[p].data_ptr() + b * B * sz[p] for p in range(3)]

        for b in range(nb):
            cs.synth_frames_device(frames.data_ptr(), n3, B, w, h, first_frame=b * B)
            cs.encode_frames_device(frames.data_ptr(), n3, B, w, h, ssc, profile, at(src, b, psz), st, psz)

        def launch(leg, b, out=half):
            if leg == "fused":
                ct.transcode_half_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, at(out, b, tpsz), tst, tpsz, profile, dsc)
            elif leg == "replaced":
                cs.decode_frames_device(at(src, b, psz), st, psz, B, w, h, profile, ssc, frames.data_ptr(), n3)
                torch.add(v00, v01, out=sm)
                torch.add(v10, v11, out=tm)
                sm.add_(tm)
                sm.mul_(0.25)
                ct.encode_frames_device(small.data_ptr(), tn3, B, tw, th, dsc, profile, at(out, b, tpsz), tst, tpsz)
            else:
                ct.transcode_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, [t.data_ptr() for t in full], st, psz, profile, dsc)

        # once: the two methods give the same planes
        other = [torch.zeros_like(t) for t in half]
        for b in range(nb):
            launch("fused", b)
            launch("replaced", b, other)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(x, y)) for x, y in zip(half, other)) and any(bool(t.any()) for t in half)
        if not same:
            raise SystemExit("%s -> %s: the fused launch and the replaced method write different planes" % (sname, dname))
        del other

        def timed(leg, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, i % nb)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        legs = [a.leg] if a.leg else LEGS
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
        else:
            rows.append(result_row(a, sname, dname, B, n, w, h, profile, same, legs, res, iters))
        for c in (cs, ct):
            c.close()
        del frames, small, tmp, v, v00, v01, v10, v11, sm, tm, src, half, full
        torch.cuda.empty_cache()
    for r in rows:
        print("%-28s fused %8.4f ms | replaced %8.4f ms (fused / replaced %.3f, gate %s) | parent %8.4f ms (fused / parent %.3f) | spread %s" %
              (r["pair"], r["fused_ms"], r["replaced_ms"], r["fused_over_replaced"], "passed" if r["gate_passed"] else "MISSED",
               r["parent_ms"], r["fused_over_parent"], r["spread"]))
    if a.out and rows:
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


def result_row(a, sname, dname, B, n, w, h, profile, same, legs, res, iters):
    """the JSON line of one pair: the median round of every leg, the ratios, the gate and the spread of the rounds"""
    med = {leg: sorted(x)[len(x) // 2] for leg, x in res.items()}
    mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
    spread = {leg: round(max(x) / min(x) - 1, 4) for leg, x in res.items()}
    margin = max(spread["fused"], spread["replaced"])
    return dict(pair="%s->%s" % (sname, dname), frames_per_launch=B, w=w, h=h, profile=profile, planes_equal=same,
                fused_ms=round(med["fused"], 4), replaced_ms=round(med["replaced"], 4), parent_ms=round(med["parent"], 4),
                fused_source_mpixel_s=round(mpx["fused"], 1), replaced_source_mpixel_s=round(mpx["replaced"], 1),
                parent_source_mpixel_s=round(mpx["parent"], 1),
                fused_over_replaced=round(med["fused"] / med["replaced"], 3), gate_margin=margin,
                gate_passed=bool(med["fused"] <= med["replaced"] * (1 + margin)),
                fused_over_parent=round(med["fused"] / med["parent"], 3),
                spread=spread, rounds=a.rounds, launches_per_round=iters, kernel_source_sha=capi.kernel_source_sha(),
                device=torch.cuda.get_device_name(0))

if __name__ == "__main__":
    main()
