#!/usr/bin/env python3
"""tools/bench/transcode_quarter.py [--rounds R] [--min-s S] [--out FILE] [--sweep FILE] -- the quarter-resolution transcode launch
(include/lumahip_rungs.h) against the method it replaces, against the half-resolution launch on the same source and against two
chained half-resolution launches.

Pairs: PQ-11 Lu'v' -> LOG-12 Lu'v' and PQ-11 Lu'v' -> the HDR10 Y'CbCr recipe (PQ-10, 10-bit colour, sc 20), profile 2 on both
sides, 8 source frames of 3840x2160 per launch (960x540 out), ordered launches on one stream, plain allocations, one process on one
box.  The source planes are real code planes (synthetic frames encoded under the source quantizer), four distinct batches.
Legs, interleaved round by round:
  fused     lumahip_transcode_quarter_frames_device;
  replaced  lumahip_decode_frames_device into a float buffer, torch's ((a + b) + (c + d)) * 0.25 on strided views twice (eight
            launches), lumahip_encode_frames_device from the quarter-size float buffer;
  half      lumahip_transcode_half_frames_device on the same source planes: it reads the same bytes and encodes four times the pixels;
  chained   two half-resolution launches through a scratch rung under the target quantizer (a second context has the target's as
            its source quantizer).  Informational: its planes are ANOTHER picture -- two roundings to codes in the place of one --
            and are not compared.
Once, before anything is timed: fused and replaced give the same planes, byte for byte.  Per leg and round: hipEvent time of
back-to-back launches, at least --min-s seconds of device time; the median round is reported.
-> profiles/transcode_quarter.jsonl: one JSON line per pair APPENDED, with ms and source Mpixel/s of each leg, fused over replaced
(the gate: <= 1 + the larger spread of the two legs' rounds), fused over half, fused over chained, the spread of the rounds (max /
min - 1 per leg) and the fraction of 8 TB/s the fused launch's 3.1875 B per source pixel come to.
--sweep FILE: instead, the fused launch alone under other launch shapes (lumahip_tune "block" / "blocks_per_cu"), a context of its own
per shape, shapes interleaved, median of 3 rounds, at 8 x 4K and at one 4K frame; the table is written to FILE."""
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
LEGS = ["fused", "replaced", "half", "chained"]
BYTES_PER_SOURCE_PIXEL = 3.0 + 3.0 / 16.0   # profile 2 -> 2: 3 read, 3/16 written
SHAPES = [("default", ()), ("block 256", (("block", 256),)), ("block 512", (("block", 512),)), ("block 1024", (("block", 1024),)),
          ("block 256, 2 per CU", (("block", 256), ("blocks_per_cu", 2))), ("block 256, 4 per CU", (("block", 256), ("blocks_per_cu", 4))),
          ("block 512, 1 per CU", (("block", 512), ("blocks_per_cu", 1))), ("block 512, 2 per CU", (("block", 512), ("blocks_per_cu", 2)))]


def lut(cfg):
    return L.build_lut(cfg[0], cfg[1], cfg[4], cfg[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-s", type=float, default=1.0, help="device time per leg and round")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_quarter.jsonl"), help="'' = print only")
    ap.add_argument("--only", default="", help="SRC:DST, one pair (for rocprofv3 captures)")
    ap.add_argument("--leg", default="", help="one of the legs only, one round, nothing written (for rocprofv3 captures)")
    ap.add_argument("--sweep", default="", help="write the launch-shape sweep of the fused launch to this file and nothing else")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, B, nb, profile = 3840, 2160, a.frames, 4, 2
    hw, hh, tw, th = w // 2, h // 2, w // 4, h // 4
    n, n3, hn3, tn3 = w * h, 3 * w * h, 3 * hw * hh, 3 * tw * th
    _, hs, st, _ = L.plane_geometry(w, h, profile)
    _, hhs, hst, _ = L.plane_geometry(hw, hh, profile)
    _, ths, tst, _ = L.plane_geometry(tw, th, profile)
    psz = [hs[p] * st[p] for p in range(3)]
    hpsz = [hhs[p] * hst[p] for p in range(3)]
    tpsz = [ths[p] * tst[p] for p in range(3)]
    s = torch.cuda.current_stream()
    rows, sweep = [], []
    for sname, dname in PAIRS:
        if a.only and a.only != "%s:%s" % (sname, dname):
            continue
        (scfg, ssc), (dcfg, dsc) = CFG[sname], CFG[dname]
        # cs: the source as a quantizer (encodes the inputs, decodes in the replaced leg); c2: the second launch of the chained leg
        cs, ct, c2 = L.Context(0), L.Context(0), L.Context(0)
        for c in (cs, ct, c2):
            c.set_stream(s.cuda_stream)
        cs.set_quantizer(*scfg, lut(scfg))
        ct.set_quantizer(*dcfg, lut(dcfg))
        ct.set_source_quantizer(*scfg, lut(scfg))
        c2.set_quantizer(*dcfg, lut(dcfg))
        c2.set_source_quantizer(*dcfg, lut(dcfg))
        frames = torch.empty(B * n3, dtype=torch.float32, device=dev)   # the replaced leg's decoded frames, and the inputs' staging
        mid = torch.empty(B * hn3, dtype=torch.float32, device=dev)     # ... its half-size means
        mtmp = torch.empty(B * hn3, dtype=torch.float32, device=dev)
        small = torch.empty(B * tn3, dtype=torch.float32, device=dev)   # ... and its quarter-size frames
        stmp = torch.empty(B * tn3, dtype=torch.float32, device=dev)
        v, mv, mt = frames.view(B, 3, h, w), mid.view(B, 3, hh, hw), mtmp.view(B, 3, hh, hw)
        sm, tm = small.view(B, 3, th, tw), stmp.view(B, 3, th, tw)
        src = [torch.zeros(nb * B * psz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        quarter = [torch.zeros(nb * B * tpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]
        rung = [torch.zeros(B * hpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]   # the half and chained legs' half-size planes
        low = [torch.zeros(B * tpsz[p], dtype=torch.uint8, device=dev) for p in range(3)]    # the chained leg's destination

        def at(t, b, sz):
            return [t[p].data_ptr() + b * B * sz[p] for p in range(3)]

        def ptrs(t):
            return [x.data_ptr() for x in t]

        for b in range(nb):
            cs.synth_frames_device(frames.data_ptr(), n3, B, w, h, first_frame=b * B)
            cs.encode_frames_device(frames.data_ptr(), n3, B, w, h, ssc, profile, at(src, b, psz), st, psz)

        def box(x, out, tmp):
            torch.add(x[..., 0::2, 0::2], x[..., 0::2, 1::2], out=out)
            torch.add(x[..., 1::2, 0::2], x[..., 1::2, 1::2], out=tmp)
            out.add_(tmp)
            out.mul_(0.25)

        def launch(leg, b, out=quarter, c=ct, nf=B):
            if leg == "fused":
                c.transcode_quarter_frames_device(at(src, b, psz), st, psz, profile, ssc, nf, w, h, at(out, b, tpsz), tst, tpsz, profile, dsc)
            elif leg == "replaced":
                cs.decode_frames_device(at(src, b, psz), st, psz, B, w, h, profile, ssc, frames.data_ptr(), n3)
                box(v, mv, mt)
                box(mv, sm, tm)
                ct.encode_frames_device(small.data_ptr(), tn3, B, tw, th, dsc, profile, at(out, b, tpsz), tst, tpsz)
            elif leg == "half":
                ct.transcode_half_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, ptrs(rung), hst, hpsz, profile, dsc)
            else:
                ct.transcode_half_frames_device(at(src, b, psz), st, psz, profile, ssc, B, w, h, ptrs(rung), hst, hpsz, profile, dsc)
                c2.transcode_half_frames_device(ptrs(rung), hst, hpsz, profile, dsc, B, hw, hh, ptrs(low), tst, tpsz, profile, dsc)

        # once: the two methods give the same planes
        other = [torch.zeros_like(t) for t in quarter]
        for b in range(nb):
            launch("fused", b)
            launch("replaced", b, other)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(x, y)) for x, y in zip(quarter, other)) and any(bool(t.any()) for t in quarter)
        if not same:
            raise SystemExit("%s -> %s: the fused launch and the replaced method write different planes" % (sname, dname))
        del other

        def timed(leg, iters, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(iters):
                launch(leg, i % nb, **kw)
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        if a.sweep:
            ctxs = []
            for name, tunes in SHAPES:
                c = L.Context(0)
                c.set_stream(s.cuda_stream)
                c.set_quantizer(*dcfg, lut(dcfg))
                c.set_source_quantizer(*scfg, lut(scfg))
                for k, val in tunes:
                    c.tune(k, val)
                ctxs.append(c)
            for nf in (B, 1):
                its = max(8, int(0.3e3 / timed("fused", 8, nf=nf)) + 1)
                res = {name: [] for name, _ in SHAPES}
                for r in range(3):
                    order = list(zip(SHAPES, ctxs))
                    for (name, _), c in (order if r % 2 == 0 else order[::-1]):
                        timed("fused", 4, c=c, nf=nf)
                        res[name].append(timed("fused", its, c=c, nf=nf))
                for name, _ in SHAPES:
                    x = sorted(res[name])
                    sweep.append("%-26s %d x 3840x2160  %-22s median %8.4f ms   rounds %s   spread %.4f" %
                                 ("%s->%s" % (sname, dname), nf, name, x[1], " ".join("%.4f" % t for t in res[name]), x[-1] / x[0] - 1))
            for c in ctxs:
                c.close()
        else:
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
        for c in (cs, ct, c2):
            c.close()
        del frames, mid, mtmp, small, stmp, v, mv, mt, sm, tm, src, quarter, rung, low
        torch.cuda.empty_cache()
    if a.sweep:
        head = ("lumahip_transcode_quarter_frames_device alone under other launch shapes (lumahip_tune), a context of its own per shape, shapes\n"
                "interleaved, 3 rounds of >= 0.3 s of device time each, profile 2 -> 2, %s, kernel sources %s\n"
                % (torch.cuda.get_device_name(0), capi.kernel_source_sha()))
        with open(a.sweep, "w") as f:
            f.write(head + "\n".join(sweep) + "\n")
        print(head + "\n".join(sweep))
        return
    for r in rows:
        print("%-28s fused %8.4f ms | replaced %8.4f ms (fused / replaced %.3f, gate %s) | half %8.4f ms (fused / half %.3f) | chained %8.4f ms "
              "(fused / chained %.3f, planes differ by definition: not compared) | spread %s" %
              (r["pair"], r["fused_ms"], r["replaced_ms"], r["fused_over_replaced"], "met" if r["gate_passed"] else "MISSED",
               r["half_ms"], r["fused_over_half"], r["chained_ms"], r["fused_over_chained"], r["spread"]))
    if a.out and rows:
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


def result_row(a, sname, dname, B, n, w, h, profile, same, legs, res, iters):
    """the JSON line of one pair: the median round of every leg, the ratios, the gate and the spread of the rounds"""
    med = {leg: sorted(x)[len(x) // 2] for leg, x in res.items()}
    mpx = {leg: B * n / (med[leg] * 1e-3) / 1e6 for leg in legs}
    spread = {leg: round(max(x) / min(x) - 1, 4) for leg, x in res.items()}
    margin = max(spread["fused"], spread["replaced"])
    row = dict(pair="%s->%s" % (sname, dname), frames_per_launch=B, w=w, h=h, profile=profile, planes_equal=same)
    for leg in legs:
        row[leg + "_ms"] = round(med[leg], 4)
        row[leg + "_source_mpixel_s"] = round(mpx[leg], 1)
    row.update(fused_over_replaced=round(med["fused"] / med["replaced"], 3), gate_margin=margin,
               gate_passed=bool(med["fused"] <= med["replaced"] * (1 + margin)),
               fused_over_half=round(med["fused"] / med["half"], 3), fused_over_chained=round(med["fused"] / med["chained"], 3),
               chained_planes="differ by definition, not compared",
               fused_fraction_of_8TBs=round(mpx["fused"] * 1e6 * BYTES_PER_SOURCE_PIXEL / 8e12, 4),
               spread=spread, rounds=a.rounds, launches_per_round=iters, kernel_source_sha=capi.kernel_source_sha(),
               device=torch.cuda.get_device_name(0))
    return row


if __name__ == "__main__":
    main()
