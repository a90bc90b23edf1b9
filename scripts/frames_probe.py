#!/usr/bin/env python3
"""Frames -> verdict bits against the router on the same frames, one run, one ctx.

Builds bench.py's config-4 batch (2^20 frames in 2 KiB slots: 2 GiB, past the Infinity Cache) and
a dense 144-byte-slot ring of the same frames, and after a warm-up takes medians of --reps runs of
  hfv_extract_records_timed, hfv_verify_batches_timed over the 24-byte records, the whole
  hfv_verify_frames region (torch events), the region without the mask kernel (extract +
  verify_batches, torch events), the mask kernel alone (hfv_debug_mask_status, torch events), and
  hfv_br_process_timed on the same frames,
plus a streaming read of the frame buffer (hfv_debug_stream_read, as bench.py uses) and the
extract kernel's algorithmic bytes: per frame the 64-byte lines that hold the fields the parser
reads, + 24 written + 3 of len/status.  Prints one JSON object and writes it to --out.

  timeout -k 10 300 python scripts/frames_probe.py [--direct] [--extract-only] [--slots 2048,144] [--rx]

--direct places the frame buffer 8 bytes off a 16-byte boundary, which the staged kernel's 16-byte
loads cannot take: the library then runs the direct kernel (every field read from global memory),
the alternative of the A/B in profiles/ab_index.md.

--rx adds, per slot under "rx", the direction-aware path (hfv_extract_records_rx /
hfv_verify_frames_rx) with the mix's own ifindex array and BR 1's internal ifindices: its extract
kernel timed alternately with hfv_extract_records_timed on the same frames (medians and their
ratio), the frames it passes, and per frame its pass bit against the verdict hfv_br_process gives
in the same run, over the frames decided by the MAC (the router's verdict is SCION_FORWARD or
INVALID_HF, and a frame from the internal link has an AS-egress IFID with a fwd_external egress
entry).  Every other field is what a run without --rx reports; the default --out becomes
profiles/frames/frames_rx_probe.json.

--fused adds, per slot under "fused", hfv_verify_frames_fused (frames to verdict bits in one launch)
with the mix's ifindex array and BR 1's internal ifindices, against the three-launch
hfv_verify_frames_rx on the same frames in the same run: the fused kernel's dispatch time
(hfv_verify_frames_fused_timed), then, interleaved rep by rep, the stream-event region around the
plain fused call, the region around hfv_verify_frames_rx, and hfv_br_process_timed (the router over
a copy of the frames runs ahead of either region, so both find the frame buffer in the same state),
and each region back to back with itself; medians and the whole range of each, whether the fused
range lies below the three-launch range, and whether the two bitmaps are equal.  The default --out becomes profiles/frames/frames_fused_probe.json.

--list adds, per slot under "list", hfv_verify_frames_batches over the frames cut into K chunks of c
frames (c = 16384, K = 64 and c = 32768, K = 32 at the default --n) against K hfv_verify_frames_fused
calls over the same chunks and against one fused call over all frames: interleaved rep by rep, the
stream-event region around one list call, the region around the K calls, the list's dispatch time
(hfv_verify_frames_batches_timed) and the one call's (hfv_verify_frames_fused_timed); medians and the
whole range of each, whether the list region's range lies below the K-call region's, the list's
dispatch median over the one call's, and whether the bitmaps of the two ways are equal.  The default
--out becomes profiles/frames/frames_list_probe.json.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scion-xdp-br_amd"))

import numpy as np  # noqa: E402


def field_lines(frame, base):
    """Number of 64-byte lines that hold the bytes the parser and the copy read of `frame`
    placed at byte address `base`."""
    import scion_hfv as hfv
    st, inf, hf = hfv.frame_locate(frame)
    assert st == 0
    ip = 14
    v4 = frame[12:14] == b"\x08\x00"
    sc = ip + (4 * (frame[ip] & 0x0F) if v4 else 40) + 8
    from scion_hfv import packets
    meta = sc + 28 + packets.ref_host_addr_len(frame[sc + 9])
    spans = [(12, 2), (ip, 1), (ip + (9 if v4 else 6), 1), (sc, 1), (sc + 8, 2), (meta, 4), (inf, 8), (hf, 12)]
    lines = set()
    for off, size in spans:
        lines.update(range((base + off) // 64, (base + off + size - 1) // 64 + 1))
    return len(lines)


def med(xs):
    return float(statistics.median(xs))


def region_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def rx_leg(torch, hfv, ctx, cfg, internal_ifx, frames, tid, ifx, master, slot, d_len, d_if, n, recs, status, bits, ver,
           warmup, reps):
    """The direction-aware path on the frames of one slot size; `ver` holds hfv_br_process's
    verdicts of this run on the same frames (None: no comparison)."""
    ctx.set_internal_ifindices(internal_ifx)
    r = {"internal_ifindices": internal_ifx, "frames_from_internal": int(np.isin(ifx, internal_ifx).sum())}
    plain = lambda: ctx.extract_records_timed(master, slot, d_len, n, recs, status)   # noqa: E731
    aware = lambda: ctx.extract_records_rx_timed(master, slot, d_len, d_if, n, recs, status)   # noqa: E731
    for _ in range(warmup):
        plain()
        aware()
    a, b = [], []
    for _ in range(reps):                                # alternating: both see the same machine
        a.append(plain())
        b.append(aware())
    r["extract_ms"] = round(med(a), 5)
    r["extract_ms_min_max"] = [round(min(a), 5), round(max(a), 5)]
    r["extract_rx_ms"] = round(med(b), 5)
    r["extract_rx_ms_min_max"] = [round(min(b), 5), round(max(b), 5)]
    r["extract_rx_over_extract"] = round(med(b) / med(a), 4)
    if ver is None:
        return r
    ctx.verify_frames_rx(master, slot, d_len, d_if, n, recs, status, bits)
    torch.cuda.synchronize()
    got = hfv.bits_to_bool(bits.cpu().numpy().view(np.uint64), n)
    r["frames_passed"] = int(got.sum())
    # the frames decided by the MAC, by the router kernel's verdicts; the fields of each template
    # frame by the host parser
    fields = [hfv.frame_extract(f[:slot], False) for f in frames]
    cons = np.array([st == 0 and bool(i[0] & 1) for st, i, h in fields])
    egr = np.array([0 if st else int.from_bytes(h[4:6] if i[0] & 1 else h[2:4], "big") for st, i, h in fields])
    ext_ifid = [int(cfg.egress[i].ifid) for i in range(cfg.n_egress) if cfg.egress[i].fwd_external]
    v = ver.cpu().numpy()
    decided = np.isin(v, [hfv.VERDICT["SCION_FORWARD"], hfv.VERDICT["INVALID_HF"]])
    internal = np.isin(ifx, internal_ifx)
    sel = decided & (~internal | np.isin(egr[tid], ext_ifid))
    fwd = v == hfv.VERDICT["SCION_FORWARD"]
    r["mac_decided"] = int(sel.sum())
    r["mac_decided_internal"] = int((sel & internal).sum())
    r["mac_decided_internal_noncons"] = int((sel & internal & ~cons[tid]).sum())
    r["mac_decided_invalid_hf"] = int((sel & ~fwd).sum())
    r["agree_with_router"] = int((got[sel] == fwd[sel]).sum())
    r["agree_with_router_internal"] = int((got[sel & internal] == fwd[sel & internal]).sum())
    r["router_forward_not_passed"] = int((fwd & ~got).sum())     # over all frames, for the record
    # the direction-blind call on the same frames, against the same verdicts
    ctx.verify_frames(master, slot, d_len, n, recs, status, bits)
    torch.cuda.synchronize()
    blind = hfv.bits_to_bool(bits.cpu().numpy().view(np.uint64), n)
    r["verify_frames_passed"] = int(blind.sum())
    r["verify_frames_agree_with_router"] = int((blind[sel] == fwd[sel]).sum())
    return r


def fused_leg(torch, ctx, internal_ifx, master, slot, d_len, d_if, n, recs, status, bits, act, ver, egr, warmup, reps):
    """The one-launch path against the three-launch path and the router, interleaved."""
    ctx.set_internal_ifindices(internal_ifx)
    fbits = torch.empty_like(bits)
    work = torch.empty_like(master)
    fused = lambda: ctx.verify_frames_fused(master, slot, d_len, n, fbits, ingress_ifindex=d_if)   # noqa: E731
    three = lambda: ctx.verify_frames_rx(master, slot, d_len, d_if, n, recs, status, bits)   # noqa: E731

    def router():
        work.copy_(master)
        return ctx.br_process_timed(work, slot, d_len, d_if, n, act, ver, egr)

    for _ in range(warmup):
        ctx.verify_frames_fused_timed(master, slot, d_len, n, fbits, ingress_ifindex=d_if)
        fused()
        three()
        router()
    torch.cuda.synchronize()
    disp = [ctx.verify_frames_fused_timed(master, slot, d_len, n, fbits, ingress_ifindex=d_if) for _ in range(reps)]
    # interleaved, every timed region behind the same predecessor (the router over a copy of the frames:
    # 2 x frame_bytes of other traffic), so neither path finds the frames left warm by the other
    f, t, b = [], [], []
    for _ in range(reps):
        b.append(router())
        f += region_ms(torch, fused, 1)
        router()
        t += region_ms(torch, three, 1)
    # and each path back to back with itself, as verify_frames_region_ms above is taken
    fw, tw = region_ms(torch, fused, reps), region_ms(torch, three, reps)
    r = {"internal_ifindices": internal_ifx}
    for name, xs in (("fused_dispatch_ms", disp), ("fused_region_ms", f), ("three_launch_region_ms", t),
                     ("fused_region_back_to_back_ms", fw), ("three_launch_region_back_to_back_ms", tw),
                     ("br_process_ms", b)):
        r[name] = round(med(xs), 5)
        r[name + "_min_max"] = [round(min(xs), 5), round(max(xs), 5)]
    r["fused_over_three_launch"] = round(med(f) / med(t), 4)
    r["fused_over_router"] = round(med(f) / med(b), 4)
    r["fused_range_below_three_launch_range"] = bool(max(f) < min(t))
    r["fused_range_below_three_launch_range_back_to_back"] = bool(max(fw) < min(tw))
    fused()
    three()
    torch.cuda.synchronize()
    r["bitmaps_equal"] = bool(torch.equal(fbits, bits))
    r["frames_passed"] = int(np.unpackbits(fbits.cpu().numpy().view(np.uint8)).sum())
    # and with no status buffer against one given: the same launch, n more bytes stored
    st = [ctx.verify_frames_fused_timed(master, slot, d_len, n, fbits, ingress_ifindex=d_if, status=status)
          for _ in range(reps)]
    r["fused_dispatch_with_status_ms"] = round(med(st), 5)
    return r


def list_leg(torch, ctx, internal_ifx, master, slot, d_len, d_if, n, warmup, reps):
    """One list call against one fused call per chunk, and against one fused call over everything."""
    ctx.set_internal_ifindices(internal_ifx)
    words = (n + 63) // 64
    lbits = torch.zeros(words, dtype=torch.int64, device="cuda")
    kbits = torch.zeros(words, dtype=torch.int64, device="cuda")
    obits = torch.zeros(words, dtype=torch.int64, device="cuda")
    out = {"internal_ifindices": internal_ifx, "cases": {}}
    for c in (n // 64, n // 32):
        assert c % 64 == 0 and n % c == 0
        K = n // c
        chunks = [(master[k * c:(k + 1) * c], d_len[k * c:(k + 1) * c], d_if[k * c:(k + 1) * c], k * c // 64)
                  for k in range(K)]
        arr = ctx.frame_batches([(f, slot, ln, c, lbits[w:w + c // 64], ifx) for f, ln, ifx, w in chunks])
        lst = lambda: ctx.verify_frames_batches(arr)   # noqa: E731
        lst_timed = lambda: ctx.verify_frames_batches_timed(arr)   # noqa: E731
        one = lambda: ctx.verify_frames_fused_timed(master, slot, d_len, n, obits, ingress_ifindex=d_if)   # noqa: E731

        def calls():
            for f, ln, ifx, w in chunks:
                ctx.verify_frames_fused(f, slot, ln, c, kbits[w:w + c // 64], ingress_ifindex=ifx)

        for _ in range(warmup):
            lst()
            calls()
            lst_timed()
            one()
        torch.cuda.synchronize()
        a, b, d, e = [], [], [], []
        for _ in range(reps):                              # interleaved: all four see the same machine
            a += region_ms(torch, lst, 1)
            b += region_ms(torch, calls, 1)
            d.append(lst_timed())
            e.append(one())
        torch.cuda.synchronize()
        r = {"chunk_frames": c, "chunks": K, "launches": -(-K // 32)}
        for name, xs in (("list_region_ms", a), ("k_calls_region_ms", b), ("list_dispatch_ms", d),
                         ("one_call_dispatch_ms", e)):
            r[name] = round(med(xs), 5)
            r[name + "_min_max"] = [round(min(xs), 5), round(max(xs), 5)]
        r["list_region_over_k_calls_region"] = round(med(a) / med(b), 4)
        r["list_range_below_k_calls_range"] = bool(max(a) < min(b))
        r["list_dispatch_over_one_call_dispatch"] = round(med(d) / med(e), 4)
        r["list_dispatch_within_1p10_of_one_call"] = bool(med(d) <= 1.10 * med(e))
        r["bitmaps_equal"] = bool(torch.equal(lbits, kbits) and torch.equal(lbits, obits))
        r["frames_passed"] = int(np.unpackbits(lbits.cpu().numpy().view(np.uint8)).sum())
        out["cases"]["%dx%d" % (K, c)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", default="2048,144")
    ap.add_argument("--direct", action="store_true", help="misalign the frame buffer: the direct kernel")
    ap.add_argument("--extract-only", action="store_true", help="A/B runs: the extract kernel alone")
    ap.add_argument("--rx", action="store_true", help="add the direction-aware path (see above)")
    ap.add_argument("--fused", action="store_true", help="add the one-launch path (see above)")
    ap.add_argument("--list", action="store_true", help="add the frame-batch list (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = ("frames_list_probe.json" if args.list else "frames_fused_probe.json" if args.fused
                else "frames_rx_probe.json" if args.rx else "frames_probe.json")
        args.out = os.path.join(ROOT, "profiles", "frames", name)
    args.extract_only |= args.direct   # the other legs want the aligned buffer
    import torch
    import bench
    import scion_hfv as hfv
    from scion_hfv import topology as TP

    n, reps = args.n, max(10, args.reps)
    frames, ifis, _, _ = bench.br_templates()
    tmpl, tid, lens, ifx, n_good = bench.br_batch(n, 0)
    ctx = hfv.Ctx(0)
    ctx.key_add(0, TP.KEYS[1])
    cfg = TP.br_config("br1")
    ctx.br_set_config(cfg)
    ctx.set_record_layout(0, 8)
    internal_ifx = [int(cfg.int_ifaces[i].ifindex) for i in range(cfg.n_int_ifaces)]
    stride = hfv.FRAME_REC_STRIDE
    d_tid = torch.from_numpy(tid.astype(np.int64)).cuda()
    d_if = torch.from_numpy(ifx.view(np.int32)).cuda()
    recs = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    act = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ver = torch.zeros_like(act)
    egr = torch.zeros(n, dtype=torch.int32, device="cuda")
    result = {"n": n, "reps": reps, "kernel": "direct" if args.direct else "staged", "hbm_peak_GBs": bench.HBM_PEAK_GBS,
              "device": torch.cuda.get_device_name(0), "slots": {}}
    for slot in [int(s) for s in args.slots.split(",")]:
        assert 64 <= slot <= bench.BR_SLOT and slot % 8 == 0
        buf = torch.empty(n * slot + 16, dtype=torch.uint8, device="cuda")
        off = (-buf.data_ptr()) % 16 + (8 if args.direct else 0)
        master = buf[off:off + n * slot].view(n, slot)
        torch.index_select(torch.from_numpy(np.ascontiguousarray(tmpl[:, :slot])).cuda(), 0, d_tid, out=master)
        assert master.data_ptr() % 16 == (8 if args.direct else 0)
        d_len = torch.from_numpy(np.minimum(lens, slot).astype(np.uint16).view(np.int16)).cuda()
        # algorithmic bytes: per template and placement phase (the ring's frames start at i * slot)
        phases = 64 // np.gcd(slot, 64)
        lines = np.array([[field_lines(f, p * slot) for p in range(phases)] for f in frames])
        alg = float((lines[tid, np.arange(n) % phases] * 64).mean()) + stride + 3
        r = {"slot": slot, "frame_bytes": int(master.numel()), "algorithmic_bytes_per_frame": round(alg, 2)}

        def extract():
            return ctx.extract_records_timed(master, slot, d_len, n, recs, status)

        for _ in range(args.warmup):
            extract()
        ex = [extract() for _ in range(reps)]
        r["status_nonzero"] = int((status != 0).sum())   # 0: every benched frame parses
        r["extract_ms"] = round(med(ex), 5)
        r["extract_ms_min_max"] = [round(min(ex), 5), round(max(ex), 5)]
        r["extract_GBs"] = round(alg * n / (med(ex) * 1e-3) / 1e9, 1)
        r["extract_frac_of_peak"] = round(r["extract_GBs"] / bench.HBM_PEAK_GBS, 4)
        r["extract_Gpkts"] = round(n / (med(ex) * 1e-3) / 1e9, 2)
        if not args.extract_only:
            sr = [ctx.stream_read_ms([master]) for _ in range(reps)]
            r["stream_read_ms"] = round(med(sr), 5)
            r["stream_read_GBs"] = round(master.numel() / (med(sr) * 1e-3) / 1e9, 1)
            # the extract's line traffic (whole 128-byte lines of the first 128 bytes of a slot, or
            # the whole dense ring) against the streaming rate of the same run
            touched = min(slot, 128) * n + (stride + 3) * n
            r["extract_line_GBs"] = round(touched / (med(ex) * 1e-3) / 1e9, 1)
            r["extract_line_frac_of_stream_read"] = round(r["extract_line_GBs"] / r["stream_read_GBs"], 4)
            batch = [(recs, n, bits, stride)]
            for _ in range(args.warmup):
                ctx.verify_batches_timed(batch)
            vb = [ctx.verify_batches_timed(batch) for _ in range(reps)]
            r["verify_batches_ms"] = round(med(vb), 5)
            vf = lambda: ctx.verify_frames(master, slot, d_len, n, recs, status, bits)   # noqa: E731

            def two():
                ctx.extract_records(master, slot, d_len, n, recs, status)
                ctx.verify_batches(batch)

            for _ in range(args.warmup):
                vf()
                two()
            torch.cuda.synchronize()
            r["verify_frames_region_ms"] = round(med(region_ms(torch, vf, reps)), 5)
            r["extract_verify_region_ms"] = round(med(region_ms(torch, two, reps)), 5)
            r["mask_ms_by_difference"] = round(r["verify_frames_region_ms"] - r["extract_verify_region_ms"], 5)
            # the mask kernel alone (idempotent: the bitmap stays what verify_frames left), between
            # events: one launch (what the event pair itself costs is in it), and 20 back to back
            mask = lambda: ctx.mask_status(status, n, bits)   # noqa: E731

            def mask20():
                for _ in range(20):
                    mask()

            for _ in range(args.warmup):
                mask20()
            torch.cuda.synchronize()
            r["mask_ms"] = round(med(region_ms(torch, mask, reps)), 5)
            r["mask_ms_per_launch_of_20"] = round(med(region_ms(torch, mask20, reps)) / 20, 5)
            passed = int(np.unpackbits(bits.cpu().numpy().view(np.uint8)).sum())
            r["frames_passed"] = passed
            work = torch.empty_like(master)
            br = []
            for k in range(args.warmup + reps):
                work.copy_(master)
                t = ctx.br_process_timed(work, slot, d_len, d_if, n, act, ver, egr)
                if k >= args.warmup:
                    br.append(t)
            r["br_process_ms"] = round(med(br), 5)
            r["router_forwarded"] = int((act == 4).sum())
            r["n_good"] = n_good
            kernels = r["extract_ms"] + r["verify_batches_ms"] + r["mask_ms"]
            r["frames_path_kernels_ms"] = round(kernels, 5)
            r["frames_path_over_router"] = round(kernels / r["br_process_ms"], 4)
            r["region_over_router"] = round(r["verify_frames_region_ms"] / r["br_process_ms"], 4)
            del work
        if args.rx:
            r["rx"] = rx_leg(torch, hfv, ctx, cfg, internal_ifx, frames, tid, ifx, master, slot, d_len, d_if, n, recs,
                             status, bits, None if args.extract_only else ver, args.warmup, reps)
        if args.fused:
            r["fused"] = fused_leg(torch, ctx, internal_ifx, master, slot, d_len, d_if, n, recs, status, bits, act, ver,
                                   egr, args.warmup, reps)
        if args.list:
            r["list"] = list_leg(torch, ctx, internal_ifx, master, slot, d_len, d_if, n, args.warmup, reps)
        result["slots"][str(slot)] = r
        del master, buf
    ctx.close()
    line = json.dumps(result)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
