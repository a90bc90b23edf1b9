#!/usr/bin/env python3
"""Frames addressed by descriptors, verified in place, against the fused call on a slot copy of the
same frames, one run, one ctx.

Builds bench.py's config-4 batch (2^20 router frames through bench.br_batch) three times as a UMEM:
  inorder    2 KiB chunks, headroom 256: frame i at i * 2048 + 256
  permuted   the same chunks in a random order
  packed     frames back to back, each pushed on by a random 0..15 bytes, so addr & 15 is random
and once as the slot copy (2 KiB slots) hfv_verify_frames_fused takes.  After a warm-up it takes
--reps timed runs of hfv_verify_frames_desc_timed per layout and of hfv_verify_frames_fused_timed on
the slot copy, interleaved rep by rep so that all four see the same machine; medians and the whole
range of each, each layout's median over the fused median, whether the layout's median lies inside
the fused call's own range, whether the bitmaps are equal, and the shader clock right behind the timed loop.  Prints
one JSON object and writes it to --out.

  timeout -k 10 300 python scripts/frames_desc_probe.py [--n N] [--reps R] [--unstaged]

--unstaged places every UMEM one byte off 16-byte alignment: the kernel without staging loads.
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

CHUNK, HEADROOM = 2048, 256


def med(xs):
    return float(statistics.median(xs))


def build_umem(torch, tmpl_dev, d_tid, lens, addr, total, misalign):
    """The frames (template tid[i], lens[i] bytes) at byte offsets addr[i] of a device buffer of
    `total` bytes, written piece by piece so that the byte index stays small."""
    raw = torch.zeros(total + 32, dtype=torch.uint8, device="cuda")
    off = (-raw.data_ptr()) % 16 + misalign
    umem = raw[off:off + total]
    n, step = len(lens), 1 << 15
    d_len = torch.from_numpy(lens.astype(np.int64)).cuda()
    d_addr = torch.from_numpy(addr.astype(np.int64)).cuda()
    flat = tmpl_dev.reshape(-1)
    for lo in range(0, n, step):
        ln, ad, td = d_len[lo:lo + step], d_addr[lo:lo + step], d_tid[lo:lo + step]
        first = torch.cumsum(ln, 0) - ln
        within = torch.arange(int(ln.sum()), device="cuda") - torch.repeat_interleave(first, ln)
        umem[torch.repeat_interleave(ad, ln) + within] = flat[torch.repeat_interleave(td * tmpl_dev.shape[1], ln) + within]
    return raw, umem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--unstaged", action="store_true", help="misalign the UMEM: the kernel without staging loads")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames", "frames_desc_probe.json"))
    args = ap.parse_args()
    import torch
    import bench
    import scion_hfv as hfv
    from scion_hfv import topology as TP

    n, reps = args.n, max(7, args.reps)
    tmpl, tid, lens, ifx, n_good = bench.br_batch(n, 0)
    slot = bench.BR_SLOT
    lens = np.minimum(lens, CHUNK - HEADROOM - 16).astype(np.uint16)   # (br_batch's frames are at most 1500 bytes)
    ctx = hfv.Ctx(0)
    ctx.key_add(0, TP.KEYS[1])
    cfg = TP.br_config("br1")
    ctx.set_internal_ifindices([int(cfg.int_ifaces[i].ifindex) for i in range(cfg.n_int_ifaces)])
    d_tid = torch.from_numpy(tid.astype(np.int64)).cuda()
    tmpl_dev = torch.from_numpy(np.ascontiguousarray(tmpl)).cuda()
    # the slot copy
    master = torch.empty((n, slot), dtype=torch.uint8, device="cuda")
    torch.index_select(tmpl_dev, 0, d_tid, out=master)
    d_len = torch.from_numpy(lens.view(np.int16)).cuda()
    d_if = torch.from_numpy(ifx.view(np.int32)).cuda()
    words = (n + 63) // 64
    fbits = torch.zeros(words, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(0xDE5C)
    layouts = {}
    order = rng.permutation(n)
    pad = rng.integers(0, 16, n)
    packed = np.cumsum(lens.astype(np.int64) + pad) - lens
    for name, addr, total in (("inorder", np.arange(n, dtype=np.int64) * CHUNK + HEADROOM, n * CHUNK),
                              ("permuted", order.astype(np.int64) * CHUNK + HEADROOM, n * CHUNK),
                              ("packed", packed, int(packed[-1] + lens[-1]))):
        raw, umem = build_umem(torch, tmpl_dev, d_tid, lens, addr, total, 1 if args.unstaged else 0)
        desc = np.zeros(n, dtype=hfv.FRAME_DESC_DTYPE)
        desc["addr"], desc["len"], desc["ifindex"] = addr, lens, ifx
        layouts[name] = {"raw": raw, "umem": umem, "bytes": total, "desc": torch.from_numpy(desc.view(np.uint8)).cuda(),
                         "bits": torch.zeros(words, dtype=torch.int64, device="cuda"), "ms": [],
                         "addr_mod16": np.bincount(addr & 15, minlength=16).tolist()}

    def fused():
        return ctx.verify_frames_fused_timed(master, slot, d_len, n, fbits, ingress_ifindex=d_if)

    def by_desc(lay):
        return ctx.verify_frames_desc_timed(lay["umem"], lay["bytes"], lay["desc"], n, lay["bits"])

    for _ in range(args.warmup):
        fused()
        for lay in layouts.values():
            by_desc(lay)
    f = []
    for _ in range(reps):                                    # interleaved: all four see the same machine
        f.append(fused())
        for lay in layouts.values():
            lay["ms"].append(by_desc(lay))
    torch.cuda.synchronize()
    # the shader clock, as block 0 of a record-verify launch over as many records sees it right behind
    # the timed loop (the frame kernels carry no clock stamps of their own)
    recs = torch.zeros((n, hfv.REC_SIZE), dtype=torch.uint8, device="cuda")
    ctx.gen_records(recs, n, 1)
    rbits = torch.zeros(words, dtype=torch.int64, device="cuda")
    ctx.verify_batches_timed([(recs, n, rbits, hfv.REC_SIZE)])
    mhz = ctx.batches_shader_mhz()
    result = {"n": n, "reps": reps, "kernel": "unstaged" if args.unstaged else "staged",
              "device": torch.cuda.get_device_name(0), "shader_mhz_behind_the_loop": mhz and round(mhz, 1),
              "n_good": n_good,
              "frames_passed": int(np.unpackbits(fbits.cpu().numpy().view(np.uint8)).sum()),
              "fused_ms": round(med(f), 5), "fused_ms_min_max": [round(min(f), 5), round(max(f), 5)], "layouts": {}}
    for name, lay in layouts.items():
        ms = lay["ms"]
        result["layouts"][name] = {
            "umem_bytes": lay["bytes"], "addr_mod16": lay["addr_mod16"],
            "desc_ms": round(med(ms), 5), "desc_ms_min_max": [round(min(ms), 5), round(max(ms), 5)],
            "desc_over_fused": round(med(ms) / med(f), 4),
            "desc_median_within_fused_range": bool(min(f) <= med(ms) <= max(f)),
            "bitmaps_equal": bool(torch.equal(lay["bits"], fbits))}
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
