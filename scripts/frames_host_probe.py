#!/usr/bin/env python3
"""hfv_verify_frames_host over the bench's frame mix in host memory: 2^20 frames in 2 KiB slots
through the call at window 128 and 256, pageable (packed windows up, two bits per frame back) and
zero-copy (the ring registered, the kernel reads it in place), beside hfv_br_process_host on the same
frames and the PCIe probe (scripts/pcie_probe.py) in the same run.  Per leg: Mpkt/s (median and range
of the repetitions), bytes over PCIe per frame (computed from what the path copies: window + len +
ifindex up and 16 bytes per 64 frames back, plus a whole slot for each frame run again; the router
also copies each window back with 6 result bytes; zero-copy: the 128-byte staged row the kernel
loads from the ring, at least, with len and ifindex copied up and the bitmap back) and the share of
frames run again.  Prints one JSON line at the end.
python scripts/frames_host_probe.py [--n N] [--reps R]   (1 GPU; HFV_LIB selects the build)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scion-xdp-br_amd"), ROOT, os.path.join(ROOT, "scripts")]
import scion_hfv as hfv  # noqa: E402
import bench  # noqa: E402
import pcie_probe  # noqa: E402
from scion_hfv import topology as TP  # noqa: E402

SLOT = 2048


def timed(fn, reps, before=None):
    ts = []
    for r in range(reps + 1):                                 # the first pass allocates the staging
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        if r:
            ts.append(time.perf_counter() - t0)
    return ts, out


def leg(name, n, ts, up, down, retried=0):
    r = {"leg": name, "mpkts": round(n / np.median(ts) / 1e6, 1), "mpkts_min": round(n / max(ts) / 1e6, 1),
         "mpkts_max": round(n / min(ts) / 1e6, 1), "pcie_bytes_per_frame": round(up + down, 2),
         "retried_share": round(retried / n, 4), "reps": len(ts)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n = a.n
    pcie_probe.main()
    ctx = hfv.Ctx(0)
    cfg = TP.br_config("br1")
    ctx.key_add(0, TP.KEYS[1])
    ctx.br_set_config(cfg)
    ctx.set_internal_ifindices([int(cfg.int_ifaces[i].ifindex) for i in range(cfg.n_int_ifaces)])
    tmpl, tid, lens, ifidx, _ = bench.br_batch(n, 0)
    ring = hfv.host_array((n, SLOT), np.uint8)                # page-aligned: registered for the zero-copy legs
    heads = np.ascontiguousarray(tmpl[:, :256])

    def fill():
        ring[:, :256] = heads[tid]

    fill()
    words = (n + 63) // 64
    bits = np.zeros(words, np.uint64)
    legs, ref = [], None
    for window in (128, 256):
        ts, retried = timed(lambda: ctx.verify_frames_host(ring, SLOT, lens, n, bits, ingress_ifindex=ifidx, window=window),
                            a.reps)
        ref = bits.copy() if ref is None else ref
        assert np.array_equal(bits, ref), "the verdicts depend on the window"
        legs.append(leg("pageable window %d" % window, n, ts, window + 6 + retried * (SLOT + 6) / n,
                        16 / 64 + retried * 16 / 64 / n, retried))
    act, ver, egr = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    for window in (128, 256):
        ts, _ = timed(lambda: ctx.br_process_host(ring, SLOT, lens, ifidx, n, act, ver, egr, window=window), a.reps,
                      before=fill)                            # the router rewrites the frames: put them back
        legs.append(leg("hfv_br_process_host window %d" % window, n, ts, window + 6, window + 6))
    fill()
    ctx.host_register(ring)
    try:
        for window in (128, 256):                             # the zero-copy path takes no window: same launch
            ts, retried = timed(lambda: ctx.verify_frames_host(ring, SLOT, lens, n, bits, ingress_ifindex=ifidx,
                                                               window=window), a.reps)
            assert np.array_equal(bits, ref) and retried == 0, "zero-copy verdicts differ"
            legs.append(leg("zero-copy (window %d given)" % window, n, ts, 128 + 6, 8 / 64))
    finally:
        ctx.host_unregister(ring)
    passed = int(np.unpackbits(ref.view(np.uint8)).sum())
    print(json.dumps({"probe": "frames_host", "n": n, "slot": SLOT, "pass": passed, "legs": legs}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
