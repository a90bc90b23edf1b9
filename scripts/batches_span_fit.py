#!/usr/bin/env python3
"""Per-block entry/finish stamps of a hfv_verify_batches launch, regressed on the block's first batch.
K = 20 and K = 64 batches of 2^20 rotated resident records, medians over `reps` timed calls; the per-XCD
(block % 8) mean is taken out of each series before the fit.  Diagnostic, not used by tests or the bench.
    python scripts/batches_span_fit.py OUT.json [reps]   (HFV_LIB selects the build)"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scion-xdp-br_amd"))
sys.path.insert(0, ROOT)
import scion_hfv as hfv  # noqa: E402
import bench  # noqa: E402


def fit(x, y):
    x, y = np.asarray(x, float), np.asarray(y, float)
    if np.ptp(x) == 0:
        return 0.0, float(y.mean()), 0.0
    a, b = np.polyfit(x, y, 1)
    r = np.corrcoef(x, y)[0, 1]
    return float(a), float(b), float(r)


def main():
    out = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    n, R = 1 << 20, 8
    ctx = hfv.Ctx(0)
    ctx.key_add(0, bench.KEY_1111)
    recs = [torch.empty((n, 64), dtype=torch.uint8, device="cuda") for _ in range(R)]
    for i in range(R):
        ctx.gen_records(recs[i], n, bench.SEED_RECORDS, first_index=i * n)
    res = {"lib": os.environ.get("HFV_LIB", "default")}
    for K in (20, 64):
        bits = [torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda") for _ in range(K)]
        blist = ctx.service_batches([(recs[k % R], n, bits[k]) for k in range(K)])
        T = K * (n // 64)
        G = min(256, T)
        first = [(T * k // G) // (n // 64) for k in range(G)]
        for _ in range(3):
            ctx.verify_batches_timed(blist)
        ent, fin, ms = [], [], []
        for _ in range(reps):
            ms.append(ctx.verify_batches_timed(blist) * 1e3)
            span = ctx.batches_block_span(G)
            ent.append([a for a, _ in span])
            fin.append([b for _, b in span])
        ent = np.median(np.array(ent), axis=0)
        fin = np.median(np.array(fin), axis=0)
        dur = fin - ent
        # take the per-XCD (block % 8) mean out before regressing on the first batch
        def dex(v):
            v = v.copy()
            for x in range(8):
                v[x::8] -= v[x::8].mean()
            return v
        r = {"K": K, "kernel_us": [round(m, 2) for m in ms], "kernel_us_median": round(statistics.median(ms), 2),
             "entry_spread_us": round(float(ent.max() - ent.min()), 2),
             "finish_min_med_max_us": [round(float(fin.min()), 2), round(float(np.median(fin)), 2), round(float(fin.max()), 2)],
             "fit_finish_on_first_batch": [round(v, 4) for v in fit(first, dex(fin))],
             "fit_duration_on_first_batch": [round(v, 4) for v in fit(first, dex(dur))],
             "fit_entry_on_first_batch": [round(v, 4) for v in fit(first, dex(ent))],
             "first_batch": first, "entry_us": [round(float(v), 2) for v in ent],
             "finish_us": [round(float(v), 2) for v in fin]}
        print(f"K {K}: kernel median {r['kernel_us_median']} us; finish min/med/max {r['finish_min_med_max_us']}; "
              f"slope finish/batch {r['fit_finish_on_first_batch']} dur/batch {r['fit_duration_on_first_batch']} "
              f"entry/batch {r['fit_entry_on_first_batch']} (us per batch, intercept, r)", flush=True)
        res[f"K{K}"] = r
        torch.cuda.synchronize()
        for k in range(K):
            assert torch.equal(bits[k], torch.from_numpy(bench.truth_bitmap(n, (k % R) * n)).cuda())
    ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=0)


if __name__ == "__main__":
    main()
