#!/usr/bin/env python3
"""Summarise the rocprofv3 traces of one build's batch-list regions: the k_verify_batches durations and
the gaps between the launches of a call from the kernel traces, and the host timeline around every
hipExtLaunchKernel (launch, event record, closing synchronize) from the HIP traces.  SRC holds, for k in
20 and 200 (the bench's --steps), kt<k>/kt<k>_kernel_trace.csv (rocprofv3 --kernel-trace --stats -d
SRC/kt<k> -o kt<k> --output-format csv -- python bench.py ...) and hip<k>/hip<k>_hip_api_trace.csv (the same
with --hip-trace alone).  Prints the summary and writes the filtered rows, small enough to keep, to OUTDIR
as TAG_*.csv (profiles/first_map/).   python scripts/region_account.py SRC TAG OUTDIR"""
import csv
import os
import statistics as st
import sys

src, tag, outdir = sys.argv[1], sys.argv[2], sys.argv[3]
os.makedirs(outdir, exist_ok=True)


def med(v):
    return st.median(v) if v else float("nan")


for k in ("20", "200"):
    # ---- kernel trace
    rows = list(csv.DictReader(open(f"{src}/kt{k}/kt{k}_kernel_trace.csv")))
    kb = [r for r in rows if "k_verify_batches" in r["Kernel_Name"]]
    with open(f"{outdir}/{tag}_kt{k}_k_verify_batches.csv", "w") as f:
        w = csv.writer(f)
        w.writerow(["Dispatch_Id", "Queue_Id", "Stream_Id", "Start_Timestamp", "End_Timestamp", "dur_ns", "gap_to_prev_end_ns", "Grid_Size_X"])
        prev = None
        for r in kb:
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            w.writerow([r["Dispatch_Id"], r["Queue_Id"], r["Stream_Id"], s, e, e - s, (s - prev) if prev else "", r["Grid_Size_X"]])
            prev = e
    durs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in kb]
    print(f"[{tag} K={k}] k_verify_batches launches {len(kb)}; durations us: " + " ".join(f"{d / 1e3:.1f}" for d in durs[:40]))
    if k == "200":
        # a call = 4 launches (64, 64, 64, 8 batches); gaps between them
        gaps = []
        for a, b in zip(kb[:-1], kb[1:]):
            g = int(b["Start_Timestamp"]) - int(a["End_Timestamp"])
            if g < 200000:
                gaps.append(g)
        print(f"[{tag} K=200] gaps between consecutive launches < 200 us: n {len(gaps)} median {med(gaps) / 1e3:.2f} us "
              f"min {min(gaps) / 1e3:.2f} max {max(gaps) / 1e3:.2f}")
    for f in (f"kt{k}_kernel_stats.csv", f"kt{k}_domain_stats.csv"):
        open(f"{outdir}/{tag}_{f}", "w").write(open(f"{src}/kt{k}/{f}").read())
    # ---- HIP trace: the thread that launches, rows around every hipExtLaunchKernel*
    rows = list(csv.DictReader(open(f"{src}/hip{k}/hip{k}_hip_api_trace.csv")))
    rows = [r for r in rows if not r["Function"].startswith("__hip")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if r["Function"].startswith("hipExtLaunchKernel") or r["Function"] == "hipExtModuleLaunchKernel"]
    names = sorted({rows[i]["Function"] for i in idx})
    keep = set()
    for i in idx:
        keep.update(range(max(0, i - 3), min(len(rows), i + 8)))
    with open(f"{outdir}/{tag}_hip{k}_around_ext_launches.csv", "w") as f:
        w = csv.writer(f)
        w.writerow(["Function", "Thread_Id", "Start_Timestamp", "End_Timestamp", "dur_ns"])
        for i in sorted(keep):
            r = rows[i]
            w.writerow([r["Function"], r["Thread_Id"], r["Start_Timestamp"], r["End_Timestamp"],
                        int(r["End_Timestamp"]) - int(r["Start_Timestamp"])])
    launch = [int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"]) for i in idx]
    # the event record that follows a launch on the same thread before the next launch / sync
    rec, sync, l2s = [], [], []
    for n, i in enumerate(idx):
        t = rows[i]["Thread_Id"]
        for j in range(i + 1, min(len(rows), i + 12)):
            r = rows[j]
            if r["Thread_Id"] != t:
                continue
            fn = r["Function"]
            if fn.startswith("hipExtLaunchKernel"):
                break
            if fn == "hipEventRecord":
                rec.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
            if fn in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize"):
                sync.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                l2s.append(int(r["End_Timestamp"]) - int(rows[i]["Start_Timestamp"]))
                break
    print(f"[{tag} K={k}] {names}: n {len(idx)} host us median {med(launch) / 1e3:.2f} (min {min(launch) / 1e3:.2f}); "
          f"hipEventRecord behind a launch: n {len(rec)} median {med(rec) / 1e3:.2f} us; "
          f"following synchronize: n {len(sync)} median {med(sync) / 1e3:.1f} us; last launch entry -> sync return median {med(l2s) / 1e3:.1f} us")
