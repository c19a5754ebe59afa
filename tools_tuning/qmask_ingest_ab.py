"""The record ingest with the QV filter as quality bytes (jl_records_append) against the filter as one bit per base
(jl_records_append_masked), on the same records, the same binary, in one process: `ccs --richQVs`-shaped synthetic records
(juliet-synth --raw-out --rich-qv), both forms uploaded (two copies each, taken in turns), the window built alternately —
bytes, mask, bytes, mask — each build between two device events on the window's stream.  Per form: median, minimum and spread
of the build time, with the bytes the form moves (its records + the planes written) and their share of the HBM peak.  The two
matrices are compared once at the end.
usage: qmask_ingest_ab.py [reads] [cols] [pairs] [min_qv] [out.txt]   (100000 3000 40 20)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

HBM_PEAK_GBS = 8000.0
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
l = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 40
min_qv = int(sys.argv[4]) if len(sys.argv) > 4 else 20
out_path = sys.argv[5] if len(sys.argv) > 5 else None
WARM, K = 6, 2

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


rec = synth.raw_records(2, n, l, extra=("--rich-qv",))
five = [rec[k] for k in ("pos", "cigar", "cig_off", "seq4", "seq_off")]
mask = capi.qmask_from_quals(rec["seq_off"], rec["qual"], rec["qual_off"], min_qv)
shared = sum(a.nbytes for a in five)
rec_bytes = {"bytes": shared + rec["qual"].nbytes + rec["qual_off"].nbytes, "mask": shared + mask.nbytes}
say(f"{n} reads x {l} columns, min_qv {min_qv}, {len(rec['cigar']) / n:.1f} ops per read, library {os.environ.get('JL_LIB', 'as built')}")

stream = torch.cuda.Stream()
recs = {"bytes": [], "mask": []}
for k in range(K):
    c = capi.Juliet(0)
    c.records_upload(*five, rec["qual"], rec["qual_off"])
    recs["bytes"].append(c)
    c = capi.Juliet(0)
    c.records_upload(*five, qmask=mask)
    recs["mask"].append(c)
wins = {f: capi.Juliet(0, stream=stream.cuda_stream) for f in recs}
plane_bytes = None
times = {f: [] for f in recs}
for p in range(WARM + pairs):
    for f in ("bytes", "mask"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
        wins[f].records_window(recs[f][p % K], l, 0, min_qv, wait=False)      # jl_records_window_async
        with torch.cuda.stream(stream):
            e1.record()
        e1.synchronize()
        if p >= WARM:
            times[f].append(1e3 * e0.elapsed_time(e1))
plane_bytes = 3 * l * wins["bytes"].plane_stride

stats = {}
for f in ("bytes", "mask"):
    t = np.array(times[f])
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    moved = rec_bytes[f] + plane_bytes
    stats[f] = (med, t.min(), t.max(), q3 - q1)
    say(f"{f:5s}: median {med:7.1f} us  min {t.min():7.1f}  max {t.max():7.1f}  spread max-min {t.max() - t.min():6.1f}  interquartile {q3 - q1:5.1f}"
        f"  | {moved / 1e6:6.1f} MB (records {rec_bytes[f] / 1e6:.1f} + planes {plane_bytes / 1e6:.1f}), frac of the HBM peak at the median "
        f"{moved / (med * 1e-6) / 1e9 / HBM_PEAK_GBS:.3f}  ({len(t)} builds)")
gain = stats["bytes"][0] - stats["mask"][0]
say(f"mask - bytes at the median: {-gain:+.1f} us; the byte form's own spread: interquartile {stats['bytes'][3]:.1f} us, max-min {stats['bytes'][2] - stats['bytes'][1]:.1f} us"
    f" -> the mask form {'clears' if gain > stats['bytes'][2] - stats['bytes'][1] else 'clears the interquartile bar only' if gain > stats['bytes'][3] else 'does NOT clear'} the bar")
same = (wins["bytes"].download_columns() == wins["mask"].download_columns()).all()
say(f"the two matrices are {'equal' if same else 'DIFFERENT'} ({n} x {l} cells)")
for cs in list(wins.values()) + recs["bytes"] + recs["mask"]:
    cs.close()
if out_path:
    with open(out_path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
sys.exit(0 if same else 1)
