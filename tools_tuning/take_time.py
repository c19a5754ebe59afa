"""jl_msa_take_async on the device at the two shapes DESIGN.md quotes, by HIP events (torch) on the destination's stream:
  downsample  100 000 -> 6000 reads x 3000 columns
  mixture     98 000 + 1000 + 1000 -> 100 000 reads x 3000 columns
and, in the same process, the route to the same 6000-read window without it: the selected records (already decoded, on the host)
through ingest_records — upload included, host clock around the blocking call — and that route's device ingest alone
(records resident, jl_records_window_async between events).
Every timed call sits between its own pair of events (a take = the upload of its indices + one launch); sources and destinations
rotate so that no launch finds its input in the Infinity Cache (4 x 112.5 MB > 256 MiB).  Reported: median and minimum of `reps`.
usage: take_time.py [reps]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
L, N = 3000, 100_000
HBM_PEAK = 8.0e12      # bytes/s, the specification's figure

stream = torch.cuda.Stream()


def ctx():
    return capi.Juliet(0, stream=stream.cuda_stream)


def filled(n, seed):
    j = ctx()
    j.alloc(n, L)
    j.synth_fill(synth.SynthParams(seed=seed, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
    return j


def timed(calls):
    """calls: one callable per repetition, each enqueueing on `stream`; microseconds of each between its own events."""
    pairs = []
    for fn in calls:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        pairs.append((e0, e1))
    stream.synchronize()
    return np.array([1e3 * a.elapsed_time(b) for a, b in pairs])


def report(name, us, n_bytes=None):
    line = f"{name}: median {np.median(us):.1f} us, min {us.min():.1f} us over {len(us)}"
    if n_bytes:
        line += f"; {n_bytes / 1e6:.1f} MB moved, {n_bytes / (np.median(us) * 1e-6) / 1e12:.2f} TB/s = {100 * n_bytes / (np.median(us) * 1e-6) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak"
    print(line, flush=True)


plane = lambda n: (n + 1023) // 1024 * 128      # bytes per plane row (jl_plane_stride)  # noqa: E731

# ---- downsample 100 000 -> 6000
srcs = [filled(N, 2 + k) for k in range(4)]
dsts = [ctx(), ctx()]
idx = capi.sample_reads(N, 6000, 0)
for d in dsts:
    for s in srcs[:2]:
        d.take([(s, idx)])       # warm-up: code object, buffers of this shape
us = timed([lambda q=q: dsts[q % 2].take([(srcs[q % 4], idx)], wait=False) for q in range(reps)])
# bytes: the gather touches every 128-byte line of the source rows (one read in sixteen is kept) + the destination's planes
report("take 100000 -> 6000 x 3000", us, 3 * L * (plane(N) + plane(6000)))
take_us = float(np.median(us))

# ---- the same 6000-read window from its records
rec = synth.raw_records(2, N, L)
co, so = rec["cig_off"].astype(np.int64), rec["seq_off"].astype(np.int64)
sel = dict(pos=rec["pos"][idx],
           cigar=np.concatenate([rec["cigar"][co[r]:co[r + 1]] for r in idx]),
           seq4=np.concatenate([rec["seq4"][so[r]:so[r + 1]] for r in idx]))
sel["cig_off"] = np.concatenate([[0], np.cumsum(co[idx + 1] - co[idx])]).astype(np.uint64)
sel["seq_off"] = np.concatenate([[0], np.cumsum(so[idx + 1] - so[idx])]).astype(np.uint64)
w = ctx()
host = []
for q in range(reps // 4 + 3):
    t0 = time.perf_counter()
    w.ingest_records(L, 0, sel["pos"], sel["cigar"], sel["cig_off"], sel["seq4"], sel["seq_off"])
    host.append(1e6 * (time.perf_counter() - t0))
report("ingest_records of the 6000 selected records, upload included (host clock, blocking)", np.array(host[3:]))
recs = [ctx() for _ in range(4)]
for r in recs:
    r.records_upload(sel["pos"], sel["cigar"], sel["cig_off"], sel["seq4"], sel["seq_off"])
wins = [ctx(), ctx()]
for x in wins:
    x.records_window(recs[0], L, 0, 0)
us = timed([lambda q=q: wins[q % 2].records_window(recs[q % 4], L, 0, 0, wait=False) for q in range(reps)])
report("  its device ingest alone (jl_records_window_async, records resident)", us)
ingest_us = float(np.median(us))
print(f"take / device ingest = {take_us / ingest_us:.2f}  (bound: at most 1)", flush=True)
for x in wins + recs + [w]:
    x.sync()
    x.close()

# ---- mixture 98 000 + 1000 + 1000 -> 100 000
minors = [[filled(20_000, 20 + k), filled(20_000, 30 + k)] for k in range(2)]
parts_idx = [capi.sample_reads(N, 98_000, 0), capi.sample_reads(20_000, 1000, 1), capi.sample_reads(20_000, 1000, 2)]
big = [ctx(), ctx()]


def mix(q, wait=False):
    m = minors[q % 2]
    big[q % 2].take([(srcs[q % 4], parts_idx[0]), (m[0], parts_idx[1]), (m[1], parts_idx[2])], wait=wait)


for q in range(4):
    mix(q, wait=True)
us = timed([lambda q=q: mix(q) for q in range(reps)])
report("take 98000 + 1000 + 1000 -> 100000 x 3000", us, 3 * L * (plane(N) + 2 * plane(20_000) + plane(N)))
sys.exit(0 if take_us <= ingest_us else 1)
