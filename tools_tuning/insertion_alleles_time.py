"""The insertion-allele stage of a record build (docs/SPEC.md §17) at 100 000 reads x 3000 columns with qualities, by HIP events
(torch) on the window's stream.  The records come from `juliet-synth --raw-out --rich-qv --ins-ppm`: insertions of 1-4 bases with
poor qualities before 300 of a million cells, some 90 000 'I' ops.  (The raw generator takes no --insert plant: the alleles of this
window are the three-base noise insertions, readable at min_qv 0 and unread at min_qv 20.)
Three builds of the same records into the same window, each between its own pair of events, the switches being the only difference:
  plain                 no tracking
  + section 11 counters jl_msa_track_insertions: the existing traversal of the same cigars (insertions_kernel), the yardstick
  + alleles             jl_msa_track_insertion_alleles: the record walk, the span pass, three memsets
so (row - plain) is what a switch adds to a build.  Beside the span pass, as its yardstick, jl_codon_deletions_async on the window
just built: the existing whole-plane popcount pass.  The kernels by themselves: run this script under
`rocprofv3 --kernel-trace --stats` (insertion_alleles_kernel, junction_span_kernel, insertions_kernel, codon_deletions_kernel).
Reported: median, minimum and the spread (max - min of the medians of five blocks of reps).  Nothing is asserted: no time is promised.
usage: insertion_alleles_time.py [reps] [min_qv]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
min_qv = int(sys.argv[2]) if len(sys.argv) > 2 else 20
L, N = 3000, 100_000
stream = torch.cuda.Stream()

rec = synth.raw_records(41, N, L, extra=("--rich-qv", "--ins-ppm", "300"))
n_ins = int(((rec["cigar"] & 15) == 1).sum())
src = capi.Juliet(0, stream=stream.cuda_stream)
src.records_upload(rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"])
win = capi.Juliet(0, stream=stream.cuda_stream)


def timed(fn, n):
    pairs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        pairs.append((e0, e1))
    stream.synchronize()
    return np.array([1e3 * a.elapsed_time(b) for a, b in pairs])


def report(name, fn):
    fn()
    win.sync()                                        # warm-up: code objects, the buffers
    blocks = [timed(fn, reps) for _ in range(5)]
    meds = [float(np.median(b)) for b in blocks]
    us = np.concatenate(blocks)
    print(f"{name}: median {np.median(us):.1f} us, min {us.min():.1f} us, block medians {min(meds):.1f} .. {max(meds):.1f} (spread {max(meds) - min(meds):.1f})", flush=True)
    return float(np.median(us))


def build(counters, alleles):
    win.track_insertions(counters)
    win.track_insertion_alleles(alleles)
    return lambda: win.records_window(src, L, 0, min_qv, wait=False)


print(f"{N} reads x {L} columns, {len(rec['cigar'])} cigar words, {n_ins} 'I' ops, min_qv {min_qv}", flush=True)
plain = report("build, plain              ", build(False, False))
old = report("build + section 11 counters", build(True, False))
new = report("build + alleles            ", build(False, True))
jcnt, rows = win.insertion_alleles()
print(f"  the switches add: section 11 counters {old - plain:.1f} us, alleles {new - plain:.1f} us; table {len(rows)} rows, "
      f"inframe {int(jcnt[:, 1].sum())}, frameshift {int(jcnt[:, 2].sum())}, unread {int(jcnt[:, 3].sum())}, span.max {int(jcnt[:, 0].max())}", flush=True)
report("codon deletions (whole call)", lambda: win.codon_deletions(wait=False))
for x in (win, src):
    x.sync()
    x.close()
