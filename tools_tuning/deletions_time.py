"""jl_codon_deletions_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole
call (zeroing the table + the kernel).  Beside it, as the yardstick, the plain pileup of the same window at the same commit — both
read the matrix once: pileup_async between the same events, and jl_time_pileup's own average over back-to-back launches of one
window.  Every timed call sits between its own pair of events; the sources rotate over four 112.9 MB windows so that no launch
finds its input in the Infinity Cache (4 x 112.9 MB > 256 MiB) — jl_time_pileup alone repeats ONE window and may.  Reported:
median and minimum of `reps`, the bytes of the matrix over the median, and the ratio.  Nothing is asserted: no time is promised.
usage: deletions_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, msa, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
L, N = 3000, 100_000
matrix_bytes = 3 * L * msa.plane_stride(N)

stream = torch.cuda.Stream()


def filled(seed):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
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


def report(name, us):
    med = float(np.median(us))
    print(f"{name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}; {matrix_bytes / med * 1e-6:.2f} TB/s of matrix at the median", flush=True)
    return med


srcs = [filled(2 + q) for q in range(4)]
genes = np.array([(1, L + 1)], dtype=capi.GENE)
for s in srcs:                                     # warm-up: code objects, the plan, the buffers
    s.pileup_async(genes)
    cnt = s.codon_deletions()
print(f"matrix {matrix_bytes / 1e6:.1f} MB; del3.max = {cnt[:, 1].max()}, partial.max = {cnt[:, 2].max()}, codon.max = {cnt[:, 0].max()}", flush=True)
plain_us = report("plain pileup 100000 x 3000 (pileup_async, rotating)", timed([lambda q=q: srcs[q % 4].pileup_async(genes) for q in range(reps)]))
del_us = report("codon deletions 100000 x 3000 (whole call, rotating)", timed([lambda q=q: srcs[q % 4].codon_deletions(wait=False) for q in range(reps)]))
print(f"  codon deletions / plain pileup = {del_us / plain_us:.2f}", flush=True)
one = 1e3 * srcs[0].time_pileup(reps)
print(f"jl_time_pileup of ONE window, average of {reps} back-to-back launches: {one:.1f} us; codon deletions / that = {del_us / one:.2f}", flush=True)
for x in srcs:
    x.sync()
    x.close()
