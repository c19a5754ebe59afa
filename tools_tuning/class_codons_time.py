"""jl_class_codons_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream:
  the per-class codon tables (label and column upload + masks + counting) with H = 5 and with H = 64 classes at all 1000
  evaluated positions of one whole-window gene,
  for the same H the route to the same tables without it: per class, jl_msa_take_async of the class's reads into a spare
  context + jl_run_async of that context without phasing (pileup + calls: the run's codon histograms are the class's table),
  the plain pileup of the window.
Every timed call sits between its own pair of events; the sources rotate over four 112.5 MB windows so that no launch finds
its input in the Infinity Cache (4 x 112.5 MB > 256 MiB).  Reported: median, minimum and the 10th..90th percentile spread of
`reps`.  No bound is asserted: the ratios are what the script is for.
usage: class_codons_time.py [reps]"""
import os
import sys

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
genes = np.array([(1, L + 1)], dtype=capi.GENE)
cols = np.arange(0, L, 3, dtype=np.uint32)      # the gene's evaluated positions: every third column
plane = lambda n: (n + 1023) // 1024 * 128      # bytes per plane row (jl_plane_stride)  # noqa: E731


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
    lo, hi = np.percentile(us, [10, 90])
    line = f"{name}: median {np.median(us):.1f} us, min {us.min():.1f} us, p10..p90 {lo:.1f}..{hi:.1f} us over {len(us)}"
    if n_bytes:
        line += f"; {n_bytes / 1e6:.1f} MB read, {n_bytes / (np.median(us) * 1e-6) / 1e12:.2f} TB/s = {100 * n_bytes / (np.median(us) * 1e-6) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak"
    print(line, flush=True)
    return float(np.median(us))


def labels_of(k):
    """A phasing run's shape: a major class, minors, a fifth of the reads in no class."""
    rng = np.random.default_rng(k)
    share = np.array([50.0] + [30.0 / (k - 1)] * (k - 1) + [20.0])
    lab = rng.choice(k + 1, size=N, p=share / share.sum()).astype(np.uint16)
    lab[lab == k] = 0xFFFF
    return lab


srcs = [filled(N, 2 + q) for q in range(4)]
spare = ctx()
matrix_bytes = 3 * L * plane(N)
params = capi.default_params()

# ---- the plain pileup of the window
for s in srcs:
    s.pileup_async(genes)
plain_us = report("plain pileup 100000 x 3000", timed([lambda q=q: srcs[q % 4].pileup_async(genes) for q in range(reps)]), matrix_bytes)

for k in (5, 64):
    lab = labels_of(k)
    members = [np.nonzero(lab == c)[0].astype(np.uint32) for c in range(k)]
    passes = (k + 15) // 16
    # ---- the codon tables by class: label and column upload + masks + counting
    for s in srcs:
        s.class_codons(lab, k, cols)       # warm-up: code objects, buffers of this shape
    us = report(f"class codons H = {k}, {len(cols)} positions", timed([lambda q=q: srcs[q % 4].class_codons(lab, k, cols, wait=False) for q in range(reps)]),
                passes * matrix_bytes + N * 2 + 2 * k * plane(N))

    # ---- the same tables by the calls of the parent commit: per class a take into a spare context and a run of it
    def route(q):
        for c in range(k):
            spare.take([(srcs[q % 4], members[c])], wait=False)
            spare.run_async(genes, None, params, None, False, 10, False)

    route(0)
    old = report(f"take + run per class, H = {k}", timed([lambda q=q: route(q) for q in range(max(4, reps // (4 if k < 16 else 10)))]))
    print(f"  class codons / take-and-run route = {us / old:.3f}; class codons / plain pileup = {us / plain_us:.2f}", flush=True)

for x in srcs + [spare]:
    x.sync()
    x.close()
