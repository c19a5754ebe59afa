"""jl_variant_linkage_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole
call (staging the positions and codons on the host, their upload, zeroing the tables, the row kernel, the product kernel) at the
window's own variant table (the rows a run calls on it: V variants at P positions), and at V = P = 1024 on synthetic positions
(every second column a codon start, seeded codons: the kernels' work does not depend on what the rows hold).  Beside it, as the
scale, the existing phasing of the same window with the same table (jl_phase_async: its upload, plan and launches).  Reported:
median and minimum of `reps`, and the achieved word-AND-popcounts a second: R (R + 1) / 2 pairs of the R = P + V stacked rows,
the upper triangle with its diagonal, times ceil(n_reads / 32) words, over the median time of the whole call.  Every timed call
sits between its own pair of events; the sources rotate over four 112.5 MB windows.  Nothing is asserted: no time is promised.
usage: linkage_time.py [reps]"""
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
    print(f"{name}: median {np.median(us):.1f} us, min {us.min():.1f} us over {len(us)}", flush=True)
    return float(np.median(us))


def linkage(name, pos_cols, var_pos, var_codon):
    for s in srcs:
        out = s.variant_linkage(pos_cols, var_pos, var_codon)       # warm-up: code objects, buffers of this shape
    us = report(name, timed([lambda q=q: srcs[q % 4].variant_linkage(pos_cols, var_pos, var_codon, wait=False) for q in range(reps)]))
    r = len(pos_cols) + len(var_pos)
    ops = r * (r + 1) // 2 * ((N + 31) // 32)
    print(f"  {ops / (us * 1e-6):.3e} word-AND-popcounts a second; both.max = {out['both'].max()}, joint.max = {out['joint'].max()}", flush=True)
    return us


srcs = [filled(2 + q) for q in range(4)]
ref = synth.reference(2, L)
genes = np.array([(1, L + 1)], dtype=capi.GENE)
srcs[0].run_async(genes, ref, capi.default_params(), None, True, 10, False)
var = srcs[0].run_fetch(True, False, cap_var=256)["variants"].copy()
pos_cols = np.unique(var["col"]).astype(np.uint32)
var_pos = np.searchsorted(pos_cols, var["col"]).astype(np.uint32)
print(f"the window's own table: V = {len(var)} variants at P = {len(pos_cols)} positions", flush=True)
for s in srcs:
    s.phase_async(var, 10)           # warm-up
phase_us = report(f"phasing of the same table (table upload + plan + launches)", timed([lambda q=q: srcs[q % 4].phase_async(var, 10) for q in range(reps)]))
own_us = linkage(f"linkage V = {len(var)}, P = {len(pos_cols)}", pos_cols, var_pos, var["codon"].copy())
print(f"  linkage / phasing = {own_us / phase_us:.2f}", flush=True)
big = capi.LINK_MAX
linkage(f"linkage V = P = {big}", 2 * np.arange(big, dtype=np.uint32), np.arange(big, dtype=np.uint32),
        np.random.default_rng(big).integers(0, 64, size=big, dtype=np.uint8))
for x in srcs:
    x.sync()
    x.close()
