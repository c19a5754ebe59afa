"""jl_read_stats_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole call
(the compare row's upload, the counting kernel, and the combine kernel or the zeroing for the atomics).  Beside it, as the
yardstick, the plain pileup of the same window at the same commit — both read the matrix once: pileup_async between the same
events, and jl_time_pileup's own average over back-to-back launches of one window.  Every timed call sits between its own pair of
events; the sources rotate over four 112.9 MB windows so that no launch finds its input in the Infinity Cache (4 x 112.9 MB >
256 MiB) — jl_time_pileup alone repeats ONE window and may.  Reported: median and minimum of `reps` in us, the bytes of the matrix,
the bytes over the median and their fraction of 8 TB/s.  With JL_LIB pointing at a -DJL_TUNING build of the library
(tools_tuning/build_tuning_lib.sh) every flush period (k = 4, 5, 6) and both ways of combining the column segments are timed;
the product library times the shape it ships.  Nothing is asserted: no time is promised.
usage: read_stats_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, msa, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])
lib = capi.load_library()

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
L, N = 3000, 100_000
matrix_bytes = 3 * L * msa.plane_stride(N)
PEAK = 8e12

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
    print(f"{name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}; {matrix_bytes} bytes of matrix, {matrix_bytes / med * 1e-6:.2f} TB/s "
          f"= {matrix_bytes / med * 1e6 / PEAK:.2f} of 8 TB/s at the median", flush=True)
    return med


srcs = [filled(2 + q) for q in range(4)]
genes = np.array([(1, L + 1)], dtype=capi.GENE)
compare = synth.reference(2, L)
for s in srcs:                                     # warm-up: code objects, the plan, the buffers
    s.pileup_async(genes)
    st = s.read_stats(compare)
print(f"matrix {matrix_bytes / 1e6:.1f} MB; bases.max = {st[0].max()}, gaps.max = {st[1].max()}, masked.max = {st[2].max()}, "
      f"mismatches.max = {st[4].max()}", flush=True)
plain_us = report("plain pileup 100000 x 3000 (pileup_async, rotating)", timed([lambda q=q: srcs[q % 4].pileup_async(genes) for q in range(reps)]))
forms = [(0, -1, "the shipped shape")]
if hasattr(lib, "jl_tuning_read_stats_shape"):
    forms = [(k, c, f"k = {k} (flush every {2 ** k - 1} columns), segments combined by {'a second kernel' if c == 0 else 'atomics'}")
             for c in (0, 1) for k in (6, 5, 4)]
for k, c, what in forms:
    if hasattr(lib, "jl_tuning_read_stats_shape"):
        assert lib.jl_tuning_read_stats_shape(k, c) == 0
        for s in srcs:                             # warm-up of this form, and its table against the shipped shape's
            got = s.read_stats(compare)
            assert s is not srcs[-1] or (got == st).all()
    us = report(f"read stats 100000 x 3000, {what} (whole call, rotating)", timed([lambda q=q: srcs[q % 4].read_stats(compare, wait=False) for q in range(reps)]))
    print(f"  read stats / plain pileup = {us / plain_us:.2f}", flush=True)
one = 1e3 * srcs[0].time_pileup(reps)
print(f"jl_time_pileup of ONE window, average of {reps} back-to-back launches: {one:.1f} us", flush=True)
for x in srcs:
    x.sync()
    x.close()
