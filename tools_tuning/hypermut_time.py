"""jl_read_hypermut_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole
call (the reference row's upload, the counting kernel, the combine kernel or the zeroing for the atomics, and the test kernel).
Beside it, as the yardstick, jl_read_stats_async of the same window at the same commit between the same events — both read the
matrix once, the hypermutation counters two halo columns a segment more.  Every timed call sits between its own pair of events;
the sources rotate over four 112.9 MB windows so that no launch finds its input in the Infinity Cache (4 x 112.9 MB > 256 MiB).
Reported: median and minimum of `reps` in us, the bytes read (3 bits a cell, halo included), the bytes over the median and their
fraction of 8 TB/s.  With JL_LIB pointing at a -DJL_TUNING build of the library (tools_tuning/build_tuning_lib.sh) every flush
period (k = 4, 5, 6) and both ways of combining the column segments are timed; the product library times the shape it ships.
Nothing is asserted: no time is promised.
usage: hypermut_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from minorseq_amd import capi, msa, synth  # noqa: E402

import readstats_shape  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])
lib = capi.load_library()

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
L, N = 3000, 100_000
shape = readstats_shape.shape(N, L)
matrix_bytes = 3 * L * msa.plane_stride(N)
halo_bytes = 3 * 2 * (shape["n_segs"] - 1) * msa.plane_stride(N)      # two columns beyond every segment but the last
PEAK = 8e12

stream = torch.cuda.Stream()


def filled(seed):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, sub_rate=0.02, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
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


def report(name, us, nbytes):
    med = float(np.median(us))
    print(f"{name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}; {nbytes} bytes read, {nbytes / med * 1e-6:.2f} TB/s "
          f"= {nbytes / med * 1e6 / PEAK:.2f} of 8 TB/s at the median", flush=True)
    return med


srcs = [filled(2 + q) for q in range(4)]
ref = synth.reference(2, L)
for s in srcs:                                     # warm-up: code objects, the buffers
    s.read_stats(ref)
    cnt, p, lp = s.read_hypermut(ref)
print(f"matrix {matrix_bytes / 1e6:.1f} MB + halo {halo_bytes / 1e6:.2f} MB ({shape['n_chunks']} chunks x {shape['n_segs']} segments of {shape['seg_cols']}); "
      f"target sites.max = {cnt[0].max()}, target mut.max = {cnt[1].max()}, control sites.max = {cnt[2].max()}, control mut.max = {cnt[3].max()}, "
      f"reads with p < 0.05: {(p < 0.05).sum()}", flush=True)
rs_us = report("read stats 100000 x 3000 (whole call, rotating)", timed([lambda q=q: srcs[q % 4].read_stats(ref, wait=False) for q in range(reps)]), matrix_bytes)
forms = [(0, -1, "the shipped shape")]
if hasattr(lib, "jl_tuning_hypermut_shape"):
    forms = [(k, c, f"k = {k} (flush every {2 ** k - 1} columns), segments combined by {'a second kernel' if c == 0 else 'atomics'}")
             for c in (0, 1) for k in (6, 5, 4)]
for k, c, what in forms:
    if hasattr(lib, "jl_tuning_hypermut_shape"):
        assert lib.jl_tuning_hypermut_shape(k, c) == 0
        for s in srcs:                             # warm-up of this form, and its table against the shipped shape's
            got = s.read_hypermut(ref)[0]
            assert s is not srcs[-1] or (got == cnt).all()
    us = report(f"hypermutation counters + test 100000 x 3000, {what} (whole call, rotating)",
                timed([lambda q=q: srcs[q % 4].read_hypermut(ref, wait=False) for q in range(reps)]), matrix_bytes + halo_bytes)
    print(f"  hypermutation / read stats = {us / rs_us:.2f}", flush=True)
for x in srcs:
    x.sync()
    x.close()
