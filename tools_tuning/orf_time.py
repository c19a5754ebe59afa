"""jl_read_orf_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole call
(the uploads of the reference row and of the segment table, the counting kernel and the combine kernel).  Beside it, as the
yardsticks, jl_read_hypermut_async and jl_read_stats_async of the same window in the same process between the same events.  Two
span lists: ONE span over the whole window (1000 codons: the matrix is read once, as the two siblings read it), and FIFTEEN
overlapping spans in the three frames (the stage's bytes grow with the sum of the span lengths, so the time per span-column is
reported too).  Every timed call sits between its own pair of events; the sources rotate over four 112.9 MB windows so that no
launch finds its input in the Infinity Cache (4 x 112.9 MB > 256 MiB).  Reported: median and minimum of `reps` in us, the bytes
read (3 bits a cell of every span-column), the bytes over the median and their fraction of 8 TB/s, and picoseconds per
span-column and read word.  With JL_LIB pointing at a -DJL_TUNING build of the library (tools_tuning/build_tuning_lib.sh) every
flush period (k = 4, 5, 6) is timed; the product library times the shape it ships.  Nothing is asserted: no time is promised.
usage: orf_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from minorseq_amd import capi, msa, synth  # noqa: E402

import orf_shape  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])
lib = capi.load_library()

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
L, N = 3000, 100_000
PEAK = 8e12
ONE = [(0, L // 3)]
# fifteen open reading frames of 150 .. 290 codons, five in each frame, each overlapping the next two or more: 9900 span-columns
FIFTEEN = [(150 * g + g % 3, 150 + 10 * g) for g in range(15)]
assert all(c + 3 * n <= L for c, n in FIFTEEN) and sorted({c % 3 for c, _ in FIFTEEN}) == [0, 1, 2]

stream = torch.cuda.Stream()


def filled(seed):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, sub_rate=0.02, del_rate=4e-3, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
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


def report(name, us, nbytes, span_cols=None):
    med = float(np.median(us))
    per = "" if span_cols is None else f"; {med * 1e6 / (span_cols * ((N + 31) // 32)):.2f} ps per span-column and read word, {med * 1e3 / span_cols:.2f} ns per span-column"
    print(f"{name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}; {nbytes} bytes read, {nbytes / med * 1e-6:.2f} TB/s "
          f"= {nbytes / med * 1e6 / PEAK:.2f} of 8 TB/s at the median{per}", flush=True)
    return med


srcs = [filled(2 + q) for q in range(4)]
ref = synth.reference(2, L)
matrix_bytes = 3 * L * msa.plane_stride(N)
for s in srcs:                                     # warm-up: code objects, the buffers
    s.read_stats(ref)
    s.read_hypermut(ref)
    base = {len(sp): s.read_orf(sp, ref) for sp in (ONE, FIFTEEN)}
cnt, first = base[1]
print(f"matrix {matrix_bytes / 1e6:.1f} MB; one span: covered.max = {cnt[0].max()}, gap cells.max = {cnt[1].max()}, codons read.max = {cnt[2].max()}, "
      f"stops.max = {cnt[3].max()}, reads with a stop: {(first != capi.ORF_NO_STOP).sum()}", flush=True)
rs_us = report("read stats 100000 x 3000 (whole call, rotating)", timed([lambda q=q: srcs[q % 4].read_stats(ref, wait=False) for q in range(reps)]), matrix_bytes)
hm_us = report("hypermutation counters + test 100000 x 3000 (whole call, rotating)",
               timed([lambda q=q: srcs[q % 4].read_hypermut(ref, wait=False) for q in range(reps)]), matrix_bytes)
ks = (6, 5, 4) if hasattr(lib, "jl_tuning_orf_shape") else (0,)
for k in ks:
    if k:
        assert lib.jl_tuning_orf_shape(k) == 0
    for spans, name in ((ONE, "one span over the window"), (FIFTEEN, "fifteen overlapping spans in three frames")):
        shape = orf_shape.shape([n for _, n in spans], N, k)
        span_cols = 3 * sum(n for _, n in spans)
        for s in srcs:                             # warm-up of this form, and its arrays against the shipped shape's
            got = s.read_orf(spans, ref)
            assert s is not srcs[-1] or all((a == b).all() for a, b in zip(got, base[len(spans)]))
        us = report(f"reading-frame counters 100000 x 3000, {name}, k = {shape['k']} (flush every {shape['flush_codons']} codons), "
                    f"{shape['n_chunks']} chunks x {shape['n_segs']} segments of {shape['seg_codons']} codons (whole call, rotating)",
                    timed([lambda q=q: srcs[q % 4].read_orf(spans, ref, wait=False) for q in range(reps)]), span_cols * 3 * msa.plane_stride(N), span_cols)
        print(f"  reading-frame / read stats = {us / rs_us:.2f}, / hypermutation = {us / hm_us:.2f}", flush=True)
for x in srcs:
    x.sync()
    x.close()
