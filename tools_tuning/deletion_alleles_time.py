"""jl_deletion_alleles_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream: the whole
call — the counting launch, the host's wait for its one number, the memsets, the walk over the runs and the rows with their flank
counts.  Three windows: the bench window (synthetic, no deletion model), one 300-base allele planted in 10 % of its reads, and
one-base deletions at 1e-3 a cell (the generator's del_rate).  Beside it, in the same run, jl_codon_deletions_async (§16) and the
plain pileup of the same windows: all three read the matrix.  Every timed call sits between its own pair of events; the sources
rotate over three 112.9 MB windows of each kind, so that no launch finds its input in the Infinity Cache (3 x 112.9 MB > 256 MiB).
Reported: median and minimum of `reps`, the bytes of the matrix over the median, and the ratios.  Nothing is asserted: no time is
promised.
usage: deletion_alleles_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, msa, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
L, N = 3000, 100_000
matrix_bytes = 3 * L * msa.plane_stride(N)
stream = torch.cuda.Stream()
genes = np.array([(1, L + 1)], dtype=capi.GENE)


def filled(seed, del_rate=0.0, plant=False):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, del_rate=del_rate, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
    if plant:   # columns 1000 .. 1299 deleted in every tenth read: the planes of those columns, a byte at a time
        planes = j.download_planes()
        reads = np.zeros(planes.shape[2] * 8, dtype=np.uint8)
        reads[0:N:10] = 1
        mask = np.packbits(reads, bitorder="little")
        planes[1000:1300, 0] &= ~mask
        planes[1000:1300, 1] &= ~mask
        planes[1000:1300, 2] |= mask
        t = torch.from_numpy(planes).cuda()
        j.adopt(t.data_ptr(), N, L, planes.shape[2], keep_alive=t)
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
    print(f"  {name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}; {matrix_bytes / med * 1e-6:.2f} TB/s of matrix at the median", flush=True)
    return med


print(f"matrix {matrix_bytes / 1e6:.1f} MB, {reps} repetitions a line", flush=True)
for name, kw in (("bench window", {}), ("one 300-base allele in 10 % of the reads", dict(plant=True)), ("one-base deletions at 1e-3 a cell", dict(del_rate=1e-3))):
    srcs = [filled(2 + q, **kw) for q in range(3)]
    for s in srcs:                                     # warm-up: code objects, the plan, the buffers
        s.pileup_async(genes)
        s.codon_deletions()
        res = s.deletion_alleles()
    print(f"{name}: bounded runs {int(res['runs'][0])}, open runs {int(res['runs'][1])}, alleles {len(res['alleles'])}, "
          f"longest {int(res['alleles']['len'].max()) if len(res['alleles']) else 0}", flush=True)
    plain = report("plain pileup (pileup_async)", timed([lambda q=q: srcs[q % 3].pileup_async(genes) for q in range(reps)]))
    cod = report("codon deletions (whole call)", timed([lambda q=q: srcs[q % 3].codon_deletions(wait=False) for q in range(reps)]))
    dal = report("deletion alleles (whole call)", timed([lambda q=q: srcs[q % 3].deletion_alleles(wait=False) for q in range(reps)]))
    print(f"  deletion alleles / codon deletions = {dal / cod:.2f}, / plain pileup = {dal / plain:.2f}", flush=True)
    for x in srcs:
        x.sync()
        x.close()
