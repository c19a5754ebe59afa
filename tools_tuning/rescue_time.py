"""jl_phase_rescue_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream, for
(Vp, H) = (16, 9), (16, 702) and (128, 702): the whole call (packing the pattern on the host, its upload, the kernel).  Beside
it, as the scale, the existing phasing of the same window at the same Vp positions (jl_phase_async with a table of Vp rows:
its upload, plan and launches).  The pattern rows are the haplotypes that phasing reports, filled up to H with seeded codons:
the kernel's work does not depend on what they hold.  Every timed call sits between its own pair of events; the sources rotate
over four 112.5 MB windows.  Reported: median and minimum of `reps`.  Nothing is asserted: no time is promised anywhere.
usage: rescue_time.py [reps]"""
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


def table(vp):
    """Vp variant rows at codon starts spread over the window (the synthetic sample's own edits lie among them or not: the phasing
    launch reads the same nine plane rows a position either way)."""
    t = np.zeros(vp, dtype=capi.VARIANT)
    t["col"] = 3 * (np.arange(vp) * ((L // 3 - 1) // vp))
    t["codon_pos"] = t["col"] // 3
    t["coverage"] = N
    return t


srcs = [filled(2 + q) for q in range(4)]
for vp, n_hap in ((16, 9), (16, 702), (128, 702)):
    tab = table(vp)
    for s in srcs:
        s.phase_async(tab, 10)       # warm-up: code objects, buffers of this shape
    ph = srcs[0].phase_fetch(want_reads=False, cap_var=vp)
    phase_us = report(f"phasing Vp = {vp} (table upload + plan + launches)", timed([lambda q=q: srcs[q % 4].phase_async(tab, 10) for q in range(reps)]))
    pos_cols = tab["col"].astype(np.uint32)
    pattern = np.random.default_rng(vp + n_hap).integers(0, 64, size=(n_hap, vp), dtype=np.uint8)
    k = min(n_hap, len(ph["hap_pattern"]))
    if ph["summary"]["n_positions"] == vp:
        pattern[:k] = ph["hap_pattern"][:k]
    for s in srcs:
        out = s.phase_rescue(pos_cols, pattern, 1)
    us = report(f"rescue  Vp = {vp}, H = {n_hap}", timed([lambda q=q: srcs[q % 4].phase_rescue(pos_cols, pattern, 1, wait=False) for q in range(reps)]))
    print(f"  tally of the last window {out['tally'].tolist()}; rescue / phasing = {us / phase_us:.2f}", flush=True)
for x in srcs:
    x.sync()
    x.close()
