"""jl_phase_recombinants_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the context's stream,
beside jl_phase_rescue_async on the same window, positions and pattern: the whole call each (packing the pattern on the host, its
upload, the kernel).  Two shapes: the window's own table — the positions and haplotypes its phasing run reports — and 702
haplotypes x 130 positions spread over the window, of seeded codons (the kernel's work does not depend on what they hold).  Every
timed call sits between its own pair of events; the sources rotate over four 112.5 MB windows.
Reported: median and minimum of `reps`, and recombinants / rescue.  Nothing is asserted: no time is promised anywhere.
usage: recombinant_time.py [reps]"""
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
ref = synth.reference(2, L)


def filled(seed):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), ref)
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


srcs = [filled(2 + q) for q in range(4)]
genes = np.array([(1, L + 1)], dtype=capi.GENE)
ph = srcs[0].run(genes, ref, capi.default_params(), phasing=True)["phase"]
vp, n_hap = ph["summary"]["n_positions"], ph["summary"]["n_haplotypes"]
own_cols, own_pattern = ph["pos_cols"][:vp].astype(np.uint32), np.ascontiguousarray(ph["hap_pattern"][:n_hap, :vp])
print(f"the window's own table: {vp} positions, {n_hap} haplotypes", flush=True)

big_vp, big_h = 130, 702
big_cols = (3 * (np.arange(big_vp) * ((L // 3 - 1) // big_vp))).astype(np.uint32)
big_pattern = np.random.default_rng(big_vp + big_h).integers(0, 64, size=(big_h, big_vp), dtype=np.uint8)

for name, pos_cols, pattern in (("own table", own_cols, own_pattern), (f"H = {big_h}, Vp = {big_vp}", big_cols, big_pattern)):
    if len(pos_cols) == 0 or len(pattern) == 0:
        print(f"{name}: nothing to time", flush=True)
        continue
    for s in srcs:   # warm-up: code objects, buffers of this shape
        s.phase_rescue(pos_cols, pattern, 1)
        out = s.phase_recombinants(pos_cols, pattern, 1)
    rescue_us = report(f"rescue          {name}", timed([lambda q=q: srcs[q % 4].phase_rescue(pos_cols, pattern, 1, wait=False) for q in range(reps)]))
    us = report(f"recombinants    {name}", timed([lambda q=q: srcs[q % 4].phase_recombinants(pos_cols, pattern, 1, wait=False) for q in range(reps)]))
    print(f"  tally of the last window {out['tally'].tolist()}; recombinants / rescue = {us / rescue_us:.2f}", flush=True)
for x in srcs:
    x.sync()
    x.close()
