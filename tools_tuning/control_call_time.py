"""jl_control_call_async on the device at 100 000 reads x 3000 columns, by HIP events (torch) on the contexts' stream: the whole call
(the checks on the host, the control kernel over the 1000 positions' histograms of both contexts, the compaction) beside
jl_call_async of the same window (the error-model call: call_kernel + compact_kernel), first against a control of equal depth, then
against one ten times shallower.  Both pileups are done before the timed calls; the windows carry the 6 / 5 / 4 / 3 % mixture
against a control without minors, so the called codons sum long tails and the noise codons short ones (the divergence between
lanes that kernels_control.hip expects).  Reported: median and minimum of `reps`, the ratio to the error-model call, and the
rows each call produced.  Every timed call sits between its own pair of events.  Nothing is asserted: no time is promised.
usage: control_call_time.py [reps]"""
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
genes = np.array([(1, L + 1)], dtype=capi.GENE)


def filled(seed, n, minors):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(n, L)
    j.synth_fill(synth.SynthParams(seed=seed, partial_rate=0.05, minor_permille=minors), ref)
    j.pileup_async(genes, ref)
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


prm = capi.default_params()
sample = filled(2, N, (60, 50, 40, 30))
sample.call_async(prm)                     # warm-up: code objects
n_model = len(sample.call_fetch())
model_us = report(f"jl_call_async (error model), {n_model} rows", timed([lambda: sample.call_async(prm) for _ in range(reps)]))
for name, n in (("equal depth", N), ("ten times shallower", N // 10)):
    control = filled(3, n, (0, 0, 0, 0))
    sample.control_call_async(control, prm)    # warm-up: code objects, the result buffers
    n_rows = len(sample.control_call_fetch()[0])
    us = report(f"jl_control_call_async, control of {n} reads ({name}), {n_rows} rows",
                timed([lambda: sample.control_call_async(control, prm) for _ in range(reps)]))
    print(f"  control call / error-model call = {us / model_us:.2f}", flush=True)
    sample.sync()
    control.close()
sample.close()
