"""jl_sites_assemble + the phasing of the site matrix (docs/SPEC.md §18) on the bench window, 100 000 reads x 3000 columns with a
handful of sites, by HIP events (torch) on the contexts' one stream.  Beside it the plain phasing of the same window with the codon
rows of the same table.  Every timed call sits between its own pair of events; the sources rotate over four 112.9 MB windows so
that no launch finds its input in the Infinity Cache (4 x 112.9 MB > 256 MiB).  The assemble call is timed alone too: it streams
18 S stride bytes (nine plane rows read, nine written, per site), reported over its median.  The events see what the stream does —
the table's copy from pinned memory and the launches; the host side of the calls shows as the gap between them only when the stream
runs dry.  Reported: median and minimum of `reps`.  Nothing is asserted: no time is promised.
usage: sites_time.py [reps]"""
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
CODON_COLS, DEL_COLS = (300, 900, 1500, 2100), (900, 1200)     # one deletion at a variant position, one elsewhere
stride = msa.plane_stride(N)

stream = torch.cuda.Stream()


def filled(seed):
    j = capi.Juliet(0, stream=stream.cuda_stream)
    j.alloc(N, L)
    j.synth_fill(synth.SynthParams(seed=seed, del_rate=4e-3, partial_rate=0.05, minor_permille=(60, 50, 40, 30)), synth.reference(2, L))
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
    print(f"{name}: median {med:.1f} us, min {us.min():.1f} us over {len(us)}", flush=True)
    return med


ref = synth.reference(2, L)
plain_table = np.zeros(len(CODON_COLS), dtype=capi.VARIANT)
for k, c in enumerate(CODON_COLS):
    r = 16 * int(ref[c]) + 4 * int(ref[c + 1]) + int(ref[c + 2])
    plain_table[k]["col"], plain_table[k]["ref_codon"], plain_table[k]["codon"] = c, r, (r + 1) % 64
sites, site_table = [], []
for c in sorted(set(CODON_COLS) | set(DEL_COLS)):
    if c in CODON_COLS:
        row = plain_table[list(CODON_COLS).index(c)].copy()
        row["col"] = 3 * len(sites)
        site_table.append(row)
        sites.append((c, capi.SITE_CODON, int(row["ref_codon"]) if c in DEL_COLS else capi.SITE_NO_FILL))
    if c in DEL_COLS:
        row = np.zeros((), dtype=capi.VARIANT)
        row["col"], row["codon"], row["ref_codon"] = 3 * len(sites), capi.SITE_DELETED, capi.SITE_PRESENT
        site_table.append(row)
        sites.append((c, capi.SITE_DELETION, capi.SITE_NO_FILL))
site_table = np.array(site_table, dtype=capi.VARIANT)
S = len(sites)
moved = 18 * S * stride

srcs = [filled(2 + q) for q in range(4)]
pc = capi.Juliet(0, stream=stream.cuda_stream)
for s in srcs:                                     # warm-up: code objects, the buffers of both contexts
    s.phase_async(plain_table, 10)
    s.phase_fetch(cap_var=64)
    pc.sites_assemble(s, sites)
    pc.phase_async(site_table, 10)
    got = pc.phase_fetch(cap_var=64)
print(f"window {3 * L * stride / 1e6:.1f} MB, {S} sites, the assemble moves {moved / 1e3:.1f} KB; site phasing: {got['summary']}", flush=True)


def both(q):
    pc.sites_assemble(srcs[q % 4], sites)
    pc.phase_async(site_table, 10)


plain_us = report("plain phasing of the window, 4 positions (phase_async, rotating)", timed([lambda q=q: srcs[q % 4].phase_async(plain_table, 10) for q in range(reps)]))
asm_us = report(f"sites_assemble alone, {S} sites (rotating)", timed([lambda q=q: pc.sites_assemble(srcs[q % 4], sites) for q in range(reps)]))
print(f"  {moved / asm_us * 1e-3:.2f} GB/s of 18 S stride at the median", flush=True)
both_us = report(f"sites_assemble + phasing of the site matrix, {S} positions (rotating)", timed([lambda q=q: both(q) for q in range(reps)]))
print(f"  (assemble + site phasing) / plain phasing = {both_us / plain_us:.2f}", flush=True)
for x in srcs + [pc]:
    x.sync()
    x.close()
