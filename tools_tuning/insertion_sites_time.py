"""What phasing over insertion sites (docs/SPEC.md §19) adds on the device, at 100 000 reads x 3000 columns with qualities and noise
insertions before 1 of a million cells (`juliet-synth --raw-out --rich-qv --ins-ppm 1`: about three insertions per thousand reads),
by HIP events (torch) on the one stream of all contexts.
  1. The read switch.  Builds of the same records into the same window, each between its own pair of events:
       + alleles            jl_msa_track_insertion_alleles alone (the walk without the event append)
       + alleles + events   jl_msa_track_insertion_reads (one more memset, the walk's other instantiation)
     so the difference of the two rows is what the switch adds to a tracking build.
  2. The site matrix of the window just built.  jl_sites_assemble on four codon sites; jl_sites_assemble_alleles on the same four
     codon sites plus four insertion sites (junctions of the table, all their alleles listed): the existing launch, the init pass
     over the insertion sites and the scatter over the events.  One window (112.9 MB, resident in the Infinity Cache between
     calls; either call reads a few plane rows of it only).
Reported: median, minimum and the spread (max - min of the medians of five blocks of reps).  Nothing is asserted: no time is promised.
usage: insertion_sites_time.py [reps] [min_qv]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from minorseq_amd import capi, synth  # noqa: E402

if os.environ.get("JL_LIB"):   # a tuning build of the library (tools_tuning/build_tuning_lib.sh)
    capi.load_library(os.environ["JL_LIB"])

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
min_qv = int(sys.argv[2]) if len(sys.argv) > 2 else 0
L, N = 3000, 100_000
CODON_COLS = (300, 900, 1500, 2100)
stream = torch.cuda.Stream()

rec = synth.raw_records(41, N, L, extra=("--rich-qv", "--ins-ppm", "1"))
n_ins = int(((rec["cigar"] & 15) == 1).sum())
src = capi.Juliet(0, stream=stream.cuda_stream)
src.records_upload(rec["pos"], rec["cigar"], rec["cig_off"], rec["seq4"], rec["seq_off"], rec["qual"], rec["qual_off"])
win = capi.Juliet(0, stream=stream.cuda_stream)
pc = capi.Juliet(0, stream=stream.cuda_stream)


def timed(fn, n):
    pairs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        pairs.append((e0, e1))
    stream.synchronize()
    return np.array([1e3 * a.elapsed_time(b) for a, b in pairs])


def report(name, fn):
    fn()
    win.sync()                                        # warm-up: code objects, the buffers
    pc.sync()
    blocks = [timed(fn, reps) for _ in range(5)]
    meds = [float(np.median(b)) for b in blocks]
    us = np.concatenate(blocks)
    print(f"{name}: median {np.median(us):.1f} us, min {us.min():.1f} us, block medians {min(meds):.1f} .. {max(meds):.1f} (spread {max(meds) - min(meds):.1f})", flush=True)
    return float(np.median(us))


def build(alleles, reads):
    win.track_insertion_alleles(alleles)
    win.track_insertion_reads(reads)
    return lambda: win.records_window(src, L, 0, min_qv, wait=False)


print(f"{N} reads x {L} columns, {len(rec['cigar'])} cigar words, {n_ins} 'I' ops ({1e3 * n_ins / N:.1f} per thousand reads), min_qv {min_qv}", flush=True)
off = report("build + alleles                ", build(True, False))
on = report("build + alleles + events       ", build(False, True))
events = win.insertion_reads()
jcnt, rows = win.insertion_alleles()
print(f"  the read switch adds {on - off:.1f} us to a tracking build; {len(events)} events (in frame {int((events['kind'] == 1).sum())}, "
      f"frameshift {int((events['kind'] == 2).sum())}, unread {int((events['kind'] == 3).sum())}), table {len(rows)} rows", flush=True)

codon_sites = [(c, capi.SITE_CODON, capi.SITE_NO_FILL) for c in CODON_COLS]
ins_cols = sorted(set(int(c) for c in rows["col"] if int(c) not in CODON_COLS))[:4]
alleles = [(int(r["col"]), int(r["len"]), int(r["seq"])) for r in rows if int(r["col"]) in ins_cols]
sites = sorted(codon_sites + [(c, capi.SITE_INSERTION, capi.SITE_NO_FILL) for c in ins_cols], key=lambda s: (s[0], s[1]))
plain_us = report(f"sites_assemble, {len(codon_sites)} codon sites                          ", lambda: pc.sites_assemble(win, codon_sites))
both_us = report(f"sites_assemble_alleles, the same + {len(ins_cols)} insertion sites, {len(alleles)} alleles", lambda: pc.sites_assemble_alleles(win, sites, alleles))
print(f"  the insertion sites add {both_us - plain_us:.1f} us (init pass over {len(ins_cols)} sites, scatter over a list of {n_ins} rows)", flush=True)
for x in (pc, win, src):
    x.sync()
    x.close()
