"""`juliet --batch` against one `juliet` process per sample, end to end.

Writes N rich-QV BAMs with `juliet-synth --rich-qv --ref-seed K --seed s` (one reference, so one config fits them all), then
times, three times each (--runs), the two ways of calling them:
  single  N child processes `juliet OPTS in.bam out.json`, one after the other, each under its own time-out
  batch   one child process `juliet OPTS --timing --batch list.tsv`
with OPTS = `-c cfg.json --mode-phasing --min-qv 20` (bench.py end_to_end's options; --opts to change).  Prints one JSON line:
samples, reads_per_sample, wall_ms (median and every run) of both forms, reads/s and samples/s of both, the speed-up.  The
batch's --timing lines of its last run go to --timing-out (default: batch_e2e_<N>x<R>_timing.txt in the current
directory) — where its time goes.

    python tools_tuning/batch_e2e.py --samples 96 --reads 6000
    python tools_tuning/batch_e2e.py --samples 32 --reads 100000
"""
import argparse
import concurrent.futures
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "minorseq_amd", "bin")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=96)
    ap.add_argument("--reads", type=int, default=6000, help="reads per sample")
    ap.add_argument("--cols", type=int, default=3000)
    ap.add_argument("--ref-seed", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--opts", default="-c cfg.json --mode-phasing --min-qv 20")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per single run; the batch gets this per sample")
    ap.add_argument("--synth-jobs", type=int, default=8)
    ap.add_argument("--dir", default=None, help="work directory (default: a temporary one, removed at the end)")
    ap.add_argument("--timing-out", default=None, help="file for the batch's --timing lines of its last run")
    args = ap.parse_args()
    work = args.dir or tempfile.mkdtemp(prefix="batch_e2e_")
    os.makedirs(work, exist_ok=True)
    try:
        print(json.dumps(measure(args, work)), flush=True)
    finally:
        if not args.dir:
            shutil.rmtree(work, ignore_errors=True)


def synth(work, k, args):
    bam = f"s{k:04d}.bam"
    cmd = [os.path.join(BIN, "juliet-synth"), "--rich-qv", "--reads", str(args.reads), "--cols", str(args.cols),
           "--seed", str(1000 + k), "--ref-seed", str(args.ref_seed), "-o", bam]
    if k == 0:
        cmd += ["--config-out", "cfg.json"]
    subprocess.run(cmd, cwd=work, check=True, stdout=subprocess.DEVNULL)
    return bam


def run(cmd, cwd, timeout):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"batch_e2e: {' '.join(cmd)} ended with status {r.returncode}")
    return r


def measure(args, work):
    t = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(args.synth_jobs) as ex:
        bams = list(ex.map(lambda k: synth(work, k, args), range(args.samples)))
    synth_s = time.perf_counter() - t
    opts = args.opts.split()
    juliet = os.path.join(BIN, "juliet")
    with open(os.path.join(work, "list.tsv"), "w") as f:
        for b in bams:
            f.write(f"{b}\tbatch_{b}.json\n")
    single_ms, batch_ms = [], []
    timing = ""
    for _ in range(args.runs):      # (alternating, so that neither form always runs on a warmer page cache)
        t = time.perf_counter()
        for b in bams:
            run([juliet, *opts, b, f"single_{b}.json"], work, args.timeout)
        single_ms.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        r = run([juliet, *opts, "--timing", "--batch", "list.tsv"], work, args.timeout * args.samples)
        batch_ms.append(1e3 * (time.perf_counter() - t))
        timing = r.stderr
    same = all(strip(os.path.join(work, f"batch_{b}.json")) == strip(os.path.join(work, f"single_{b}.json")) for b in bams)
    tout = args.timing_out or f"batch_e2e_{args.samples}x{args.reads}_timing.txt"
    with open(tout, "w") as f:
        f.write(timing)
    reads = args.samples * args.reads

    def form(ms):
        m = statistics.median(ms)
        return {"wall_ms": round(m, 1), "runs_ms": [round(x, 1) for x in ms], "reads_per_s": round(reads / (m / 1e3)),
                "samples_per_s": round(args.samples / (m / 1e3), 2)}

    s, b = form(single_ms), form(batch_ms)
    return {"samples": args.samples, "reads_per_sample": args.reads, "cols": args.cols, "opts": args.opts,
            "single": s, "batch": b, "speedup": round(s["wall_ms"] / b["wall_ms"], 2), "outputs_equal": same,
            "synth_s": round(synth_s, 1), "timing_lines": tout}


def strip(path):
    j = json.load(open(path))
    j["input"].pop("timestamp")
    j["input"].pop("command_line")
    return j


if __name__ == "__main__":
    main()
