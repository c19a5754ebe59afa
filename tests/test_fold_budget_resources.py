"""The register budgets of the counting kernels, from the compiler's kernel-resource-usage remarks for gfx950 (no GPU: hipcc
cross-compiles, device code only).  The figures a kernel is held to are those recorded in profiles/fold_budget/resource_usage.txt
("== parent": the commit before the budget, "== new": with it):

  * the folded index kernels: JL_IX_FOLD_WAVES = 5 waves per SIMD, scratch no larger than recorded;
  * the unfolded index kernels: 8 waves per SIMD, no scratch;
  * call_kernel, call_group_kernel: no scratch, no more VGPRs than the parent;
  * the plane kernels: no more VGPRs than the parent and no more scratch than the parent.  (They are not free of scratch, and were
    not before: the parent's remarks give 44 to 80 bytes a lane for every plane kernel, in the tile walk, which this budget does not
    touch.  "No scratch" is therefore pinned as "none that the parent did not have".)

Only the remarks are read; nothing looks into the assembly.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minorseq_amd", "csrc")
RECORD = os.path.join(ROOT, "profiles", "fold_budget", "resource_usage.txt")
FOLD_WAVES = 5
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--offload-arch=gfx950", "-ffp-contract=off",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]


def parse(lines):
    """{kernel name without the anonymous namespace's prefix: {"VGPRs", "Scratch", "Occupancy"}} from remark lines."""
    out, cur = {}, None
    for line in lines:
        line = re.sub(r"^.*remark: ", "", line).strip()
        line = re.sub(r"\s*\[-Rpass-analysis.*$", "", line)
        m = re.match(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", m.group(1)), {})
            continue
        m = re.match(r"(VGPRs|ScratchSize|Occupancy)[^:]*: (\d+)", line)
        if m and cur is not None:
            cur[{"ScratchSize": "Scratch"}.get(m.group(1), m.group(1))] = int(m.group(2))
    return out


def recorded():
    text = open(RECORD).read()
    parent, new = text.split("== new")
    return parse(parent.splitlines()), parse(new.splitlines())


@pytest.fixture(scope="module")
def compiled():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = {}
    for src in ("kernels_pileup.hip", "kernels_call.hip"):
        r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        out.update(parse(r.stderr.splitlines()))
    return out


def pick(figs, prefix):
    got = {k: v for k, v in figs.items() if k.startswith(prefix)}
    assert got, prefix
    return got


def test_folded_index_kernels_hold_their_budget(compiled):
    _, new = recorded()
    for prefix in ("pileup_index_fold_kernelE", "pileup_index_fold_group_kernelE"):
        (name, f), = pick(compiled, prefix).items()
        assert f["Occupancy"] == FOLD_WAVES, (name, f)
        assert f["VGPRs"] <= 512 // FOLD_WAVES // 8 * 8, (name, f)
        assert f["Scratch"] <= new[name]["Scratch"], (name, f, new[name])


def test_unfolded_index_kernels_keep_eight_waves(compiled):
    for prefix in ("pileup_index_kernelE", "pileup_index_group_kernelE"):
        (name, f), = pick(compiled, prefix).items()
        assert f["Occupancy"] == 8 and f["Scratch"] == 0, (name, f)


def test_call_kernels_no_scratch_no_more_registers(compiled):
    parent, _ = recorded()
    for prefix in ("call_kernelE", "call_group_kernelE"):
        (name, f), = pick(compiled, prefix).items()
        assert f["Scratch"] == 0 and f["VGPRs"] <= parent[name]["VGPRs"], (name, f, parent[name])


def test_plane_kernels_no_more_registers_no_more_scratch(compiled):
    parent, _ = recorded()
    n = 0
    for prefix in ("pileup_planes_kernelI", "pileup_planes_group_kernelI", "pileup_fold_kernelI", "pileup_fold_group_kernelI"):
        for name, f in pick(compiled, prefix).items():
            assert f["VGPRs"] <= parent[name]["VGPRs"] and f["Scratch"] <= parent[name]["Scratch"], (name, f, parent[name])
            n += 1
    assert n == 10
