"""The registers, scratch, occupancy and LDS of the three kernels on the shared haplotype walk (csrc/hap_walk.h: the rescue, the
nearest-haplotype call, the recombinant call), from the compiler's kernel-resource-usage remarks for gfx950 (no GPU: hipcc
cross-compiles, device code only).  Each is held to the figures of the commit before the shared walk, recorded under "== parent"
in profiles/hap_walk/resource_usage.txt: no scratch, occupancy not below, VGPRs and static LDS not above.

Only the remarks are read; nothing looks into the assembly.

Figures as of the shared walk ("== new" of the record), parent -> new:
  phase_rescue_kernel        VGPRs 110 -> 110, 4 waves/SIMD, scratch 0, LDS 6912
  phase_nearest_kernel       VGPRs 122 -> 122, 4 waves/SIMD, scratch 0, LDS 4096
  phase_recombinants_kernel  VGPRs 135 -> 131, 3 waves/SIMD, scratch 0, LDS 4096
The counts are sensitive to how the shared pieces are called: a functor handed to the walk by reference, or the per-read expansion
behind a function, costs the rescue and the nearest kernel one to three registers (docs/HISTORY.md).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minorseq_amd", "csrc")
RECORD = os.path.join(ROOT, "profiles", "hap_walk", "resource_usage.txt")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--offload-arch=gfx950", "-ffp-contract=off",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
KERNELS = {"phase_rescue_kernel": "kernels_rescue.hip", "phase_nearest_kernel": "kernels_nearest.hip",
           "phase_recombinants_kernel": "kernels_recomb.hip"}


def parse(lines):
    """{kernel name: {"VGPRs", "Scratch", "Occupancy", "LDS"}} from remark lines."""
    out, cur = {}, None
    for line in lines:
        line = re.sub(r"^.*remark: ", "", line).strip()
        line = re.sub(r"\s*\[-Rpass-analysis.*$", "", line)
        m = re.match(r"Function Name: _ZN12_GLOBAL__N_1\d+(\w+_kernel)E", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)   # (not "VGPRs Spill")
        if m and cur is not None:
            cur[{"S": "Scratch", "O": "Occupancy", "L": "LDS", "V": "VGPRs"}[m.group(1)[0]]] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def parent():
    text = open(RECORD).read()
    figs = parse(text.split("== new")[0].splitlines())
    assert set(figs) == set(KERNELS)
    return figs


@pytest.fixture(scope="module")
def compiled():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = {}
    for src in KERNELS.values():
        r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", os.devnull], cwd=CSRC, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        out.update(parse(r.stderr.splitlines()))
    assert set(out) == set(KERNELS)
    return out


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_less_occupancy_no_more_lds(compiled, parent, kernel):
    f, p = compiled[kernel], parent[kernel]
    print(kernel, "new", f, "parent", p)
    assert f["Scratch"] == 0, (f, p)
    assert f["Occupancy"] >= p["Occupancy"], (f, p)
    assert f["LDS"] <= p["LDS"], (f, p)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_more_registers(compiled, parent, kernel):
    f, p = compiled[kernel], parent[kernel]
    print(kernel, "new", f, "parent", p)
    assert f["VGPRs"] <= p["VGPRs"], (f, p)
