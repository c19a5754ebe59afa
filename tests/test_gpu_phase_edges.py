"""Every phasing pipeline at its position-count, table, selection and id-width edges (tests/phase_edges.py: 46 designed windows
with host variant tables), field by field and read by read against a plain numpy statement of SPEC §8.

Each case goes through the stage API on a fresh context and, with the table the call stage gives for its matrix, through the
whole-path run and through group runs of three windows, with the per-read ids written by the phasing launch and by the separate
launch (phase_edges.NO_WHOLE_PATH, NO_GROUP: the few that cannot, and why).  Which pipeline ran — one-word, two-word or
multi-word — with its key words, positions, overflow bits and id width, and who wrote a group launch's ids, is read from the
-DJL_TUNING build of the library (jl_tuning_ctx_meta, jl_tuning_phase_form, jl_tuning_group_ids_inline) and asserted, so a case
that lands on another path fails.  A process loads one library, so the parts run in child processes (tests/phase_edges_child.py).
Runs only on a real MI355X: `pytest -m gpu`.
"""
import os
import subprocess
import sys
import time

import pytest

import phase_edges as pe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNING_LIB = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")
ATTEMPTED = set()   # parts whose child was started in this session
COMPARED = {}       # part -> the cases its child compared


def run_child(part):
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: tools_tuning/build_tuning_lib.sh (build() runs it)"
    env = dict(os.environ, JL_LIB=TUNING_LIB)
    for k in ("JL_NO_GRAPH", "JL_NO_FOLD_CALL", "JL_FORCE_IDS_WAIT_TIMEOUT", "JL_EXCHANGE_STAGED"):
        env.pop(k, None)
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(HERE, "phase_edges_child.py"), part], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print("part %s: %.1f s" % (part, time.time() - t0))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "PHASE-EDGES-OK %s" % part in out.stdout
    return [line.split()[1] for line in out.stdout.splitlines() if line.startswith("COMPARED ")]


def compare_part(part):
    ATTEMPTED.add(part)
    names = run_child(part)
    assert names == pe.PARTS[part], (part, names)
    COMPARED[part] = names


@pytest.mark.parametrize("part", [p for p in pe.PARTS if p != "wide"])
def test_designed_windows_through_every_entry_that_phases(part):
    """Every case of the part: summary, positions, haplotypes, hit, co-occurrence and every read's id equal the numpy statement on
    every entry, and the library says the pipeline ran that the case was designed for."""
    compare_part(part)


def test_windows_on_both_sides_of_the_plans_lds_bitset():
    """131072 and 131073 columns, 64 reads: the plan ranks the variant columns out of its LDS bitset, then through HBM."""
    compare_part("wide")


def test_the_form_of_a_context_only_grows():
    """One context asked for 10, 11, 21, then 10 positions; a fresh one for 21 first: the re-run protocol and the key buffer's
    growth, every result exact."""
    assert run_child("growth") == list(pe.GROWTH) + [pe.GROWTH_FRESH, pe.GROWTH[0]]


def test_every_case_was_compared():
    """No case is skipped or excused: the children compared as many cases as the module defines.  A part whose item was not
    started in this session (deselected) is run here; one that was started and did not finish its comparison is not started again."""
    failed = sorted(ATTEMPTED - set(COMPARED))
    assert not failed, "parts that were run and did not compare their cases: %s" % failed
    for part in pe.PARTS:
        if part not in ATTEMPTED:
            compare_part(part)
    assert sum(len(v) for v in COMPARED.values()) == len(pe.CASES) == 46
    assert sorted(n for v in COMPARED.values() for n in v) == sorted(pe.CASES)
