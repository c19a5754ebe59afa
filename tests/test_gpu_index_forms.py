"""Launches that count from the deviation index: the folded kernels' deep list walk at its round and batch edges, and the form
of a group launch by what it counts from (csrc/group_form.h: from the index, folded only when alone on the device).

Which form a launch took is read from the -DJL_TUNING build's jl_tuning_group_forms_by_count (tools_tuning/build_tuning_lib.sh,
built by build()); a process loads one library and reads JL_NO_FOLD_CALL once, so the scenarios run in child processes
(tests/index_forms_child.py).  The decision alone, on the host: test_group_form_host.py.  Runs only on a real MI355X: `pytest -m gpu`.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNING_LIB = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")


def run_child(scenario, **env_extra):
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: tools_tuning/build_tuning_lib.sh (build() runs it)"
    env = dict(os.environ, JL_LIB=TUNING_LIB, **env_extra)
    env.pop("JL_NO_GRAPH", None)
    if "JL_NO_FOLD_CALL" not in env_extra:
        env.pop("JL_NO_FOLD_CALL", None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "index_forms_child.py"), scenario], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("form", ["folded", "unfolded"])
def test_list_length_edges_of_the_walk(form):
    """One window of 116 000 reads x 36 columns whose twelve chunks have lists of 0, 1, 1023, 1024, 1025, 4096, 8191, 8192, 8193,
    16 383, 16 384 and 16 385 entries — the edges of a round (1024 entries) and of one and two batches of the folded kernels' eight
    rounds in flight —, all under the density bound (16 416) and all indexed.  Run alone three times (run 3: the single index
    kernel) and in a group of two windows three more (launch 3: the group index kernel): column counts, codon histograms and the
    variant table of the index-form runs equal the plane-form run's byte for byte, and the oracle's.  folded: the kernels with the
    Fisher epilogue, eight rounds deep; unfolded (JL_NO_FOLD_CALL=1): the plain ones, one round deep."""
    extra = dict(JL_NO_FOLD_CALL="1") if form == "unfolded" else {}
    assert "EDGES-OK " + form in run_child("edges", **extra)


def test_form_by_counting_form():
    """Two groups of three windows.  Launches from the index that are collected before the next are folded, every one; then ten
    rounds of group A and group B back to back without collecting: every result equals the single runs' and the oracle's whatever
    form was taken, the counts by (form, counting form) add up launch by launch, and at least one launch from the index found the
    other group's launch incomplete and went unfolded — where a launch from the planes, with its threshold of three, would have
    folded.  No sleeps, nothing timed."""
    out = run_child("forms")
    print(out)      # (the four counts of the back-to-back rounds)
    assert "FORMS-OK" in out
