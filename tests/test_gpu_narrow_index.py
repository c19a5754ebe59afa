"""The deviation index with 16-bit stored entries (csrc/deviation_index.h: the three codes, no read number): a lane's round of the
list walk is one 8-byte load of four entries, two to a dword, and a list begins on 8 bytes against its neighbour's end.

Windows of 12 to 36 columns at the smallest shapes at which that walk can go wrong (tests/narrow_index_child.py):

  * adjacent     lists of 0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1 and 0 entries in adjacent chunks: a list that ends inside a dword or an
                 8-byte load lies against padding slots and its neighbour's first entry, which must never be counted;
  * round edge   1023 / 1024 / 1025 entries at 8192 reads (chunk bound 1152);
  * batch edges  2047 / 2048 / 2049 entries at 15 360 reads (bound 2160): the unfolded kernels hold 2 rounds; 16 383 / 16 384 /
                 16 385 at 116 000 reads (bound 16 416): the folded kernels hold 16;
  * every code   about a tenth of 8192 reads carry a code drawn from 0..6 (bases, gap, N, uncovered) in every column of a chunk.

Each is run alone three times and in a group of two windows three more: the index-form runs (run 3, launch 3) equal the window's
own plane-form run bit for bit, and the oracle: column counts, codon histograms, the variant table.  jl_msa_index_info's entries
and indexed chunks are what was planted, and its bytes are exactly half of what the 4-byte entry took.  folded: the kernels with
the Fisher epilogue; unfolded: JL_NO_FOLD_CALL=1.  Which form a group launch took is read from the -DJL_TUNING build, as
test_gpu_index_forms.py does.  The format on the host: test_narrow_entry_host.py.  Runs only on a real MI355X: `pytest -m gpu`.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUNING_LIB = os.path.join(ROOT, "tools_tuning", "lib_exp", "libjuliet_hip.so")


@pytest.mark.parametrize("form", ["folded", "unfolded"])
def test_narrow_entries_at_the_walks_edges(form):
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: tools_tuning/build_tuning_lib.sh (build() runs it)"
    env = dict(os.environ, JL_LIB=TUNING_LIB)
    env.pop("JL_NO_GRAPH", None)
    env.pop("JL_NO_FOLD_CALL", None)
    if form == "unfolded":
        env["JL_NO_FOLD_CALL"] = "1"
    out = subprocess.run([sys.executable, os.path.join(HERE, "narrow_index_child.py")], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "NARROW-OK " + form in out.stdout
