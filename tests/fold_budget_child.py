"""Child process of tests/test_gpu_fold_budget.py (not a test module: the form counter lives in the -DJL_TUNING build of the
library, and a process loads one library).

    python fold_budget_child.py         JL_LIB: the tuning build

Three 240-column windows of about 5 000 reads, one of them without any variant, as one group: three launches, each collected before
the next.  Launches 1 and 2 count from the planes, the indexes are built behind launch 2, launch 3 counts from the index — and every
launch is folded, nothing else being in flight (pileup_fold_group_kernel twice, pileup_index_fold_group_kernel once).  Every
launch's variant table (p_value and log_p bit for bit), haplotypes, per-read ids and summary against jl_run_async on a context of
its own that holds the same reads, and against the oracle.  Prints FOLD-BUDGET-OK as its last line.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle_lib  # noqa: E402
from group_forms_child import check_window, forms_taken, make_windows  # noqa: E402
from minorseq_amd import capi, msa  # noqa: E402


def main():
    lib = capi.load_library(os.environ["JL_LIB"])
    lib.jl_tuning_group_forms.restype = None
    orc = oracle_lib.load()
    l = 240
    genes = np.array([(1, l + 1)], dtype=capi.GENE)
    prm = capi.default_params()
    ref, wins = make_windows(3, l, 4100, n0=5000)
    exp, single = [], []
    for j, rows in wins:
        ev = orc.call(rows, genes, refseq=ref)
        exp.append((ev, orc.phase(rows, ev)))
        alone = capi.Juliet(0)      # the window alone: a context of its own, so that the group's windows are at run 1 below
        alone.upload_columns(msa.pack_columns(rows), len(rows))
        single.append(alone.run(genes, ref, prm, None, True))
        alone.close()
    assert len(exp[1][0]) == 0 and len(exp[0][0]) > 0 and len(exp[2][0]) > 0
    grp = capi.Group([j for j, _ in wins])
    assert forms_taken(lib) == (0, 0)
    for launch in (1, 2, 3):
        grp.run_async(genes, ref, prm, True, 10, True)
        for (j, _), (ev, ep), s in zip(wins, exp, single):
            check_window(j, ev, ep, s, True)
        infos = [j.index_info(wait=True) for j, _ in wins]
        assert [i["runs"] for i in infos] == [launch] * 3, infos
        assert [i["last_form"] for i in infos] == [1 if launch == 3 else 0] * 3, (launch, infos)
        if launch == 2:
            assert all(i["state"] == capi.INDEX_BUILT and i["indexed_chunks"] > 0 for i in infos), infos
        assert forms_taken(lib) == (launch, 0)
    grp.close()
    for j, _ in wins:
        j.close()
    print("FOLD-BUDGET-OK")


if __name__ == "__main__":
    main()
