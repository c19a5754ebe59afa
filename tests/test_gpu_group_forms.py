"""The two forms of a group run (capi_group.hip): the Fisher stage in the pileup launch's epilogue (folded) or as
call_group_kernel behind the plain pileup (unfolded), chosen per launch from what else is in flight on the device.

Both forms must give, for every window, exactly what jl_run_async gives on that window alone and what the oracle gives.
Which form a launch took is read from a counter of the -DJL_TUNING build of the library (tools_tuning/build_tuning_lib.sh,
built by build()); a process loads one library, so the scenarios run in child processes (tests/group_forms_child.py).
Runs only on a real MI355X: `pytest -m gpu`.
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
    out = subprocess.run([sys.executable, os.path.join(HERE, "group_forms_child.py"), scenario], env=env, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("form", ["folded", "unfolded"])
def test_each_form_equals_single_runs_and_oracle(form):
    """Groups of 1, 3 and 8 windows, phasing on and off, one window without any variant, one group with per-window DRM
    masks: variant table, haplotypes, per-read ids and summary of every window against jl_run_async on that window alone
    (bit for bit) and against the oracle.  Each launch is collected before the next, so nothing else is in flight and the
    library folds; JL_NO_FOLD_CALL=1 makes every launch unfolded.  The child checks the form counter too."""
    extra = dict(JL_EXPECT_FORM=form)
    if form == "unfolded":
        extra["JL_NO_FOLD_CALL"] = "1"
    assert "FORMS-OK " + form in run_child("forms", **extra)


def test_form_switch_between_launches():
    """Five groups of different reads launched back to back without collecting (later launches see earlier ones
    incomplete), collected in launch order, then the same five again one at a time (each sees nothing in flight), three
    rounds: every result as above, and the library's own count shows that both forms were taken.  No sleeps, nothing timed."""
    assert "SWITCH-OK" in run_child("switch")


def test_timing_hook_leaves_the_run_alone():
    """jl_group_time_pileup times the plain grouped pileup kernel and has no side effect: after it, jl_group_views, the
    run views and jl_call_fetch + jl_phase_fetch of every window still return the run's results (against single runs and
    the oracle), and the device's run counters — n_occupied, the overflow bits jl_phase_rerun_ids_separate looks at, the
    summary — are byte for byte what the run left (read through the tuning build's jl_tuning_ctx_meta)."""
    assert "HOOK-OK" in run_child("hook")
