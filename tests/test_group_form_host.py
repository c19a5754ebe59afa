"""The form of a group launch as a pure decision (csrc/group_form.h): folded or unfolded by the launches in flight, with a
threshold per counting form (planes 3, deviation index 1), and which other form is worth a captured graph — through a stand-alone
C++ program (tests/cpp/group_form_check.cpp) built with the host sanitizers.  The launches themselves: test_gpu_index_forms.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_group_form_decision_on_the_host(tmp_path):
    exe = str(tmp_path / "group_form_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "group_form_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.startswith("ok ")
