"""The stored form of a deviation-index entry (csrc/deviation_index.h): 16 bits that carry the three codes and nothing of the read
number, two to a dword as the counting kernel decodes them, the allocation in bytes and the flush bounds at every walk depth the
kernels use, through a stand-alone C++ program (tests/cpp/narrow_entry_check.cpp) built with the host sanitizers.  The kernels on
them: test_gpu_narrow_index.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_narrow_entry_on_the_host(tmp_path):
    exe = str(tmp_path / "narrow_entry_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "narrow_entry_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.startswith("ok ")
