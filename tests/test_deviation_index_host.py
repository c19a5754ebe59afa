"""The host half of the deviation index (csrc/deviation_index.h): entry encode / decode, the per-chunk and total bounds, and the
counting kernel's field-overflow bound, through a stand-alone C++ program (tests/cpp/deviation_index_check.cpp) built with the
host sanitizers.  The kernels on them: test_gpu_deviation_index.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_deviation_index_header_on_the_host(tmp_path):
    exe = str(tmp_path / "deviation_index_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "cpp", "deviation_index_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.startswith("ok ")
