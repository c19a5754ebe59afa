"""The host front end of the read-against-haplotype calls (csrc/hap_stage.h: the rescue, the nearest-haplotype call, the
recombinant call), through a stand-alone C++ program (tests/cpp/hap_stage_check.cpp) built with the host sanitizers: the packed
pattern against a numpy packing, forward and reversed, and every refusal with the status and the text the calls had when each
carried its own copy of the checks.  The calls themselves: test_gpu_rescue.py, test_gpu_nearest.py, test_gpu_recombinant.py."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ARG, STATE = -1, -4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hap_stage") / "hap_stage_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "cpp", "hap_stage_check.cpp")])
    return out


def numpy_pat4(pattern, n_pos, n_hap):
    """byte q of dword [g][h] = pattern[h][4 g + q], 0 where either does not exist"""
    hap_pad, groups = (n_hap + 63) // 64 * 64, (n_pos + 3) // 4
    padded = np.zeros((hap_pad, 4 * groups), dtype=np.uint8)
    padded[:n_hap, :n_pos] = pattern[:, :n_pos]
    return np.ascontiguousarray(padded.reshape(hap_pad, groups, 4).transpose(1, 0, 2)).view("<u4").reshape(groups, hap_pad)


@pytest.mark.parametrize("n_hap", [1, 64, 65, 702])
@pytest.mark.parametrize("n_pos", [1, 3, 4, 5, 64, 65])
def test_pack_pat4_against_numpy(exe, tmp_path, n_pos, n_hap):
    rng = np.random.default_rng(1000 * n_pos + n_hap)
    for stride in (n_pos, n_pos + 3):        # a row of its own length, and pattern_stride > n_pos: the bytes between rows are not read
        pattern = rng.integers(0, 64, size=(n_hap, stride), dtype=np.uint8)
        pattern[:, n_pos:] = 0xFF
        pattern.tofile(str(tmp_path / "in"))
        for reversed_ in (0, 1):
            r = subprocess.run([exe, "pack", str(n_pos), str(n_hap), str(stride), str(reversed_), str(tmp_path / "in"), str(tmp_path / "out")],
                               capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
            hap_pad, groups = (n_hap + 63) // 64 * 64, (n_pos + 3) // 4
            assert [int(x) for x in r.stdout.split()] == [hap_pad, groups, groups * hap_pad, n_pos + groups * hap_pad]
            got = np.fromfile(str(tmp_path / "out"), dtype="<u4")
            assert got.size == n_pos + groups * hap_pad
            cols = 7 + 10 * np.arange(n_pos, dtype=np.uint32)
            rows = pattern[:, :n_pos]
            if reversed_:
                cols, rows = cols[::-1], rows[:, ::-1]
            assert (got[:n_pos] == cols).all()
            pat4 = got[n_pos:].reshape(groups, hap_pad)
            assert (pat4 == numpy_pat4(rows, n_pos, n_hap)).all()
            # padding: the lanes h >= n_hap, and the positions past n_pos in the last group
            assert not pat4[:, n_hap:].any()
            if n_pos % 4:
                assert not (pat4[-1] >> (8 * (n_pos % 4))).any()


# name -> (status, text): the texts of capi_rescue.hip, capi_nearest.hip, capi_recomb.hip, capi_link.hip and
# capi_class_codons.hip before the checks moved to hap_stage.h, byte for byte; a case that is wrong twice pins the order
REFUSALS = {
    "passes": (0, ""),
    "no_matrix_first": (STATE, "jl_phase_rescue_async: no resident matrix"),
    "no_positions": (ARG, "jl_phase_rescue_async: no positions array"),
    "no_pattern": (ARG, "jl_phase_rescue_async: no pattern array"),
    "zero_positions": (ARG, "jl_phase_rescue_async: 0 positions, 1 to 4096"),
    "too_many_positions": (ARG, "jl_phase_rescue_async: 4097 positions, 1 to 4096"),
    "zero_haplotypes": (ARG, "jl_phase_rescue_async: 0 haplotypes, 1 to 702"),
    "too_many_haplotypes": (ARG, "jl_phase_rescue_async: 703 haplotypes, 1 to 702"),
    "short_stride": (ARG, "jl_phase_rescue_async: pattern_stride 3 below the 4 positions of a row"),
    "zero_min_positions": (ARG, "jl_phase_rescue_async: min_positions 0, 1 to the 4 positions"),
    "min_positions_above": (ARG, "jl_phase_rescue_async: min_positions 5, 1 to the 4 positions"),
    "codon_beyond_window": (ARG, "jl_phase_rescue_async: position 3: the codon at column 98 ends beyond the window's 100 columns"),
    "not_ascending": (ARG, "jl_phase_rescue_async: position 2: columns not strictly ascending"),
    "beyond_before_ascending": (ARG, "jl_phase_rescue_async: position 1: the codon at column 98 ends beyond the window's 100 columns"),
    "no_codon": (ARG, "jl_phase_rescue_async: pattern byte 64 of haplotype 1 at position 2 is no codon (0..63)"),
    "stride_padding_is_not_read": (0, ""),
    "shape_passes": (0, ""),
    "shape_positions": (ARG, "jl_haplotype_recombinants: 0 positions, 1 to 4096"),
    "shape_haplotypes": (ARG, "jl_haplotype_recombinants: 703 haplotypes, 1 to 702"),
    "shape_stride": (ARG, "jl_haplotype_recombinants: pattern_stride 3 below the 4 positions of a row"),
    "columns_last_codon_fits": (0, ""),
    "columns_beyond": (ARG, "jl_variant_linkage_async: position 0: the codon at column 98 ends beyond the window's 100 columns"),
    "columns_equal": (ARG, "jl_class_codons_async: position 1: columns not strictly ascending"),
}


def test_refusals_keep_status_text_and_order(exe):
    r = subprocess.run([exe, "refuse"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = {}
    for line in r.stdout.splitlines():
        name, status, text = line.split("\t")
        got[name] = (int(status), text)
    assert got == REFUSALS
