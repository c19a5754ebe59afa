"""The conditions that keep tests/test_gpu_stage_sequences.py from passing vacuously, checked from the mirrors alone: no GPU, no
library.  The device module calls the same function before its first test."""
import numpy as np

import stage_sequences as ss


def test_expected_values_are_not_vacuous():
    cases = ss.check_not_vacuous()
    assert set(cases) == {"A", "A2", "B", "C"}


def test_matrices_and_parameters_are_seeded():
    """Made twice, the same: the device tests and this file see one set of rows, parameters and expected values."""
    for name, (n, l, seed) in ss.SHAPES.items():
        rows, haps = ss.mixture(n, l, seed)
        c = ss.case(name)
        assert (rows == c.rows).all() and (haps == c.haps).all()
        assert len(np.unique(rows)) == 7                      # every code, the ragged ends' 6 among them
        for setting in c.settings:
            again = ss.parameters(rows, setting, seed, haps)
            for key, value in c.prm[setting].items():
                assert np.array_equal(again[key], value), (name, setting, key)


def test_large_setting_needs_its_columns():
    """C holds three codon starts: it takes the small setting only, and the sequences use it there."""
    assert len(ss.codon_starts(9)) == 3 and len(ss.codon_starts(66)) == len(ss.codon_starts(130)) == 22
    for l in (66, 130):
        assert int(ss.codon_starts(l)[-1]) + 2 < l
    assert ss.case("C").settings == (ss.SMALL,)
