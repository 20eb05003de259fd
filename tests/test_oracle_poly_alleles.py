"""CPU: the ploidy-4 oracle above 16 alleles per locus, pinned byte for byte in reference configuration to trajectories of the
REAL reference's sweeps (tests/golden/tw_*.golden, written by tests/golden/make_golden_alleles.py): both tetraploid variants,
loci of 17..24 alleles next to loci of 1..4."""
import os
import subprocess

import pytest

import golden_util as gu
import orc

import make_golden_alleles as mga

DUMP = os.path.join(orc.ORC_DIR, "orc_dump_poly")


@pytest.fixture(scope="module", autouse=True)
def _build():
    orc.build()


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_reference_configuration_is_byte_identical_above_16_alleles(name, tmp_path):
    out = str(tmp_path / (name + ".out"))
    allo = mga.CASES[name][-1]
    args = [DUMP] + mga.dump_args(name, os.path.join(gu.GOLDEN, name + ".txt"), out)[:14] + (["0", "0", "0", "1"] if allo else [])
    assert subprocess.call(args, timeout=600) == 0
    with open(out, "rb") as a, open(os.path.join(gu.GOLDEN, name + ".golden"), "rb") as g:
        assert a.read() == g.read()


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_fixture_data_has_the_listed_allele_counts(name):
    from instruct_amd import synth
    _, _, allelenum = synth.code_tetraploid(mga.data_for(name))
    assert tuple(allelenum) == mga.CASES[name][3]
    assert max(allelenum) > 16
