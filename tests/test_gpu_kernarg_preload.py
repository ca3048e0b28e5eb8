"""GPU: the mean kernels' leading plain parameters (kernel-argument preloading; cpi_mean_kernels.hpp: CPI_MEAN_LEAD_PARAMS,
CPI_TILED_LEAD_PARAMS) leave every output BIT-EQUAL to the library of the commit before the change -- dense, CSR first / count,
the stream entries (windows cut by a kernel of their own, cut in the mean kernel's prologue, many runs), the carry entry, the tiled
layout plain and SPLIT, knots 8 bytes behind a 2 MiB boundary, and knots beyond 2^32 bytes reached through `first`.  The cases and
the recorded digests: tests/kernarg_cases.py, tests/golden/kernarg_parent_sha256.json.  sha256 over raw bytes: no tolerance."""
import pytest

from tests import kernarg_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import cpi_amd
    return cpi_amd.Engine()


@pytest.fixture(scope="module")
def golden():
    return kc.load_golden()["groups"]


@pytest.mark.parametrize("gid", [g for g, _ in kc.groups()])
def test_outputs_bit_equal_to_the_parent_library(eng, golden, gid):
    got = dict(kc.groups())[gid](eng)
    want = golden[gid]
    assert set(got) == set(want), "the cases of %s differ from the recorded ones" % gid
    bad_inputs = sorted(k for k in got if k.endswith("inputs") and got[k] != want[k])
    assert not bad_inputs, "%s: the generated INPUTS differ from the recorded ones (%s): the generator drifted, not the kernels" % (gid, bad_inputs)
    assert not any(v.startswith("refused") for v in want.values()), "%s: a recorded case was refused by the library" % gid
    bad = sorted(k for k in got if got[k] != want[k])
    assert not bad, "%s: %d of %d outputs differ in their bytes from the parent library's: %s" % (gid, len(bad), len(got), bad[:12])
