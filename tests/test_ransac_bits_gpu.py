"""GPU: the bits of osg_sim3_ransac_batch, osg_mlpnp_ransac_batch, osg_two_view_reconstruct_batch and
osg_optimize_sim3_batch on their BATCH fixture lists, against tests/golden/ransac_digests.json.

The tolerance tests of these modules compare with numpy restatements that use another eigen-solver, so they
cannot see one copy of a shared routine drift from another by an ulp.  This one can: tools/ransac_digests.py
makes one batched call per module, every optional per-hypothesis array requested, and hashes every result
field of every fixture (SHA-256 of the raw bytes, scalars at their ABI width); the golden file holds what the
commit named in its header produced.  The kernels use no atomics on floats and no in-launch hand-off, so the
bits are the same on every run.

A pull request that changes these kernels' arithmetic on purpose regenerates the file with
tools/ransac_digests.py and says so; any other difference is a defect of the change.
"""
import json

import pytest

from tools import ransac_digests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(ctx):
    return ransac_digests.digests(ctx)


@pytest.fixture(scope="module")
def want():
    with open(ransac_digests.GOLDEN) as f:
        gold = json.load(f)
    assert gold["recorded_at_commit"] and gold["rocm_version"]
    return gold["digests"]


@pytest.mark.parametrize("module", ["sim3ransac", "mlpnp", "twoview", "sim3opt"])
def test_every_field_of_every_fixture_has_the_recorded_bits(got, want, module):
    assert sorted(got[module]) == sorted(want[module])
    differ = []
    for name, fields in want[module].items():
        assert sorted(got[module][name]) == sorted(fields), name
        differ += [(name, f) for f, sha in fields.items() if got[module][name][f] != sha]
    assert not differ, differ
