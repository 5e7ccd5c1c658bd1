"""GPU: the bits of PoseOptimization, PoseInertialOptimization, the IMU preintegration (with the host functions
osg_imu_delta and osg_imu_predict_state), OptimizeEssentialGraph and OptimizeEssentialGraph4DoF, against
tests/golden/optimizer_digests.json.

These modules share the small dense routines of csrc/small_linalg.h and csrc/so3_common.h (LDL^T, cyclic Jacobi, the
3 x 3 products, the SO(3) functions).  Their tolerance tests compare with numpy restatements and cannot see a shared
routine move by an ulp; this one can: tools/ransac_digests.py's ``optimizer`` table makes one call per module through
the public Python API and hashes every result field of every problem (SHA-256 of the raw bytes, scalars at their ABI
width); the golden file holds what the commit named in its header produced.  The kernels use no atomics on floats and
sum in a fixed order, so the bits are the same on every run.

A pull request that changes these kernels' arithmetic on purpose regenerates the file with
``tools/ransac_digests.py --table optimizer`` and says so; any other difference is a defect of the change.
"""
import json

import pytest

from tools import ransac_digests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(ctx):
    return ransac_digests.optimizer_digests(ctx)


@pytest.fixture(scope="module")
def want():
    with open(ransac_digests.GOLDEN_OPTIMIZER) as f:
        gold = json.load(f)
    assert gold["recorded_at_commit"] and gold["rocm_version"]
    return gold["digests"]


@pytest.mark.parametrize("module", ["pose", "poseinertial", "preintegration", "essgraph", "essgraph4dof"])
def test_every_field_of_every_problem_has_the_recorded_bits(got, want, module):
    assert sorted(got[module]) == sorted(want[module])
    differ = []
    for name, fields in want[module].items():
        assert sorted(got[module][name]) == sorted(fields), name
        differ += [(name, f) for f, sha in fields.items() if got[module][name][f] != sha]
    assert not differ, differ
