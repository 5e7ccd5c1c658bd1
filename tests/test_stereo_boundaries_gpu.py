"""stereo.hip's three kernels and triang.hip's k_stereo_fisheye on the boundary fixtures of
tests/stereo_boundary_fixtures.py (tests/test_stereo_boundaries.py proves on the CPU that each sits on its
decisions), bit for bit against the oracle (the floats by their bit patterns), on every form in which a frame
reaches the kernels:

* every stereo case through ComputeStereoMatches with host pyramids; with both pyramids on the device (read in
  place); with bordered host levels (row step != cols, repacked by the host);
* a batch of three whose middle frame has no left keypoint, and a batch that holds the case twice (the frames share
  one row buffer and one grid sized by the largest);
* every fisheye case through ComputeStereoFishEyeMatches;
* the row limit of k_stereo_rows: 8192 rows run, 8193 are refused."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import OsgError
from orb_slam3_comments_ghr_amd import stereo as st
from tests import oracle_calls as oc
from tests import stereo_boundary_fixtures as sb
from tests.test_stereo_fisheye import run_oracle as run_fisheye_oracle

pytestmark = pytest.mark.gpu

STEREO = sb.of_kind("stereo")
FISH = sb.of_kind("fish")


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's answer for a case, computed once."""
    made = {}

    def get(case):
        if case.id not in made:
            made[case.id] = (oc.stereo if case.kind == "stereo" else run_fisheye_oracle)(oracle, case.frame)
        return made[case.id]
    return get


def check(got, want, what):
    for g, w, field in zip(got[:2], want[:2], ("mvuRight", "mvDepth")):
        np.testing.assert_array_equal(np.asarray(g).view(np.int32), np.asarray(w).view(np.int32),
                                      err_msg=f"{what}: {field}")
    assert int(got[2]) == int(want[2]), f"{what}: kept {got[2]} != {want[2]}"


@pytest.mark.parametrize("case", STEREO, ids=lambda c: c.id)
def test_stereo_case_host_pyramids(ctx, ref, case):
    check(st.ComputeStereoMatches(ctx, case.frame), ref(case), case.id)


@pytest.mark.parametrize("case", STEREO, ids=lambda c: c.id)
def test_stereo_case_device_pyramids(ctx, ref, case):
    check(st.ComputeStereoMatches(ctx, case.frame.to_device()), ref(case), f"{case.id} on the device")


@pytest.mark.parametrize("case", STEREO, ids=lambda c: c.id)
def test_stereo_case_bordered_levels(ctx, ref, case):
    F = sb.bordered(case.frame)
    assert all(lv.strides[0] > lv.shape[1] for lv in F.left.levels + F.right.levels)
    check(st.ComputeStereoMatches(ctx, F), ref(case), f"{case.id} bordered")


@pytest.mark.parametrize("case", STEREO, ids=lambda c: c.id)
def test_stereo_case_in_batches(ctx, ref, case):
    F, want = case.frame, ref(case)
    outs, nm = st.ComputeStereoMatchesBatch(ctx, [F, sb.without_left(F), F])
    assert nm[1] == 0 and outs[1][0].size == 0
    for b in (0, 2):
        check((*outs[b], nm[b]), want, f"{case.id}: frame {b} of three")
    outs, nm = st.ComputeStereoMatchesBatch(ctx, [F, F])
    for b in (0, 1):
        check((*outs[b], nm[b]), want, f"{case.id}: frame {b} of two")


@pytest.mark.parametrize("case", FISH, ids=lambda c: c.id)
def test_fisheye_case(ctx, ref, case):
    got, want = st.ComputeStereoFishEyeMatches(ctx, case.frame), ref(case)
    assert got[4] == want[4], f"{case.id}: nMatches {got[4]} != {want[4]}"
    for g, w, field in zip(got[:4], want[:4], ("mvLeftToRightMatch", "mvRightToLeftMatch", "mvDepth",
                                               "mvStereo3Dpoints")):
        np.testing.assert_array_equal(g.view(np.int32), w.view(np.int32), err_msg=f"{case.id}: {field}")


def test_row_limit(ctx, oracle):
    """k_stereo_rows counts the rows of level 0 in LDS: an image of 8192 rows (eight rows per scan segment) runs
    and equals the oracle, one of 8193 is refused before anything is launched."""
    F = sb.tall_frame(8192)
    want = oc.stereo(oracle, F)
    assert want[2] == 3
    check(st.ComputeStereoMatches(ctx, F), want, "8192 rows")
    with pytest.raises(OsgError, match="invalid argument.*8193 image rows"):
        st.ComputeStereoMatches(ctx, sb.tall_frame(8193))
    check(st.ComputeStereoMatches(ctx, F), want, "8192 rows after the refusal")
