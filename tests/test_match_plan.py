"""CPU: osg_debug_match_plan, the host function that picks k_match's grid-staging level and dynamic
LDS size (run_batch applies it to every launch).  Properties over every frame size, and the threshold
sizes as hand-derived literals.

The layout (comment above match_lds_bytes in csrc/match.hip), for n keypoints and k grids (k = 2 on a
two-camera rig), with c16(n) = n rounded up to a multiple of 16 and GS_PAD = 64 * 48 + 1 rounded up to
a multiple of 4 = 3076 cell offsets (12304 bytes) per grid:
    R(n)     = 12 n + 2 c16(n)                        resolve arrays (level 0)
    L1(n, k) = R(n) + 12304 k + 16 n                  + grids and per-entry records (level 1)
    L2(n, k) = L1(n, k) rounded up to 16  + 32 n      + descriptors (level 2)
and a level fits when its bytes are at most lds_per_block - 8192."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import OsgError, match_plan

LDS = (65536, 163840)
MAX_SLOTS = 8192


def c16(n):
    return (n + 15) // 16 * 16


@pytest.fixture(scope="module")
def plans():
    """(stage, lds_bytes) arrays over n = 0..8192 for every (lds_per_block, two_cam, cap); -1 where the
    plan reports that the frame does not fit at all.  Computed once (54 k host calls, well under 1 s)."""
    out = {}
    for lds in LDS:
        for two in (False, True):
            for cap in (0, 1, 2):
                st = np.full(MAX_SLOTS + 1, -1, np.int64)
                by = np.full(MAX_SLOTS + 1, -1, np.int64)
                for n in range(MAX_SLOTS + 1):
                    try:
                        st[n], by[n] = match_plan(lds, cap, n, two)
                    except OsgError:
                        pass
                out[lds, two, cap] = (st, by)
    return out


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("cap", [0, 1, 2])
def test_plan_properties(plans, lds, two, cap):
    st, by = plans[lds, two, cap]
    fits = st >= 0
    # a frame that does not fit is followed by frames that do not fit; 160 KiB holds every size
    assert (np.diff(fits.astype(int)) <= 0).all()
    if lds == 163840:
        assert fits.all()
    n = np.nonzero(fits)[0]
    s, b = st[n], by[n]
    assert (np.diff(s) <= 0).all(), "the level never rises as n_slots grows"
    assert s.max() <= cap and s.min() >= 0
    assert s[0] == cap, "an empty frame takes the cap itself"
    # whatever launches fits the budget (level 0 included: its resolve arrays are dynamic LDS too)
    assert (b <= lds - 8192).all()
    resolve = 12 * n + 2 * np.array([c16(int(v)) for v in n])
    assert (b >= resolve).all()
    assert (b[s == 0] == resolve[s == 0]).all(), "level 0 takes the resolve arrays alone"
    # staging costs LDS: more than the resolve arrays, and level 2 more than level 1 would
    assert (b[s >= 1] >= resolve[s >= 1] + 12304 * (2 if two else 1) + 16 * n[s >= 1]).all()
    assert (b[s == 2] >= resolve[s == 2] + 12304 * (2 if two else 1) + 48 * n[s == 2]).all()
    # the descriptors of a level-2 launch start on a 16-byte boundary and end the block
    assert ((b[s == 2] - 32 * n[s == 2]) % 16 == 0).all()


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("cap", [0, 1, 2])
def test_two_cameras_never_stage_higher(plans, lds, cap):
    one, two = plans[lds, False, cap][0], plans[lds, True, cap][0]
    assert (two <= one).all()


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("two", [False, True])
def test_cap_only_lowers(plans, lds, two):
    """A cap changes nothing below itself: min(uncapped level, cap), and the same bytes when equal."""
    s2, b2 = plans[lds, two, 2]
    for cap in (0, 1):
        s, b = plans[lds, two, cap]
        assert (s == np.minimum(s2, cap)).all()
        assert (b[s == s2] == b2[s == s2]).all()


# Largest n at level 2 and at level 1, and the bytes there (budget: 163840 - 8192 = 155648 and
# 65536 - 8192 = 57344):
#  160 KiB, one camera
#    L2(2311, 1) = 64708 + 4640 + 12304 = 81652 -> 81664, + 73952 = 155616 fits
#    L2(2312, 1) = 64736 + 4640 + 12304 = 81680,          + 73984 = 155664 does not
#    L1(4777, 1) = 133756 + 9568 + 12304 = 155628 fits;  L1(4778, 1) = 133784 + 9568 + 12304 = 155656 not
#  160 KiB, two cameras
#    L2(2113, 2) = 59164 + 4256 + 24608 = 88028 -> 88032, + 67616 = 155648 fits exactly
#    L2(2114, 2) = 59192 + 4256 + 24608 = 88056 -> 88064, + 67648 = 155712 does not
#    L1(4368, 2) = 122304 + 8736 + 24608 = 155648 fits exactly;  L1(4369, 2) = 122332 + 8768 + 24608 = 155708 not
#  64 KiB, one camera
#    L2(726, 1) = 20328 + 1472 + 12304 = 34104 -> 34112, + 23232 = 57344 fits exactly
#    L2(727, 1) = 20356 + 1472 + 12304 = 34132 -> 34144, + 23264 = 57408 does not
#    L1(1501, 1) = 42028 + 3008 + 12304 = 57340 fits;  L1(1502, 1) = 42056 + 3008 + 12304 = 57368 not
#  64 KiB, two cameras
#    L2(528, 2) = 14784 + 1056 + 24608 = 40448, + 16896 = 57344 fits exactly
#    L2(529, 2) = 14812 + 1088 + 24608 = 40508 -> 40512, + 16928 = 57440 does not
#    L1(1090, 2) = 30520 + 2208 + 24608 = 57336 fits;  L1(1091, 2) = 30548 + 2208 + 24608 = 57364 not
# (first term 28 n = 12 n + 16 n, second 2 c16(n), third the grids.)
KNOWN = [
    # lds_per_block, two_cam, last n at level 2, bytes there, last n at level 1, bytes there
    (163840, False, 2311, 155616, 4777, 155628),
    (163840, True, 2113, 155648, 4368, 155648),
    (65536, False, 726, 57344, 1501, 57340),
    (65536, True, 528, 57344, 1090, 57336),
]


@pytest.mark.parametrize("lds,two,n2,b2,n1,b1", KNOWN)
def test_known_thresholds(lds, two, n2, b2, n1, b1):
    assert match_plan(lds, 2, n2, two) == (2, b2)
    assert match_plan(lds, 2, n2 + 1, two)[0] == 1
    assert match_plan(lds, 2, n1, two) == (1, b1)
    assert match_plan(lds, 1, n1, two) == (1, b1)
    # 160 KiB: past level 1 every size up to 8192 launches at level 0 with
    # R(8192) = 98304 + 16384 = 114688 bytes
    if lds == 163840:
        r = 12 * (n1 + 1) + 2 * c16(n1 + 1)
        assert match_plan(lds, 2, n1 + 1, two) == (0, r)
        assert match_plan(lds, 2, 8192, two) == (0, 114688)


def test_known_level0_limit_at_64k():
    """R(4096) = 49152 + 8192 = 57344 is the budget of a 64 KiB device exactly; R(4097) = 49164 +
    8224 = 57388 is past it, and such a frame is refused instead of launched."""
    for two in (False, True):
        assert match_plan(65536, 2, 4096, two) == (0, 57344)
        with pytest.raises(OsgError, match="unsupported"):
            match_plan(65536, 2, 4097, two)


def test_plan_rejects_bad_arguments():
    for n in (-1, 8193):
        with pytest.raises(OsgError, match="invalid"):
            match_plan(163840, 2, n, False)
    # caps outside [0, 2] clamp, as the environment variable's value does
    assert match_plan(163840, 7, 100, False) == match_plan(163840, 2, 100, False)
    assert match_plan(163840, -3, 100, False) == match_plan(163840, 0, 100, False)
