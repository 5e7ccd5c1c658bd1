"""The boundary fixtures of tests/stereo_boundary_fixtures.py on the CPU: the Python restatements of the two stereo
matchers equal the C oracle on every case, and for every named decision ("Matcher decisions") the
restatement with that one decision flipped leaves the oracle on every case that claims to sit on it."""
import numpy as np
import pytest

from tests import oracle_calls as oc
from tests import pyref_stereo as ps
from tests import stereo_boundary_fixtures as sb
from tests.test_stereo_fisheye import run_oracle as run_fisheye_oracle

CASES = sb.CASES

# Literal on purpose: a decision that loses its flip or its fixture shows up here in review.
DECISIONS = (
    "rows.radius", "rows.radius:one", "rows.span", "rows.span:exclusive", "rows.clip", "stereo.row",
    "stereo.window", "stereo.window:max", "stereo.level", "stereo.level:narrow", "stereo.high", "stereo.tie",
    "stereo.accept",
    "sad.round", "sad.level", "sad.bound", "sad.inside", "sad.inside:bottom", "sad.inside:bottom_r",
    "sad.inside:right", "sad.inside:strip", "sad.first", "sad.edge", "sad.edge:hi",
    "disp.min", "disp.min:open", "disp.max", "disp.clamp",
    "median.index", "median.cut",
    "fish.second", "fish.ratio", "fish.two", "fish.mono", "fish.mono:right", "fish.octave", "fish.last",
)
# the families of each matcher: a stereo decision is pinned by stereo cases, a fisheye decision by fish cases
KIND = {"rows": "stereo", "stereo": "stereo", "sad": "stereo", "disp": "stereo", "median": "stereo", "fish": "fish"}


def run_oracle(oracle, case):
    """stereo: (mvuRight, mvDepth, kept); fish: (mvLeftToRightMatch, mvRightToLeftMatch, nMatches, rows with a depth)."""
    if case.kind == "stereo":
        return oc.stereo(oracle, case.frame)
    l2r, r2l, depth, p3d, n = run_fisheye_oracle(oracle, case.frame)
    assert np.array_equal(depth != -1, l2r >= 0) and np.array_equal(depth[l2r >= 0], p3d[l2r >= 0, 2])
    return l2r, r2l, n, depth != -1


def run_pyref(case, flip=None):
    if case.kind == "stereo":
        return ps.compute_stereo_matches(case.frame, flip=flip)
    return ps.compute_stereo_fisheye_matches(case.frame, flip=flip)


def same(a, b):
    """Bit for bit: the floats by their patterns."""
    def bits(v):
        v = np.asarray(v)
        return v.view(np.int32) if v.dtype == np.float32 else v
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_every_flip_is_listed():
    assert set(DECISIONS) == set(ps.FLIPS) and len(DECISIONS) == len(set(DECISIONS))
    assert {f for c in CASES for f in c.flips} == set(DECISIONS)


def test_the_cases_stay_small():
    """At most 64 keypoints a side and 64 x 96 pixels, but for the cases named after the structure they straddle:
    130 keypoints on one row, the two heights either side of 1024 rows."""
    for c in CASES:
        size = sb.sizes(c)
        assert size[0] <= (130 if c.structure else 64), c.id
        if c.kind == "stereo":
            assert len(c.frame.scale) <= 3 and size[2] <= 96 and (size[1] <= 64 or c.name in ("rows_1024", "rows_1025")), c.id


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_python_equals_oracle(oracle, case):
    ref, got = run_oracle(oracle, case), run_pyref(case)
    assert same(ref, got), (ref, got)


@pytest.mark.parametrize("name", DECISIONS)
def test_flip_leaves_the_oracle(oracle, name):
    cases = [c for c in CASES if name in c.flips]
    assert cases and {c.kind for c in cases} == {KIND[name.split(".")[0]]}
    for case in cases:
        assert not same(run_oracle(oracle, case), run_pyref(case, flip=name)), \
            f"{case.id}: flip {name} ({ps.FLIPS[name]}) gives the oracle's result"


def test_hand_cases(oracle):
    """The two hand cases that tests/test_stereo.py asserts in words are cases here."""
    by = {c.name: c for c in CASES}
    sb.check_hand([run_oracle(oracle, by["hand_median_zero"]), run_oracle(oracle, by["hand_clamp"])])


def test_every_structural_case_matches_something(oracle):
    """A structural case that matched nothing would pass a kernel that does nothing."""
    for c in CASES:
        if c.structure and c.kind == "stereo":
            ur, _, n = run_oracle(oracle, c)
            assert n == c.frame.n and (ur >= 0).all(), c.id
    fish = [c for c in sb.of_kind("fish") if c.structure]
    assert sum(run_oracle(oracle, c)[2] for c in fish) >= 8


def test_ratio_in_float_is_the_ratio_in_double():
    """d0 < d1 * 0.7 as float times double and as a float product agree on every pair of distances 0 .. 256, so
    fish.ratio has no float variant ("Matcher decisions")."""
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    double = d0.astype(np.float32).astype(np.float64) < d1.astype(np.float32).astype(np.float64) * 0.7
    single = d0.astype(np.float32) < d1.astype(np.float32) * np.float32(0.7)
    assert np.array_equal(double, single)


def test_clamp_in_float_is_the_clamp_in_double():
    """bestuR = uL - 0.01 in double and in float round to the same float for every float32 uL in [1, 128): within a
    binade uL - 0.01 sits at one fixed offset from the float grid, so disp.clamp has no float variant."""
    lo, hi = np.float32(1).view(np.int32), np.float32(128).view(np.int32)
    for a in range(int(lo), int(hi), 1 << 22):
        u = np.arange(a, min(a + (1 << 22), int(hi)), dtype=np.int32).view(np.float32)
        assert np.array_equal((u.astype(np.float64) - 0.01).astype(np.float32), u - np.float32(0.01))
