"""The boundary fixtures of tests/matcher_boundary_fixtures.py on the CPU: the Python restatement equals the C
oracle on every case, and for every named decision ("Matcher decisions") the restatement with that
one decision flipped leaves the oracle on every case that claims to sit on it."""
import pytest

from tests import matcher_boundary_fixtures as mb
from tests import pyref_match as pr

# Literal on purpose: a decision that loses its flip or its fixture shows up here in review.
DECISIONS = (
    "area.window", "area.order", "area.clamp",
    "fuse.level", "fuse.level:narrow", "fuse.chi2_mono", "fuse.chi2_stereo", "fuse.chi2_stereo:kpr", "fuse.tie",
    "fuse.accept", "fuse.right_index",
    "sim3.accept", "sim3.accept:double", "sim3.taken", "sim3.taken:never", "sim3.tie", "sim3.level",
    "sim3.level:narrow",
    "bysim3.accept", "bysim3.mutual",
    "tri.tie", "tri.accept", "tri.epipole", "tri.epipole:always", "tri.epipolar", "tri.filters", "tri.filters:mp1",
    "tri.filters:stereo1", "tri.filters:stereo2", "tri.filters:coarse",
    "rot.round", "rot.round:wrap", "maxima.order", "maxima.tenth",
    "init.level0", "init.level0:f2", "init.md", "init.top2", "init.accept", "init.accept:ratio", "init.steal_hist",
)
# where each shared decision has to be pinned: the area walk under every matcher that walks it, the histogram
# under both matchers that keep one
KINDS = {"area": ("fuse", "sim3", "bysim3"), "rot": ("tri", "init"), "maxima": ("tri", "init")}


def test_every_flip_is_listed():
    assert set(DECISIONS) == set(pr.FLIPS) and len(DECISIONS) == len(set(DECISIONS))
    assert {f for c in mb.CASES for f in c.flips} == set(DECISIONS)


@pytest.mark.parametrize("case", mb.CASES, ids=lambda c: c.id)
def test_python_equals_oracle(oracle, case):
    assert max(case.args[0].n, case.args[1].n) <= 64
    for mode in mb.modes(case):
        ref, got = mb.run_oracle(oracle, case, mode), mb.run_pyref(case, mode)
        assert mb.same(ref, got), (mode, ref, got)


@pytest.mark.parametrize("name", DECISIONS)
def test_flip_leaves_the_oracle(oracle, name):
    cases = [c for c in mb.CASES if name in c.flips]
    family = name.split(".")[0]
    assert {c.kind for c in cases} == set(KINDS.get(family, (family,)))
    for case in cases:
        differs = [mode for mode in mb.modes(case)
                   if not mb.same(mb.run_oracle(oracle, case, mode), mb.run_pyref(case, mode, flip=name))]
        assert differs, f"{case.id}: flip {name} ({pr.FLIPS[name]}) gives the oracle's result in every mode"


def test_the_pile_up_leaves_a_case_its_decisions(oracle):
    """pile_up adds histogram entries of its own; the cases still equal the oracle with it (the GPU test runs
    them through k_init's serial walk this way)."""
    for case in mb.of_kind("init"):
        piled = mb.pile_up(case)
        assert mb.same(mb.run_oracle(oracle, piled, None), mb.run_pyref(piled, None))
