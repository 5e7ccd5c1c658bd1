"""GPU parity of the two-tiles-per-wave FP4 top-2 kernel (k_top2_fp4q2<16,256>, OSG_TOP2_MFMA_SHAPE=14):
bit-exact against the oracle's serial loop at the 32-, 64- and 1024-query boundaries (a wave's second tile
wholly inactive, holding one query, the second workgroup holding one query) and at the 32-row tile and
256-row chunk boundaries, three distinct frames per launch (frame and query-block indexing at nqb = 2).

The shape is read once per process, so one child process runs every problem under the variable and saves
the outputs; the tests compare them with the oracle.  The previous default, k_top2_fp4<16,1,256,3>, stays
reachable as OSG_TOP2_MFMA_SHAPE=3 and runs the same problems; with the variable unset the library plans and
launches the new kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import synth
from tests.test_top2_gpu import otop2

pytestmark = pytest.mark.gpu

NB = 3
# every nq edge with two nt values, every nt edge with two nq values
SHAPES = [(1, 1), (1, 257), (32, 33), (32, 288), (33, 31), (33, 513), (63, 32), (63, 257), (64, 255), (64, 513),
          (65, 256), (65, 33), (1023, 257), (1023, 32), (1024, 288), (1024, 1), (1025, 513), (1025, 31),
          (1057, 255), (1057, 256)]


def _frames(nq, nt):
    return [synth.descriptors_c2(nq, nt, seed=7000 + 100 * b + nq + 3 * nt) for b in range(NB)]


def _ties():
    """Exact duplicates of every query, shuffled across the tiles and chunks of 3000 rows, for 1100 queries
    (both workgroups, both tiles of a wave): the first of the equal rows wins."""
    rng = np.random.default_rng(14)
    q = rng.integers(0, 256, (1100, 32), dtype=np.uint8)
    t = np.concatenate([q, q, rng.integers(0, 256, (800, 32), dtype=np.uint8)])
    rng.shuffle(t, axis=0)
    return [(q, t), (q[::-1].copy(), t)]


def _all_256():
    """Every train row the complement of the one query descriptor: every distance is 256, nothing enters."""
    rng = np.random.default_rng(15)
    q = rng.integers(0, 256, (1, 32), dtype=np.uint8).repeat(70, 0)
    return [(q, np.repeat(~q[:1], 300, axis=0)), synth.descriptors_c2(70, 300, seed=16)]


def _past_nt(nt):
    """Frame 0's queries (an all-zero one among them, at distance 0 from a zero-filled row) have their exact
    copies only in the rows that follow frame 0's nt rows in memory (frame 1's first rows; as many as fit):
    a row past nt that took part would win with an index >= nt."""
    rng = np.random.default_rng(17 + nt)
    q0 = rng.integers(0, 256, (65, 32), dtype=np.uint8)
    q0[3] = 0
    t0 = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    t0[:, 0] |= 1   # no frame-0 row is all zero
    t1 = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    t1[:min(65, nt)] = q0[:min(65, nt)]
    return [(q0, t0), (rng.integers(0, 256, (65, 32), dtype=np.uint8), t1)]


def _problems():
    probs = {f"s{nq}_{nt}": _frames(nq, nt) for nq, nt in SHAPES}
    probs["ties"] = _ties()
    probs["all256"] = _all_256()
    probs["past40"] = _past_nt(40)
    probs["past257"] = _past_nt(257)
    return probs


_CHILD = ("import sys\n"
          "import numpy as np\n"
          "from orb_slam3_comments_ghr_amd import Context\n"
          "from tests.test_top2_gpu import _batch\n"
          "from tests.test_top2_q2_gpu import _problems\n"
          "ctx = Context(0)\n"
          "out = {}\n"
          "for name, fr in _problems().items():\n"
          "    if len(sys.argv) > 2 and name not in sys.argv[2:]:\n"
          "        continue\n"
          "    qs, ts = zip(*fr)\n"
          "    out[name] = _batch(ctx, qs, ts)\n"
          "    out['plan_' + name] = np.array(ctx.hamming_top2_batch_plan(qs[0].shape[0], ts[0].shape[0], len(qs)))\n"
          "np.savez(sys.argv[1], **out)\n")


def _run_child(path, shape, names=()):
    """Every problem (or those named) in a fresh process with OSG_TOP2_MFMA_SHAPE=shape (None: unset)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OSG_TOP2_FP4="1", OSG_TOP2_BATCH_MFMA="1")
    env.pop("OSG_TOP2_MFMA_SHAPE", None)
    if shape is not None:
        env["OSG_TOP2_MFMA_SHAPE"] = shape
    r = subprocess.run([sys.executable, "-c", _CHILD, path, *names], cwd=root, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.fixture(scope="module")
def q2_outputs(tmp_path_factory):
    return _run_child(str(tmp_path_factory.mktemp("q2") / f"q2_{os.getpid()}.npz"), "14")


@pytest.fixture(scope="module")
def shape3_outputs(tmp_path_factory):
    return _run_child(str(tmp_path_factory.mktemp("q2") / f"s3_{os.getpid()}.npz"), "3")


def _check(oracle, got, frames):
    assert got.shape == (len(frames), frames[0][0].shape[0], 3)
    for b, (q, t) in enumerate(frames):
        for k, ref in enumerate(otop2(oracle, q, t)):
            np.testing.assert_array_equal(got[b, :, k], ref, err_msg=f"frame {b} column {k}")


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_q2_equals_serial_loop(oracle, q2_outputs, nq, nt):
    name = f"s{nq}_{nt}"
    # the child really ran the new kernel, on ceil(nq / 1024) workgroups of 1024 threads per frame
    assert str(q2_outputs["plan_" + name]) == f"k_top2_fp4q2<16,256> grid={(nq + 1023) // 1024 * NB} x 1024"
    _check(oracle, q2_outputs[name], _frames(nq, nt))


def test_q2_ties_take_the_first_index(oracle, q2_outputs):
    frames = _ties()
    got = q2_outputs["ties"]
    _check(oracle, got, frames)
    q, t = frames[0]
    first = np.array([np.nonzero((t == row).all(axis=1))[0][0] for row in q[:50]])
    np.testing.assert_array_equal(got[0, :50, 0], first)
    assert (got[0, :, 1] == 0).all() and (got[0, :, 2] == 0).all()   # the duplicate is the second distance


def test_q2_all_distances_256(oracle, q2_outputs):
    got = q2_outputs["all256"]
    _check(oracle, got, _all_256())
    assert (got[0, :, 0] == -1).all() and (got[0, :, 1:] == 256).all()


@pytest.mark.parametrize("nt", [40, 257])
def test_q2_rows_past_nt_never_win(oracle, q2_outputs, nt):
    got = q2_outputs[f"past{nt}"]
    _check(oracle, got, _past_nt(nt))
    assert (got[0, :, 0] < nt).all() and (got[0, :, 1] > 0).all()
    assert (got[1, :, 1] >= 0).all()


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_shape3_is_the_previous_default(oracle, shape3_outputs, nq, nt):
    name = f"s{nq}_{nt}"
    assert str(shape3_outputs["plan_" + name]) == f"k_top2_fp4<16,1,256,3> grid={(nq + 511) // 512 * NB} x 1024"
    _check(oracle, shape3_outputs[name], _frames(nq, nt))


def test_shape3_ties_sentinels_and_rows_past_nt(oracle, shape3_outputs):
    for name, frames in [("ties", _ties()), ("all256", _all_256()), ("past40", _past_nt(40)),
                         ("past257", _past_nt(257))]:
        _check(oracle, shape3_outputs[name], frames)


def test_unset_shape_runs_the_q2_kernel(oracle, tmp_path):
    got = _run_child(str(tmp_path / f"d_{os.getpid()}.npz"), None, ("s1057_255", "s33_513"))
    assert str(got["plan_s1057_255"]) == f"k_top2_fp4q2<16,256> grid={2 * NB} x 1024"
    _check(oracle, got["s1057_255"], _frames(1057, 255))
    _check(oracle, got["s33_513"], _frames(33, 513))
