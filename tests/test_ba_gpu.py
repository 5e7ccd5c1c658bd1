"""GPU parity: PoseOptimization (batched) and LocalBundleAdjustment through the C ABI against the
CPU oracle.

PoseOptimization (pinhole mono + stereo) is bit-exact: the kernel sums every chi2 /
H / b stream in edge order and both sides evaluate sin / cos / pow(., 3) correctly rounded
(csrc/exact_math.h), so LM iteration and trial counts, outlier flags and the pose are asserted
EQUAL, for every waves-per-frame variant of the kernel (OSG_POSE_NW pins it).  KannalaBrandt8
fisheye frames too: the projection's float atan2f is glibc's algorithm restated bit for bit
(csrc/glibc_math.h, pinned against the host libm by tests/test_exact_math.py), and its double
cos / sin / atan2 are correctly rounded on both sides.

LocalBundleAdjustment: integer outcomes (edge classification) identical; LM trial counts may
differ by a few: once converged, a step changes chi2 by less than FP64 rounding of the sum
(|d chi2| ~ 1e-13 chi2), so the sign of rho — accept or reject — depends on summation order.  A
different accept/reject there changes lambda for the following steps, so the final states of two
correct implementations differ at the size of the last LM steps (measured: <= 3e-8 on these
problems, against 1-px measurement noise that leaves ~1e-3 m of uncertainty), and in rare cases
the iteration at which LM terminates moves by one.  Required: iteration counts within 1, chi2
within 1e-9 relative, states within 1e-6."""
import json
import os

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import optimizer as op
from tests import oracle_calls as oc

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-6      # LBA poses and points (metres / unit quaternion)
CHI2_RTOL = 1e-9
# Observed margins inside those tolerances, one JSON line per checked graph, so a
# drift that stays inside 1e-6 still shows round to round: OSG_BA_MARGINS names the file
# (default gpurun_out/ba_margins.jsonl under the repository root)
MARGINS = os.environ.get("OSG_BA_MARGINS", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "gpurun_out", "ba_margins.jsonl"))


def record_margins(kind, G, got, ref):
    rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "kind": kind,
           "n_poses": int(len(G.pose)), "n_points": int(len(G.point)), "n_edges": int(len(G.e_point)),
           "iterations": [int(got.iterations), int(ref.iterations)], "trials": [int(got.trials), int(ref.trials)],
           "d_iterations": int(got.iterations - ref.iterations), "d_trials": int(got.trials - ref.trials),
           "max_abs_d_pose": float(np.max(np.abs(got.pose - ref.pose))) if got.pose.size else 0.0,
           "max_abs_d_point": float(np.max(np.abs(got.point - ref.point))) if got.point.size else 0.0,
           "chi2_final_rel": float(abs(got.chi2_final - ref.chi2_final) / max(abs(ref.chi2_final), 1e-300)),
           "chi2_initial_rel": float(abs(got.chi2_initial - ref.chi2_initial) / max(abs(ref.chi2_initial), 1e-300))}
    try:
        os.makedirs(os.path.dirname(MARGINS), exist_ok=True)
        with open(MARGINS, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    return rec


def trials_close(a, b):
    return abs(a - b) <= max(2, int(0.1 * b))


def assert_pose_equal(got, ref):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.n_inliers == r.n_inliers, i
        assert g.lm_iterations == r.lm_iterations, (i, g.lm_iterations, r.lm_iterations)
        assert g.lm_trials == r.lm_trials, (i, g.lm_trials, r.lm_trials)
        np.testing.assert_array_equal(g.outlier, r.outlier)
        np.testing.assert_array_equal(g.pose, r.pose)


@pytest.mark.parametrize("nw", [None, "1", "2", "4", "8"])
def test_pose_optimization_batch(ctx, oracle, monkeypatch, nw):
    if nw is not None:
        monkeypatch.setenv("OSG_POSE_NW", nw)
    rng = np.random.default_rng(11)
    probs = [op.synth_pose_problem(rng, n_edges=int(rng.integers(30, 600)), stereo_frac=rng.uniform(0, 1))
             for _ in range(48)]
    ref = oc.pose(oracle, probs)
    got = op.Optimizer(ctx).PoseOptimization(probs)
    assert_pose_equal(got, ref)


@pytest.mark.parametrize("rowsum", ["0", "1"])
@pytest.mark.parametrize("nw", ["1", "8"])
def test_pose_optimization_rowsum_variants(ctx, oracle, monkeypatch, nw, rowsum):
    """The edge-order sums over whole zero-padded rows (default) and the per-chunk sums
    (OSG_POSE_ROWSUM=0): the same add chain, both bit-exact against the oracle, ragged last chunks."""
    monkeypatch.setenv("OSG_POSE_NW", nw)
    monkeypatch.setenv("OSG_POSE_ROWSUM", rowsum)
    rng = np.random.default_rng(16)
    probs = [op.synth_pose_problem(rng, n_edges=n, stereo_frac=0.4) for n in (3, 63, 64, 65, 191, 318, 513, 1100)]
    assert_pose_equal(op.Optimizer(ctx).PoseOptimization(probs), oc.pose(oracle, probs))
    for p in probs[-3:]:  # lone frames: the multi-wave layout the drop-in's one-frame call takes
        assert_pose_equal([op.Optimizer(ctx).PoseOptimization(p)], oc.pose(oracle, [p]))


@pytest.mark.parametrize("n_edges", [64, 65, 127, 129, 1000, 2500])
def test_pose_optimization_single_frame_sizes(ctx, oracle, n_edges):
    """The drop-in's one-frame call (multi-wave variant) across chunk boundaries and large frames."""
    rng = np.random.default_rng(n_edges)
    p = op.synth_pose_problem(rng, n_edges=n_edges, stereo_frac=0.5)
    assert_pose_equal([op.Optimizer(ctx).PoseOptimization(p)], oc.pose(oracle, [p]))


@pytest.mark.parametrize("nw", [None, "1", "8"])
def test_pose_optimization_kb8_fisheye(ctx, oracle, monkeypatch, nw):
    """KannalaBrandt8 camera (TUM-VI-like fisheye): project / projectJac with the host libm's float
    atan2f (restated, glibc_math.h) and correctly rounded cos / sin / atan2: bit-exact, like pinhole."""
    if nw is not None:
        monkeypatch.setenv("OSG_POSE_NW", nw)
    rng = np.random.default_rng(14)
    probs = [op.synth_pose_problem(rng, n_edges=int(rng.integers(30, 400)), cam=op.kb8_camera()) for _ in range(16)]
    ref = oc.pose(oracle, probs)
    got = op.Optimizer(ctx).PoseOptimization(probs)
    for i, r in enumerate(ref):
        assert r.n_inliers > 0.6 * len(probs[i].kind), "fisheye problems are well posed"
    assert_pose_equal(got, ref)


@pytest.mark.parametrize("nw", [None, "2"])
def test_pose_optimization_kb8_two_camera(ctx, oracle, monkeypatch, nw):
    """C5 shape: KB8 fisheye pair with right-camera (body) edges through Trl; bit-exact."""
    if nw is not None:
        monkeypatch.setenv("OSG_POSE_NW", nw)
    rng = np.random.default_rng(15)
    probs = [op.synth_pose_problem(rng, n_edges=int(rng.integers(60, 400)), cam=op.kb8_camera(), body_frac=0.4)
             for _ in range(16)]
    ref = oc.pose(oracle, probs)
    got = op.Optimizer(ctx).PoseOptimization(probs)
    for i in range(len(probs)):
        assert (probs[i].kind == 2).any()
    assert_pose_equal(got, ref)


def test_pose_optimization_small_and_degenerate(ctx, oracle):
    rng = np.random.default_rng(12)
    probs = [op.synth_pose_problem(rng, n_edges=n) for n in (0, 1, 2, 3, 5, 9, 10, 11)]
    ref = oc.pose(oracle, probs)
    got = op.Optimizer(ctx).PoseOptimization(probs)
    assert_pose_equal(got, ref)
    for g, p in zip(got, probs):
        if p.n < 3:
            assert g.n_inliers == 0 and np.array_equal(g.pose, p.pose)


def test_pose_optimization_all_outliers(ctx, oracle):
    """Every edge a gross outlier: later rounds have no active edge (g2o returns immediately)."""
    rng = np.random.default_rng(13)
    p = op.synth_pose_problem(rng, n_edges=50, outlier_frac=1.0)
    assert_pose_equal([op.Optimizer(ctx).PoseOptimization(p)], oc.pose(oracle, [p]))


def check_lba(ctx, oracle, G, exact=False):
    """exact: SURVEY §8(c)'s bar for the well-conditioned C4 windows (LM runs without rejected steps):
    the same iteration and trial counts, states within 1e-7."""
    ref = oc.lba(oracle, G)
    got = op.Optimizer(ctx).LocalBundleAdjustment(G)
    record_margins("lba_exact" if exact else "lba", G, got, ref)
    if exact:
        assert (got.iterations, got.trials) == (ref.iterations, ref.trials)
        np.testing.assert_allclose(got.pose, ref.pose, atol=1e-7, rtol=0)
        np.testing.assert_allclose(got.point, ref.point, atol=1e-7, rtol=0)
    assert abs(got.iterations - ref.iterations) <= 1
    assert trials_close(got.trials, ref.trials), (got.trials, ref.trials)
    assert abs(got.chi2_initial - ref.chi2_initial) <= CHI2_RTOL * ref.chi2_initial
    assert abs(got.chi2_final - ref.chi2_final) <= CHI2_RTOL * ref.chi2_final
    np.testing.assert_allclose(got.pose, ref.pose, atol=STATE_TOL, rtol=0)
    np.testing.assert_allclose(got.point, ref.point, atol=STATE_TOL, rtol=0)
    np.testing.assert_array_equal(got.edge_bad, ref.edge_bad)
    return got, ref


@pytest.mark.parametrize("n_kf,n_pts,stereo", [(5, 300, 0.0), (10, 1000, 0.0), (20, 2500, 0.3), (12, 800, 1.0)])
def test_lba_parity(ctx, oracle, n_kf, n_pts, stereo):
    rng = np.random.default_rng(n_kf * 100 + n_pts)
    G = op.synth_lba_graph(rng, n_kf=n_kf, n_points=n_pts, stereo_frac=stereo)
    got, ref = check_lba(ctx, oracle, G)
    assert got.chi2_final < got.chi2_initial


def test_lba_user_lambda_and_stop_flag(ctx, oracle):
    rng = np.random.default_rng(9)
    G = op.synth_lba_graph(rng, n_kf=8, n_points=600)
    G.user_lambda_init = 100.0  # inertial maps: setUserLambdaInit(100)
    check_lba(ctx, oracle, G)
    stop = np.ones(1, np.uint8)  # the reference's bool *pbStopFlag
    r = op.Optimizer(ctx).LocalBundleAdjustment(G, stop_flag=stop)
    assert r.aborted == 1 and r.iterations == 0
    np.testing.assert_array_equal(r.pose, G.pose)


def test_lba_all_fixed_poses(ctx, oracle):
    rng = np.random.default_rng(10)
    G = op.synth_lba_graph(rng, n_kf=6, n_points=400)
    G.pose_fixed[:] = 1
    check_lba(ctx, oracle, G)


def test_lba_c4_full_size(ctx, oracle):
    """C4: 50 KF x 10k points (~5e4 edges)."""
    rng = np.random.default_rng(0x0B5EED04)
    G = op.synth_lba_graph(rng, n_kf=50, n_points=10000)
    got, ref = check_lba(ctx, oracle, G, exact=True)
    assert got.iterations >= 1


def _rig_graph(rng, n_kf, n_pts, body_frac=0.5, kb8=False):
    """An LBA window of a two-camera rig (LocalBundleAdjustment's EdgeSE3ProjectXYZToBody, ref:src/
    Optimizer.cc:2009-2032): body_frac of the left (mono) observations get a right-camera edge on the same
    (KeyFrame, MapPoint), so those Hessian blocks carry two edges (k_linearize<true>; the compact factor
    sums their M).  The right observation is the current estimate seen through Trl plus 1 px of noise;
    with kb8 both cameras are KannalaBrandt8 and the left observations are re-projected through it."""
    from orb_slam3_comments_ghr_amd import _abi
    G = op.synth_lba_graph(rng, n_kf=n_kf, n_points=n_pts)
    cam1 = op.kb8_camera() if kb8 else G.cams[0]
    cam2 = (op.kb8_camera if kb8 else op.pinhole_camera)(trl=op.TUMVI_TRL)
    R = np.array([op.quat_to_rot(q[:4]) for q in G.pose])
    Xl = np.einsum("eij,ej->ei", R[G.e_pose], G.point[G.e_point]) + G.pose[G.e_pose, 4:]

    def proj(cam, X):
        if kb8:
            return np.stack(op.kb8_project(cam, X), 1)
        return np.stack([cam.fx * X[:, 0] / X[:, 2] + cam.cx, cam.fy * X[:, 1] / X[:, 2] + cam.cy], 1)
    obs = G.e_obs.copy()
    mono = G.e_kind == _abi.EDGE_MONO
    if kb8:
        obs[mono, :2] = proj(cam1, Xl[mono]) + rng.normal(size=(int(mono.sum()), 2))
    add = np.nonzero(mono & (rng.random(len(G.e_point)) < body_frac))[0]
    Rrl, trl = op.quat_to_rot(np.array(op.TUMVI_TRL[:4])), np.array(op.TUMVI_TRL[4:])
    Xr = Xl[add] @ Rrl.T + trl
    obs_r = np.zeros((len(add), 3))
    obs_r[:, :2] = proj(cam2, Xr) + rng.normal(size=(len(add), 2))
    return op.BAGraph(G.pose, G.pose_fixed, G.point,
                      np.concatenate([G.e_point, G.e_point[add]]), np.concatenate([G.e_pose, G.e_pose[add]]),
                      np.concatenate([G.e_kind, np.full(len(add), _abi.EDGE_BODY, np.int8)]),
                      np.concatenate([G.e_cam, np.ones(len(add), np.int32)]),
                      np.concatenate([obs, obs_r]).astype(np.float32).astype(np.float64),
                      np.concatenate([G.e_inv_sigma2, G.e_inv_sigma2[add]]), [cam1, cam2])


@pytest.mark.parametrize("n_kf,n_pts,kb8", [(8, 600, False), (20, 2500, False), (12, 1200, True)])
def test_lba_two_camera_rig(ctx, oracle, n_kf, n_pts, kb8):
    """Two-camera rig windows (left mono + right body edges on the same blocks, pinhole and KB8) against
    the oracle: the blocks with several edges, in either Hessian-block form."""
    rng = np.random.default_rng(4242 + n_kf)
    G = _rig_graph(rng, n_kf, n_pts, kb8=kb8)
    pairs = G.e_pose.astype(np.int64) * (len(G.point) + 1) + G.e_point
    assert len(np.unique(pairs)) < len(pairs)  # some blocks carry two edges
    check_lba(ctx, oracle, G)


def test_lba_batch_equals_single_calls(ctx, oracle):
    """Lockstep batch of heterogeneous windows: every graph's result equals its own single call
    exactly (same kernels, per-graph deterministic reductions) and the oracle within tolerance."""
    rng = np.random.default_rng(31)
    graphs = [op.synth_lba_graph(rng, n_kf=int(k), n_points=int(p), stereo_frac=s)
              for k, p, s in [(5, 300, 0.0), (12, 900, 0.3), (8, 600, 1.0), (20, 2000, 0.0), (6, 400, 0.0)]]
    graphs[2].user_lambda_init = 100.0
    graphs[4].pose_fixed[:] = 1
    opt = op.Optimizer(ctx)
    batch = opt.LocalBundleAdjustmentBatch(graphs)
    for i, (G, got) in enumerate(zip(graphs, batch)):
        single = opt.LocalBundleAdjustment(G)
        assert (got.iterations, got.trials) == (single.iterations, single.trials), i
        assert got.chi2_initial == single.chi2_initial and got.chi2_final == single.chi2_final, i
        np.testing.assert_array_equal(got.pose, single.pose)
        np.testing.assert_array_equal(got.point, single.point)
        np.testing.assert_array_equal(got.edge_bad, single.edge_bad)
        ref = oc.lba(oracle, G)
        assert abs(got.iterations - ref.iterations) <= 1
        np.testing.assert_allclose(got.pose, ref.pose, atol=STATE_TOL, rtol=0)
        np.testing.assert_array_equal(got.edge_bad, ref.edge_bad)


def _lba_batch_graphs():
    rng = np.random.default_rng(0x0B5EED04 + 11)
    graphs = [op.synth_lba_graph(rng, n_kf=50, n_points=10000) for _ in range(3)]
    graphs += [op.synth_lba_graph(rng, n_kf=int(k), n_points=int(p), stereo_frac=s)
               for k, p, s in [(5, 300, 0.0), (12, 900, 0.3), (20, 2000, 1.0)]]
    return graphs


def _gba_variant_graph():
    rng = np.random.default_rng(3000 + 30)
    return op.synth_gba_graph(rng, n_kf=30, n_points=3000, bRobust=False, stereo_frac=0.3)


def _env_map_graphs():
    """Reduced systems past CMAX (n = 894) with narrow envelopes: a 150-KF open map and one closed into a
    loop (at most 7 envelope row blocks below a column block)."""
    return [op.synth_map_graph(np.random.default_rng(71), n_kf=150, n_points=12000, loop=False),
            op.synth_map_graph(np.random.default_rng(72), n_kf=150, n_points=12000, loop=True)]


def _ba_child(env, maps=False):
    """LocalBundleAdjustmentBatch of _lba_batch_graphs, then BundleAdjustment of _gba_variant_graph (or, with
    maps, of each of _env_map_graphs) in a child process under `env` (the kernel knobs are read once per
    process)."""
    import subprocess
    import sys
    out = f"/tmp/_osg_ba_child_{os.getpid()}_{abs(hash(tuple(sorted(env.items()))))}.npz"
    code = ("import numpy as np\n"
            "from orb_slam3_comments_ghr_amd import Context, optimizer as op\n"
            "from tests.test_ba_gpu import _lba_batch_graphs, _gba_variant_graph, _env_map_graphs\n"
            "o = op.Optimizer(Context(0))\n"
            f"gba = {'_env_map_graphs()' if maps else '[_gba_variant_graph()]'}\n"
            "res = o.LocalBundleAdjustmentBatch(_lba_batch_graphs()) + [o.BundleAdjustment(G) for G in gba]\n"
            f"np.savez('{out}', **{{f'p{{i}}': r.pose for i, r in enumerate(res)}},\n"
            "         **{f'q{i}': r.point for i, r in enumerate(res)},\n"
            "         it=np.array([[r.iterations, r.trials] for r in res]),\n"
            "         chi=np.array([[r.chi2_initial, r.chi2_final] for r in res]))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(np.load(out))
    os.remove(out)
    return got


def test_lba_compact_factor_vs_whole_hpl(ctx):
    """The compact per-block factor (the default: M = P^T rho' W P per block, Hpl = S(Xc)^T M R rebuilt by
    its readers) against the whole-Hpl form (OSG_LBA_HPL=1): the same Hessian in another rounding, so
    identical iteration / trial counts, chi2 and states equal to rounding, on the LBA batch (mono, stereo,
    and the 5- to 50-KF windows) and the bRobust = false GBA graph."""
    o = op.Optimizer(ctx)
    res = o.LocalBundleAdjustmentBatch(_lba_batch_graphs()) + [o.BundleAdjustment(_gba_variant_graph())]
    full = _ba_child({"OSG_LBA_HPL": "1"})
    np.testing.assert_array_equal(full["it"], [[r.iterations, r.trials] for r in res])
    np.testing.assert_allclose(full["chi"], [[r.chi2_initial, r.chi2_final] for r in res], rtol=1e-12, atol=0)
    for i, r in enumerate(res):
        np.testing.assert_allclose(full[f"p{i}"], r.pose, atol=1e-9, rtol=0)
        np.testing.assert_allclose(full[f"q{i}"], r.point, atol=1e-9, rtol=0)


def test_lba_chol_fused_vs_column_launches(ctx):
    """The one-workgroup factorisation k_chol_dense (LocalBundleAdjustment windows, the default) against the
    per-column k_chol_col launches (OSG_CHOL_DENSE=0): the same blocked LL^T with its sums in another order,
    so identical iteration / trial counts and states equal to rounding.  The maps past CMAX take the column
    launches (k_chol_col + k_chol_trail, k_chol_back_large) in both processes: bit-identical."""
    o = op.Optimizer(ctx)
    lba = o.LocalBundleAdjustmentBatch(_lba_batch_graphs())
    maps = [o.BundleAdjustment(G) for G in _env_map_graphs()]
    col = _ba_child({"OSG_CHOL_DENSE": "0"}, maps=True)
    np.testing.assert_array_equal(col["it"], [[r.iterations, r.trials] for r in lba + maps])
    np.testing.assert_allclose(col["chi"][:len(lba)], [[r.chi2_initial, r.chi2_final] for r in lba], rtol=1e-12, atol=0)
    for i, r in enumerate(lba):
        np.testing.assert_allclose(col[f"p{i}"], r.pose, atol=1e-9, rtol=0)
        np.testing.assert_allclose(col[f"q{i}"], r.point, atol=1e-9, rtol=0)
    for i, r in enumerate(maps, start=len(lba)):
        np.testing.assert_array_equal(col["chi"][i], [r.chi2_initial, r.chi2_final])
        np.testing.assert_array_equal(col[f"p{i}"], r.pose)
        np.testing.assert_array_equal(col[f"q{i}"], r.point)


def test_lba_batch_c4_windows(ctx, oracle):
    """8 C4-sized windows (50 KF x 10k points) in one batch against the oracle."""
    rng = np.random.default_rng(0x0B5EED04 + 7)
    graphs = [op.synth_lba_graph(rng, n_kf=50, n_points=10000) for _ in range(8)]
    got = op.Optimizer(ctx).LocalBundleAdjustmentBatch(graphs)
    for G, g in zip(graphs, got):
        ref = oc.lba(oracle, G)
        record_margins("lba_batch_c4", G, g, ref)
        assert (g.iterations, g.trials) == (ref.iterations, ref.trials)
        np.testing.assert_allclose(g.pose, ref.pose, atol=1e-7, rtol=0)
        np.testing.assert_allclose(g.point, ref.point, atol=1e-7, rtol=0)
        np.testing.assert_array_equal(g.edge_bad, ref.edge_bad)


def check_gba(ctx, oracle, G):
    ref = oc.lba(oracle, G)
    got = op.Optimizer(ctx).BundleAdjustment(G)
    record_margins("gba", G, got, ref)
    assert abs(got.iterations - ref.iterations) <= 1
    assert trials_close(got.trials, ref.trials), (got.trials, ref.trials)
    assert abs(got.chi2_initial - ref.chi2_initial) <= CHI2_RTOL * ref.chi2_initial
    assert abs(got.chi2_final - ref.chi2_final) <= CHI2_RTOL * ref.chi2_final
    np.testing.assert_allclose(got.pose, ref.pose, atol=STATE_TOL, rtol=0)
    np.testing.assert_allclose(got.point, ref.point, atol=STATE_TOL, rtol=0)
    return got, ref


@pytest.mark.parametrize("n_kf,n_pts,robust,stereo", [(12, 1000, False, 0.0), (30, 3000, True, 0.3),
                                                      (80, 8000, False, 0.0), (150, 12000, False, 0.2)])
def test_gba_parity(ctx, oracle, n_kf, n_pts, robust, stereo):
    """Optimizer::BundleAdjustment: 80 and 150 keyframes put the reduced system (474 / 894) past the
    LocalBA size, through the chunked column updates and k_chol_back_large."""
    rng = np.random.default_rng(3000 + n_kf)
    G = op.synth_gba_graph(rng, n_kf=n_kf, n_points=n_pts, bRobust=robust, stereo_frac=stereo)
    got, ref = check_gba(ctx, oracle, G)
    assert got.chi2_final < got.chi2_initial and got.iterations >= 1


@pytest.mark.parametrize("n_kf,n_pts", [(400, 40000), (1500, 150000)])
def test_gba_map_scale(ctx, oracle, n_kf, n_pts):
    """BundleAdjustment at map scale (ref:src/Optimizer.cc:2850-3237, LinearSolverEigen): keyframes
    along a 0.45 km open path sharing points with their neighbours, so the reduced camera system is a
    band.  400 keyframes (n = 2394) run the envelope-aware right-looking factorisation and the LDS
    back-substitution; 1500 keyframes x 150 k points (n = 8994, 600 k edges) are past the 1024 free
    KeyFrames the LDS back-substitution holds and take k_back_step.  Against the oracle (its LDL^T on
    the envelope) within §5's tolerances."""
    G = op.synth_map_graph(np.random.default_rng(4100 + n_kf), n_kf=n_kf, n_points=n_pts)
    got, ref = check_gba(ctx, oracle, G)
    assert got.chi2_final < 0.2 * got.chi2_initial and got.iterations >= 5


@pytest.mark.parametrize("n_kf,n_pts", [(400, 40000), (1500, 150000)])
def test_gba_map_loop_closed(ctx, oracle, n_kf, n_pts):
    """The global BA LoopClosing runs right after closing a loop (ref:src/LoopClosing.cc:2436 ->
    ref:src/Optimizer.cc:2831-2839): the map's path closed into a circle, so the last keyframes share
    points with the first ones and the reduced camera system is the band plus the corner blocks that
    join its ends.  The rows of the last keyframes reach column 0: the envelope factorisation runs them
    densely (k_chol_col / k_chol_trail over each column's envelope rows), k_schur_pairs writes only the
    pairs the factorisation reads.  Against the oracle's envelope LDL^T within §5's tolerances."""
    G = op.synth_map_graph(np.random.default_rng(4200 + n_kf), n_kf=n_kf, n_points=n_pts, loop=True)
    first = set(G.e_point[G.e_pose < 5].tolist())
    last = set(G.e_point[G.e_pose >= n_kf - 5].tolist())
    assert first & last, "the loop joins the first and the last keyframes"
    got, ref = check_gba(ctx, oracle, G)
    assert got.chi2_final < 0.2 * got.chi2_initial and got.iterations >= 5


def test_gba_loop_map_device_bytes_on_envelope():
    """The 1500-KF loop-closed map's reduced system lives on its envelope tiles (hs_at), not as the
    dense 8 994^2 matrix (647 MB): a fresh context's arena after one call stays under 0.5 GB."""
    from orb_slam3_comments_ghr_amd import Context
    G = op.synth_map_graph(np.random.default_rng(4200 + 1500), n_kf=1500, n_points=150000, loop=True)
    c = Context(0)
    try:
        r = op.Optimizer(c).BundleAdjustment(G)
        held = c.device_bytes()
    finally:
        c.close()
    assert r.iterations >= 5 and r.chi2_final < 0.2 * r.chi2_initial
    assert held <= 500e6, held


def test_gba_9000_kf_loop_map_accepted():
    """A 9 000-KeyFrame loop-closed map (n = 53 994, 3.6 M edges): past the old dense-matrix cap of 7 723
    free KeyFrames.  No oracle at this size (its envelope LDL^T takes minutes): the call must converge
    like the smaller maps, and the same map run twice gives the same result bit for bit."""
    from orb_slam3_comments_ghr_amd import Context
    G = op.synth_map_graph(np.random.default_rng(4900), n_kf=9000, n_points=900000, loop=True, vectorized=True)
    G.iterations = 5
    c = Context(0)
    try:
        opt = op.Optimizer(c)
        r = opt.BundleAdjustment(G)
        r2 = opt.BundleAdjustment(G)
        held = c.device_bytes()
    finally:
        c.close()
    assert r.iterations >= 3 and r.chi2_final < 0.5 * r.chi2_initial, (r.iterations, r.chi2_initial, r.chi2_final)
    assert np.isfinite(r.pose).all() and np.isfinite(r.point).all()
    assert (r.iterations, r.trials) == (r2.iterations, r2.trials)
    np.testing.assert_array_equal(r.pose, r2.pose)
    assert held < 8e9, held


def test_gba_and_lba_in_one_batch(ctx, oracle):
    """A LocalBA window and a whole-map BA in one lockstep batch: each equals its own call."""
    rng = np.random.default_rng(3300)
    graphs = [op.synth_lba_graph(rng, n_kf=20, n_points=2000), op.synth_gba_graph(rng, n_kf=90, n_points=6000)]
    opt = op.Optimizer(ctx)
    batch = opt.LocalBundleAdjustmentBatch(graphs)
    for G, b in zip(graphs, batch):
        s = opt.LocalBundleAdjustment(G)
        assert (b.iterations, b.trials) == (s.iterations, s.trials)
        np.testing.assert_array_equal(b.pose, s.pose)
        np.testing.assert_array_equal(b.point, s.point)
