"""LocalMapping::CreateNewMapPoints through the ORB-SLAM3-side adapter (adapters/orbslam3/osg_orbslam3.h:
NewPointsGather, create_new_map_points; the body of adapters/orbslam3/LocalMapping_osg.cc) on the mock KeyFrames
of tests/adapter/mock_orbslam3.h and mock_localmapping.h, driven by tests/adapter/newpoints_driver.cpp.

* CPU: the gather on a mock KeyFrame set equals a Python restatement exactly: the neighbour list with the inertial
  mPrevKF append (ref:src/LocalMapping.cc:531-552), the keypoint choice by NLeft, mvKeys for UnprojectStereo, the
  poses and cameras, median_depth, ratioFactor.
* GPU: after the adapter's CreateNewMapPoints the mock map holds pyref's MapPoints in pyref's order, with the same
  observations and KeyFrame slots (a KF2 slot overwritten by a second point included), positions within the
  fixture group's tolerance, one ComputeDistinctiveDescriptors and one UpdateNormalAndDepth per point, the same
  mlpRecentAddedMapPoints order; and only neighbour 0 processed when the mock's CheckNewKeyFrames is true.
"""
import os
import subprocess

import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import _abi
from tests import newpoints_fixtures as FX
from tests import pyref_newpoints as R
from tools.adapter_arrays import read_arrays, write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "adapter", "newpoints_driver.cpp")
PKG = os.path.join(ROOT, "orb_slam3_comments_ghr_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("newpoints") / "newpoints_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-result", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), DRIVER_SRC, "-o", exe, "-L" + PKG, "-lorbslam3_amd",
                        "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(driver, tmp_path, mode, arrays):
    fi, fo = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
    write_arrays(fi, arrays)
    r = subprocess.run([driver, mode, fi, fo], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return read_arrays(fo)


def raw(struct):
    return np.frombuffer(bytes(struct), np.uint8).copy()


def geometry_bytes(g):
    s = g.struct()
    s.depth = s.keys_x = s.keys_y = None
    return raw(s)


def kf_arrays(pre, K, g, pair_geometry, scene_depths):
    """A KeyFrame for build_triang_kf ("desc", "kp_*", ...) plus what mock_localmapping.h adds."""
    a = {"desc": K.desc.reshape(-1), "nleft": np.array([K.nleft], np.int32), "two_cam": np.array([K.two_cam], np.int32),
         "kp_x": K.kp_x, "kp_y": K.kp_y, "kp_angle": K.kp_angle, "kp_octave": K.kp_octave, "has_mp": K.has_mp,
         "scale": K.scale, "level_sigma2": K.level_sigma2, "node_id": K.node_id.astype(np.int32),
         "node_start": K.node_start, "feat": K.feat, "geometry": geometry_bytes(g),
         "pair_geometry": raw(pair_geometry), "scene_depths": np.asarray(scene_depths, np.float32)}
    if K.u_right is not None:
        a.update(u_right=K.u_right, depth=g.depth, keys_x=g.keys_x, keys_y=g.keys_y)
    return {pre + k: v for k, v in a.items()}


def world(P, covisible=None, prev=None, new_keyframes=False):
    """The array file of a NewPointsProblem: K0 the current KeyFrame, K1.. its neighbours in P's order.  A
    neighbour's scene depths are chosen so that their (size - 1) / 2 element is P's median_depth."""
    B = P.n_neigh
    a = {"params": np.array([B + 1, P.monocular, P.inertial, P.far_points, new_keyframes, P.coarse], np.int32),
         "th_far": np.array([P.th_far_points], np.float32),
         "covisible": np.asarray(covisible if covisible is not None else np.arange(1, B + 1), np.int32),
         "prev": np.asarray(prev if prev is not None else np.full(B + 1, -1), np.int32)}
    a.update(kf_arrays("K0.", P.kf1, P.g1, _abi.OsgTriangGeom(), [1.0]))
    for b in range(B):
        m = np.float32(P.g2[b].median_depth)
        a.update(kf_arrays("K%d." % (b + 1), P.kf2[b], P.g2[b], P.geom[b].struct(), [m + 2, m / 2, m, m + 1]))
    return a


def neighbour_list(n_cov, prev, nn, inertial):
    """ref:src/LocalMapping.cc:531-552 on the indices of the array file"""
    v = list(n_cov[:nn])
    if inertial:
        k, count = 0, 0
        while len(v) <= nn and prev[k] >= 0 and count < nn:
            count += 1
            if prev[k] not in v:
                v.append(int(prev[k]))
            k = int(prev[k])
    return v


@pytest.mark.parametrize("name", ["claim3", "stereo10", "rig4", "inertial"])
def test_gather_equals_the_restatement(driver, tmp_path, name):
    P = FX.build(name)
    B = P.n_neigh
    # the covisibility list holds the first B - 1 neighbours; the last one is reached through mPrevKF, behind a
    # KeyFrame that is in the list already (skipped by std::find)
    cov, prev = np.arange(1, B + 1), np.full(B + 1, -1)
    if P.inertial:
        cov = np.arange(1, B)
        prev[0], prev[1], prev[B] = 1, B, -1
    a = world(P, cov, prev)
    out = run(driver, tmp_path, "gather", a)
    want = neighbour_list(list(cov), prev, 30 if P.monocular else 10, P.inertial)
    assert out["neighbours"].tolist() == want == list(range(1, B + 1))
    assert out["flags"].tolist() == [B, int(P.monocular), int(P.inertial), int(P.coarse), int(P.far_points)]
    assert out["floats"].tobytes() == np.array([P.th_far_points, np.float32(1.5) * P.kf1.scale[1]], np.float32).tobytes()
    for k, (K, g) in enumerate([(P.kf1, P.g1)] + list(zip(P.kf2, P.g2))):
        pre = "S%d." % k
        stereo = K.u_right is not None and not K.two_cam
        assert out[pre + "head"].tolist() == [K.n, K.nleft, K.two_cam, len(K.scale), int(K.u_right is not None), int(stereo)]
        for f in ("kp_x", "kp_y", "kp_octave", "has_mp"):   # mvKeysUn, or mvKeys / mvKeysRight by NLeft
            assert out[pre + f].tobytes() == getattr(K, f).tobytes(), (k, f)
        assert out[pre + "desc"].tobytes() == K.desc.tobytes()
        if stereo:
            for f in ("depth", "keys_x", "keys_y"):        # mvDepth, mvKeys (not mvKeysUn)
                assert out[pre + f].tobytes() == getattr(g, f).tobytes(), (k, f)
            assert out[pre + "u_right"].tobytes() == K.u_right.tobytes()
            assert not np.array_equal(g.keys_x, K.kp_x)
        exp = g.struct()
        exp.depth = exp.keys_x = exp.keys_y = None
        if not (k > 0 and P.monocular):
            exp.median_depth = 0.0   # ComputeSceneMedianDepth is only called for a monocular neighbour
        assert out[pre + "geometry"].tobytes() == bytes(exp), k   # poses, centres, mRwc / mTwc, cameras, scalars
        if k > 0:
            assert out[pre + "pair_geometry"].tobytes() == bytes(P.geom[k - 1].struct())


def test_neighbour_list_restatement():
    assert neighbour_list([1, 2, 3], [-1] * 4, 10, False) == [1, 2, 3]
    assert neighbour_list(list(range(1, 13)), [-1] * 13, 10, False) == list(range(1, 11))
    assert neighbour_list([1, 2], [3, -1, -1, 2, -1], 10, True) == [1, 2, 3]   # 3 appended, then 2 found, chain ends


def expected_map(P, ref):
    pts = ref.created()
    slots = [np.full(K.n, -1, np.int32) for K in [P.kf1] + list(P.kf2)]
    for k, K in enumerate([P.kf1] + list(P.kf2)):
        slots[k][K.has_mp != 0] = -2
    for j, (b, i1, i2) in enumerate(pts):
        slots[0][i1] = j
        slots[b + 1][i2] = j   # a second point on the same KF2 keypoint overwrites the slot
    return pts, slots


@pytest.mark.gpu
@pytest.mark.parametrize("name,new_keyframes", [("claim3", False), ("claim3", True), ("stereo10", False), ("rig4", False)])
def test_adapter_leaves_pyrefs_map(driver, tmp_path, name, new_keyframes):
    P = FX.build(name)
    ref = R.run(P, first_only=True) if new_keyframes else FX.reference(name)
    out = run(driver, tmp_path, "run", world(P, new_keyframes=new_keyframes))
    pts, slots = expected_map(P, ref)
    bl = FX.borderline(name)
    assert not bl or name not in FX.HAND_MADE
    got = out["points"].reshape(-1, 7)
    print(name, "points", len(got), "want", len(pts), "CheckNewKeyFrames calls", int(out["rc"][1]))
    if not bl:
        assert out["rc"][0] == len(pts) and out["rc"][1] == 1
        assert [(int(k) - 1, int(i1), int(i2)) for k, i1, i2 in got[:, :3]] == pts
        assert np.all(got[:, 3] == 1) and np.all(got[:, 4] == 1)    # one ComputeDistinctiveDescriptors / UpdateNormalAndDepth
        assert np.all(got[:, 5] == 2) and np.all(got[:, 6] == 1)    # two observations, the current KeyFrame first
        n = len(pts)
        assert out["recent"].tolist() == list(range(n)) and out["atlas"].tolist() == list(range(n))
        for k in range(P.n_neigh + 1):
            assert out["slots%d" % k].tolist() == slots[k].tolist(), k
        tol = FX.tolerances(name)["x3d"]
        worst = max((FX.x3d_rel(P, ref, b, i1, x) for (b, i1, _), x in zip(pts, out["x3d"].reshape(-1, 3))), default=0.0)
        print(name, "largest x3D difference", worst, "tolerance", tol)
        assert worst <= tol
    if new_keyframes:
        assert set(got[:, 0].tolist()) == {1}   # only neighbour 0
    if name == "claim3" and not new_keyframes:
        # two points on one KF2 keypoint: the slot holds the later one, both keep their observation
        b, i2 = [(b, i2) for j, (b, _, i2) in enumerate(pts) if [(q[0], q[2]) for q in pts].count((b, i2)) > 1][0]
        ids = [j for j, q in enumerate(pts) if (q[0], q[2]) == (b, i2)]
        assert len(ids) == 2 and out["slots%d" % (b + 1)][i2] == ids[1]
