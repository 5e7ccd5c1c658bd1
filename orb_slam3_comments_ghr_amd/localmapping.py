"""Host mirror of ``LocalMapping::CreateNewMapPoints`` (ref:src/LocalMapping.cc:526-934) on top of the C ABI
(``osg_create_new_map_points[_batch]``): the current KeyFrame against all its neighbours in one call.

    cnmp = CreateNewMapPoints(ctx)
    out = cnmp.run(problem)            # NewPointsOutput
    outs = cnmp.run([p0, p1, ...])     # independent current KeyFrames in the same launches

The MapPoints to create are ``out.created()``: (neighbour, KF1 index, KF2 index, x3D) in the reference's
creation order.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import Context, OsgError, _abi, load_library
from .frames import KFSide, TriangGeom, _c, _p

NP_CODES = ("none", "created", "low_parallax", "no_point", "z1", "z2", "reproj1", "reproj2", "zero_dist", "far",
            "scale")
# status codes after which x3d holds the point
NP_HAS_POINT = (_abi.NP_CREATED, _abi.NP_Z1, _abi.NP_Z2, _abi.NP_REPROJ1, _abi.NP_REPROJ2, _abi.NP_ZERO_DIST,
                _abi.NP_FAR, _abi.NP_SCALE)


@dataclass
class NpKeyFrame:
    """A KeyFrame's geometry as CreateNewMapPoints reads it (osg_np_kf); float32 values are the reference's own."""
    Tcw: np.ndarray                 # (3, 4): GetPose().matrix3x4()
    Ow: np.ndarray                  # (3,): GetCameraCenter()
    Rwc: np.ndarray                 # (3, 3): mRwc
    twc: np.ndarray                 # (3,): mTwc.translation()
    cam: np.ndarray                 # (8,): mpCamera's parameters (fx fy cx cy [k0..k3])
    fx: float
    fy: float
    cx: float
    cy: float
    invfx: float
    invfy: float
    mb: float
    mbf: float
    cam_type: int = _abi.CAM_PINHOLE
    Tcw_r: np.ndarray | None = None  # the right camera of a rig: GetRightPose(), GetRightCameraCenter(), mpCamera2
    Ow_r: np.ndarray | None = None
    cam_r: np.ndarray | None = None
    depth: np.ndarray | None = None  # mvDepth
    keys_x: np.ndarray | None = None  # mvKeys
    keys_y: np.ndarray | None = None
    median_depth: float = 0.0        # ComputeSceneMedianDepth(2) (neighbours, monocular)

    def __post_init__(self):
        f = np.float32
        self.Tcw = _c(self.Tcw, f).reshape(3, 4)
        self.Ow = _c(self.Ow, f).reshape(3)
        self.Rwc = _c(self.Rwc, f).reshape(3, 3)
        self.twc = _c(self.twc, f).reshape(3)
        self.cam = np.concatenate([_c(self.cam, f).reshape(-1), np.zeros(8, f)])[:8]
        if self.Tcw_r is not None:
            self.Tcw_r = _c(self.Tcw_r, f).reshape(3, 4)
            self.Ow_r = _c(self.Ow_r, f).reshape(3)
            self.cam_r = np.concatenate([_c(self.cam_r, f).reshape(-1), np.zeros(8, f)])[:8]
        self.depth, self.keys_x, self.keys_y = _c(self.depth, f), _c(self.keys_x, f), _c(self.keys_y, f)

    def struct(self):
        s = _abi.OsgNpKf()
        tr = self.Tcw_r if self.Tcw_r is not None else np.zeros((3, 4), np.float32)
        owr = self.Ow_r if self.Ow_r is not None else np.zeros(3, np.float32)
        cr = self.cam_r if self.cam_r is not None else np.zeros(8, np.float32)
        for name, a in (("Tcw", np.concatenate([self.Tcw.ravel(), tr.ravel()])), ("Ow", np.concatenate([self.Ow, owr])),
                        ("Rwc", self.Rwc.ravel()), ("twc", self.twc), ("cam", np.concatenate([self.cam, cr]))):
            dst = getattr(s, name)
            for i, v in enumerate(a):
                dst[i] = float(v)
        s.cam_type = int(self.cam_type)
        for name in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf", "median_depth"):
            setattr(s, name, float(getattr(self, name)))
        s.depth, s.keys_x, s.keys_y = _p(self.depth), _p(self.keys_x), _p(self.keys_y)
        return s


@dataclass
class NewPointsProblem:
    """One current KeyFrame and its neighbours in the order of vpNeighKFs (osg_newpoints_problem).  The
    neighbours must be distinct KeyFrames."""
    kf1: KFSide
    g1: NpKeyFrame
    kf2: list = field(default_factory=list)     # [KFSide]
    g2: list = field(default_factory=list)      # [NpKeyFrame]
    geom: list = field(default_factory=list)    # [TriangGeom] of (kf1, neighbour)
    monocular: bool = False
    inertial: bool = False
    coarse: bool = False
    far_points: bool = False
    th_far_points: float = 0.0
    ratio_factor: float = 1.5 * 1.2

    @property
    def n_neigh(self):
        return len(self.kf2)

    def fill(self, s, keep):
        """Fill the osg_newpoints_problem ``s``; the ctypes arrays it points to are appended to ``keep``."""
        B = self.n_neigh
        assert len(self.g2) == B and len(self.geom) == B
        s.kf1, s.g1, s.n_neigh = self.kf1.struct(), self.g1.struct(), B
        if B:
            a = (_abi.OsgKfSide * B)(*[k.struct() for k in self.kf2])
            g = (_abi.OsgNpKf * B)(*[k.struct() for k in self.g2])
            t = (_abi.OsgTriangGeom * B)(*[k.struct() for k in self.geom])
            keep += [a, g, t]
            s.kf2, s.g2, s.geom = C.addressof(a), C.addressof(g), C.addressof(t)
        s.monocular, s.inertial = int(bool(self.monocular)), int(bool(self.inertial))
        s.coarse, s.far_points = int(bool(self.coarse)), int(bool(self.far_points))
        s.th_far_points, s.ratio_factor = float(self.th_far_points), float(np.float32(self.ratio_factor))

    def struct(self):
        s = _abi.OsgNewPointsProblem()
        s._keep = []
        self.fill(s, s._keep)
        return s


@dataclass
class NewPointsOutput:
    match: np.ndarray      # (B, n1) int32: KF2 index, -1
    status: np.ndarray     # (B, n1) uint8: _abi.NP_* | NP_STEREO_BIT
    x3d: np.ndarray        # (B, n1, 3) float32
    skipped: np.ndarray    # (B,) uint8
    n_created: np.ndarray  # (B,) int32
    total: int = 0

    def created(self):
        """[(b, idx1, idx2, x3D)] in the reference's creation order (ascending b, then idx1)."""
        b, i = np.nonzero((self.status & 0x7f) == _abi.NP_CREATED)
        return [(int(x), int(y), int(self.match[x, y]), self.x3d[x, y].copy()) for x, y in zip(b, i)]


def check_problem(problem: NewPointsProblem) -> int:
    """The host-side argument check of the two entry points (no context, no GPU): 0 or an OSG_E_* code."""
    return int(load_library().osg_create_new_map_points_check(C.byref(problem.struct())))


class CreateNewMapPoints:
    def __init__(self, ctx: Context):
        self.ctx = ctx

    def run(self, problems, outputs=("match", "status", "x3d", "skipped", "n_created")):
        """One NewPointsProblem -> NewPointsOutput; a list -> a list (one batched call).  ``outputs`` names
        the arrays to fetch: the others are passed as null and come back as None."""
        single = isinstance(problems, NewPointsProblem)
        ps = [problems] if single else list(problems)
        n = len(ps)
        keep = []
        st = (_abi.OsgNewPointsProblem * max(n, 1))()
        rs = (_abi.OsgNewPointsResult * max(n, 1))()
        outs = []
        for c, p in enumerate(ps):
            p.fill(st[c], keep)
            B, n1 = p.n_neigh, p.kf1.n
            o = NewPointsOutput(
                match=np.full((B, n1), -1, np.int32) if "match" in outputs else None,
                status=np.zeros((B, n1), np.uint8) if "status" in outputs else None,
                x3d=np.zeros((B, n1, 3), np.float32) if "x3d" in outputs else None,
                skipped=np.zeros(B, np.uint8) if "skipped" in outputs else None,
                n_created=np.zeros(B, np.int32) if "n_created" in outputs else None)
            rs[c].match, rs[c].status, rs[c].x3d = _p(o.match), _p(o.status), _p(o.x3d)
            rs[c].skipped, rs[c].n_created = _p(o.skipped), _p(o.n_created)
            outs.append(o)
        lib, h = self.ctx.lib, self.ctx.handle
        if single:
            rc = lib.osg_create_new_map_points(h, C.byref(st[0]), C.byref(rs[0]))
        else:
            rc = lib.osg_create_new_map_points_batch(h, C.addressof(st), C.addressof(rs), n)
        if rc < 0:
            msg = lib.osg_ctx_last_error(h).decode()
            e = OsgError(f"CreateNewMapPoints: {lib.osg_strerror(rc).decode()} ({msg})")
            e.code = rc
            raise e
        if single:
            outs[0].total = rc
            return outs[0]
        for o in outs:
            o.total = int(o.n_created.sum()) if o.n_created is not None else -1
        return outs


# ------------------------------------------------------------------------------------- synthetic scenes

def _se3(R, C):
    """(Tcw 3x4, Ow, Rwc, twc) as float32 of a camera with rotation R (world -> camera) and centre C."""
    t = -R @ C
    return (np.hstack([R, t[:, None]]).astype(np.float32), C.astype(np.float32), R.T.astype(np.float32),
            C.astype(np.float32))


def synth_newpoints_problem(rng, B=4, n1=300, n2=300, stereo=False, kb8=False, rig=False, monocular=None,
                            inertial=False, n_nodes=60, common=0.6, mp_frac=0.3, noise=0.5, flip=0.04, n_levels=8,
                            baselines=None, depth_range=(2.0, 8.0), near_frac=0.0, depth0_frac=0.0, mb=None,
                            mbf=None, far_points=False, th_far_points=0.0, ratio_factor=None, distract=0.1):
    """One current KeyFrame and ``B`` neighbours seeing one scene (EuRoC image, pinhole or ``kb8`` cameras).
    KF1 keypoint i observes world point i (back-projected to ``depth_range``; ``near_frac`` of them to 0.4-1 m, where
    a stereo keypoint's own parallax beats the rays'); a neighbour observes ``common`` of the points (noise ``noise``
    px x 1.2^octave, noisy descriptor copies, the point's vocabulary node) and random keypoints otherwise,
    ``distract`` of them descriptor copies at random positions.  ``mp_frac`` of every KeyFrame's keypoints already
    carry a MapPoint.  ``stereo``: half of the keypoints get mvuRight / mvDepth (``depth0_frac`` of those a zero
    depth) and mvKeys differs from mvKeysUn by a small distortion.  ``rig``: two-camera KeyFrames (NLeft = n / 2,
    right camera 0.11 m to the right).  ``baselines``: per neighbour the distance of its centre from KF1's
    (default 0.15-0.5 m).  ``mbf`` / ``mb``: per neighbour mbf (default: EuRoC's; its mvuRight follows it) and mb
    (default: mbf / fx).  ``kb8`` problems are coarse (bCoarse):
    the matcher then needs no epipolar geometry.  Returns a NewPointsProblem."""
    from .frames import (KB8_TRIANG, _flip, _rot, fundamental, kb8_project, scale_factors)
    from .synth import EUROC_BF, EUROC_CX, EUROC_CY, EUROC_FX, EUROC_FY, EUROC_H, EUROC_W
    if monocular is None:
        monocular = not stereo and not rig
    K = np.array([[EUROC_FX, 0, EUROC_CX], [0, EUROC_FY, EUROC_CY], [0, 0, 1.0]])
    Kinv = np.linalg.inv(K)
    cam = KB8_TRIANG.copy() if kb8 else np.array([EUROC_FX, EUROC_FY, EUROC_CX, EUROC_CY, 0, 0, 0, 0], np.float32)
    rb = np.array([0.11, 0.0, 0.0])  # right camera centre in the left camera's frame

    def proj(Xc):
        if kb8:
            return kb8_project(KB8_TRIANG, Xc)
        return (K @ (Xc / Xc[2]))[:2]

    # poses: KF1 away from the origin and turned, the neighbours around it
    R1 = _rot(rng, 25.0)
    C1 = np.array([1.5, -0.7, 0.4])
    poses = [(R1, C1)]
    for b in range(B):
        d = rng.normal(size=3) * np.array([1.0, 0.4, 0.25])
        d /= np.linalg.norm(d)
        bl = rng.uniform(0.15, 0.5) if baselines is None else baselines[b]
        poses.append((_rot(rng, rng.uniform(0.5, 3.0)) @ R1, C1 + (R1.T @ d) * bl))
    ns = [n1] + [n2] * B
    nleft = [n // 2 if rig else -1 for n in ns]
    lv = np.array([1.2 ** -i for i in range(n_levels)])
    sf = scale_factors(n_levels)
    if ratio_factor is None:
        ratio_factor = float(np.float32(1.5) * sf[1])   # 1.5f * mfScaleFactor in float, :575
    w = 1.0 / np.arange(1, n_nodes + 1) ** 1.1
    node_ids = np.sort(rng.choice(np.arange(0, 10 * n_nodes), size=n_nodes, replace=False)).astype(np.uint32)

    def cam_pose(k, right):
        R, Cc = poses[k]
        return (R, Cc + R.T @ rb) if right else (R, Cc)

    # KF1 keypoints and the world points behind them
    x1 = rng.uniform(20, EUROC_W - 20, n1)
    y1 = rng.uniform(20, EUROC_H - 20, n1)
    oct1 = rng.choice(n_levels, size=n1, p=lv / lv.sum()).astype(np.int32)
    dep = rng.uniform(*depth_range, n1)
    near = rng.random(n1) < near_frac
    dep[near] = rng.uniform(0.4, 1.0, near.sum())
    Xw = np.zeros((n1, 3))
    for i in range(n1):
        right = rig and i >= nleft[0]
        R, Cc = cam_pose(0, right)
        if kb8:
            Xc = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.6, 0.6), 1.0]) * dep[i]
            x1[i], y1[i] = proj(Xc)
        else:
            Xc = Kinv @ np.array([x1[i], y1[i], 1.0]) * dep[i]
        Xw[i] = R.T @ Xc + Cc
    desc_w = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    node_w = rng.choice(n_nodes, size=n1, p=w / w.sum())

    sides, geos, geoms = [], [], []
    for k in range(B + 1):
        n = ns[k]
        if k == 0:
            x, y, octv = x1.copy(), y1.copy(), oct1.copy()
            depth = dep.copy()
            desc = _flip(rng, desc_w, flip)
            node = node_w.copy()
            x += rng.normal(0, noise, n) * 1.2 ** octv
            y += rng.normal(0, noise, n) * 1.2 ** octv
        else:
            x = rng.uniform(0, EUROC_W, n)
            y = rng.uniform(0, EUROC_H, n)
            octv = rng.choice(n_levels, size=n, p=lv / lv.sum()).astype(np.int32)
            depth = rng.uniform(*depth_range, n)
            desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            node = rng.choice(n_nodes, size=n, p=w / w.sum())
            m = int(common * min(n1, n))
            src = rng.choice(n1, size=m, replace=False)
            dst = rng.choice(n, size=m, replace=False)
            used = np.zeros(n, bool)
            for a, c in zip(src, dst):
                right = rig and c >= nleft[k]
                R, Cc = cam_pose(k, right)
                Xc = R @ (Xw[a] - Cc)
                if Xc[2] <= 0.1:
                    continue
                u = proj(Xc)
                if not (0 <= u[0] < EUROC_W and 0 <= u[1] < EUROC_H):
                    continue
                s = 1.2 ** oct1[a]
                octv[c] = oct1[a]
                x[c], y[c] = u[0] + rng.normal(0, noise * s), u[1] + rng.normal(0, noise * s)
                depth[c] = Xc[2]
                desc[c] = _flip(rng, desc_w[a][None], flip)[0]
                node[c] = node_w[a]
                used[c] = True
            rest = np.flatnonzero(~used)
            for c in rng.choice(rest, size=min(len(rest), int(distract * n)), replace=False):
                a = rng.integers(n1)
                desc[c] = _flip(rng, desc_w[a][None], flip)[0]
                node[c] = node_w[a]
                octv[c] = oct1[a]
        x = np.clip(x, 0, EUROC_W - 1e-3).astype(np.float32)
        y = np.clip(y, 0, EUROC_H - 1e-3).astype(np.float32)
        ur = dp = kx = ky = None
        bf = EUROC_BF if (mbf is None or k == 0) else mbf[k - 1]
        if stereo:
            has = rng.random(n) < 0.5
            dp = np.where(has, depth * (1 + rng.normal(0, 0.002, n)), -1.0).astype(np.float32)
            ur = np.where(has, x - bf / np.maximum(depth, 1e-3), -1.0).astype(np.float32)
            dp[has & (rng.random(n) < depth0_frac)] = 0.0
            kx = (x + np.float32(0.25) * np.sin(y / 40.0)).astype(np.float32)  # mvKeys is not mvKeysUn
            ky = (y + np.float32(0.25) * np.cos(x / 40.0)).astype(np.float32)
        used_nodes = np.unique(node)
        start = np.zeros(len(used_nodes) + 1, np.int32)
        feats = []
        for q, nd in enumerate(used_nodes):
            f = np.flatnonzero(node == nd)
            feats.append(f)
            start[q + 1] = start[q] + len(f)
        sides.append(KFSide(desc=desc, kp_x=x, kp_y=y, kp_angle=rng.uniform(0, 360, n), kp_octave=octv, u_right=ur,
                            has_mp=rng.random(n) < mp_frac, node_id=node_ids[used_nodes], node_start=start,
                            feat=np.concatenate(feats) if feats else np.zeros(0, np.int32), nleft=nleft[k],
                            two_cam=int(rig), scale=sf))
        R, Cc = poses[k]
        Tcw, Ow, Rwc, twc = _se3(R, Cc)
        g = NpKeyFrame(Tcw=Tcw, Ow=Ow, Rwc=Rwc, twc=twc, cam=cam, fx=EUROC_FX, fy=EUROC_FY, cx=EUROC_CX, cy=EUROC_CY,
                       invfx=np.float32(1.0) / np.float32(EUROC_FX), invfy=np.float32(1.0) / np.float32(EUROC_FY),
                       mb=bf / EUROC_FX if (mb is None or k == 0) else mb[k - 1], mbf=bf,
                       cam_type=_abi.CAM_KB8 if kb8 else _abi.CAM_PINHOLE, depth=dp, keys_x=kx, keys_y=ky)
        if rig:
            Rr, Cr = cam_pose(k, True)
            g.Tcw_r, g.Ow_r, _, _ = _se3(Rr, Cr)
            g.cam_r = g.cam.copy()
        if k > 0:
            Xc = (R @ (Xw - Cc).T).T
            z = np.sort(Xc[:, 2])
            g.median_depth = float(np.float32(z[(len(z) - 1) // 2])) if len(z) else 1.0
            F, R12s, t12s = [], [], []
            for c1 in (0, 1) if rig else (0,):
                for c2 in (0, 1) if rig else (0,):
                    Ra, Ca = cam_pose(0, c1)
                    Rb, Cb = cam_pose(k, c2)
                    R12 = Ra @ Rb.T
                    t12 = -Ra @ Ca - R12 @ (-Rb @ Cb)
                    F.append(fundamental(K, K, R12, t12))
                    R12s.append(R12.astype(np.float32))
                    t12s.append(t12.astype(np.float32))
            e = R @ (poses[0][1] - Cc)
            ep = proj(e) if abs(e[2]) > 1e-9 else (0.0, 0.0)
            ep = (np.float32(ep[0]), np.float32(ep[1]))
            if kb8:
                geoms.append(TriangGeom(ep=ep, F12=np.stack(F), pinhole=False, R12=np.stack(R12s), t12=np.stack(t12s),
                                        kb=np.tile(KB8_TRIANG, (4, 1))))
            else:
                geoms.append(TriangGeom(ep=ep, F12=np.stack(F)))
        geos.append(g)
    return NewPointsProblem(kf1=sides[0], g1=geos[0], kf2=sides[1:], g2=geos[1:], geom=geoms, monocular=monocular,
                            inertial=inertial, coarse=bool(kb8), far_points=far_points, th_far_points=th_far_points,
                            ratio_factor=ratio_factor)
