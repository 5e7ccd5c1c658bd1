"""Host mirror of the per-frame projection step of ``Tracking::SearchLocalPoints`` (ref:src/Tracking.cc:4097-4182)
on top of the C ABI: ``Frame::isInFrustum`` over the local MapPoints (``osg_frustum[_batch]``) and the fused
isInFrustum + SearchByProjection call (``osg_search_local_points[_batch]``).

    out = frustum(ctx, frame, points)                       # FrustumOutput
    n, out = search_local_points(ctx, F, frame, points, th=1, slot_mp=slots, slot_taken=taken)

``mp_queries(points, out)`` is the host step of the two-step path: the MPQueries SearchByProjection reads, from
the frustum's outputs.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import Context, _abi
from .frames import FrameSoA, MPQueries, _c, _p

STATUS_NAMES = ("not_candidate", "neg_depth", "outside", "distance", "view_cos", "in_view")


@dataclass
class FrustumCamera:
    """One camera's constants (osg_frustum_camera); float32 values are the reference's own."""
    R: np.ndarray            # (3, 3): mRcw; right camera Rrl * mRcw
    t: np.ndarray            # (3,): mtcw; right camera Rrl * mtcw + trl
    c: np.ndarray            # (3,): mOw; right camera mRwc * tlr + mOw
    cam: np.ndarray          # fx fy cx cy [k0 k1 k2 k3]
    cam_type: int = _abi.CAM_PINHOLE

    def __post_init__(self):
        f = np.float32
        self.R, self.t, self.c = _c(self.R, f).reshape(3, 3), _c(self.t, f).reshape(3), _c(self.c, f).reshape(3)
        self.cam = np.concatenate([_c(self.cam, f).reshape(-1), np.zeros(8, f)])[:8]


@dataclass
class FrustumFrame:
    """A frame's constants (osg_frustum_frame); two cameras: the Nleft != -1 path of a rig."""
    cams: list
    min_x: float
    max_x: float
    min_y: float
    max_y: float
    mbf: float
    log_scale_factor: float
    n_levels: int

    @property
    def two_cam(self):
        return len(self.cams) == 2

    def fill(self, s):
        s.two_cam = int(self.two_cam)
        for k, cam in enumerate(self.cams):
            d = s.cam[k]
            for name, a in (("R", cam.R.ravel()), ("t", cam.t), ("c", cam.c), ("cam", cam.cam)):
                dst = getattr(d, name)
                for i, v in enumerate(a):
                    dst[i] = float(v)
            d.cam_type = int(cam.cam_type)
        for name in ("min_x", "max_x", "min_y", "max_y", "mbf", "log_scale_factor"):
            setattr(s, name, float(np.float32(getattr(self, name))))
        s.n_levels = int(self.n_levels)

    def struct(self):
        s = _abi.OsgFrustumFrame()
        self.fill(s)
        return s


@dataclass
class LocalPoints:
    """mvpLocalMapPoints as arrays (osg_frustum_points; with mp_id / desc / has_obs: osg_local_points)."""
    pos: np.ndarray                  # (n, 3): GetWorldPos()
    normal: np.ndarray               # (n, 3): GetNormal()
    max_dist: np.ndarray             # mfMaxDistance (raw)
    min_dist: np.ndarray             # mfMinDistance (raw)
    candidate: np.ndarray            # mnLastFrameSeen != id && !isBad()
    prev_depth: np.ndarray | None = None  # rig: mTrackDepth before the call
    mp_id: np.ndarray | None = None
    desc: np.ndarray | None = None
    has_obs: np.ndarray | None = None

    def __post_init__(self):
        f = np.float32
        self.pos, self.normal = _c(self.pos, f).reshape(-1, 3), _c(self.normal, f).reshape(-1, 3)
        self.max_dist, self.min_dist = _c(self.max_dist, f), _c(self.min_dist, f)
        self.candidate = _c(self.candidate, np.uint8)
        self.prev_depth = _c(self.prev_depth, f)
        self.mp_id, self.has_obs = _c(self.mp_id, np.int32), _c(self.has_obs, np.uint8)
        self.desc = None if self.desc is None else _c(self.desc, np.uint8).reshape(-1, 32)

    @property
    def n(self):
        return self.pos.shape[0]

    def fill(self, s):
        s.n = self.n
        s.pos, s.normal, s.max_dist, s.min_dist = _p(self.pos), _p(self.normal), _p(self.max_dist), _p(self.min_dist)
        s.candidate, s.prev_depth = _p(self.candidate), _p(self.prev_depth)

    def fill_local(self, s):
        self.fill(s.pts)
        s.mp_id, s.desc, s.has_obs = _p(self.mp_id), _p(self.desc), _p(self.has_obs)


@dataclass
class FrustumOutput:
    """Per camera (row 0 left, row 1 the right camera of a rig) and MapPoint; see include/osg.h for which
    elements the reference wrote at each status."""
    status: np.ndarray     # (ncam, n) uint8: _abi.FRUSTUM_*
    proj_x: np.ndarray     # (ncam, n) float32
    proj_y: np.ndarray
    view_cos: np.ndarray
    depth: np.ndarray
    level: np.ndarray      # (ncam, n) int32
    proj_xr: np.ndarray | None   # (n,) float32, Nleft == -1 only
    n_to_match: int = 0

    @classmethod
    def empty(cls, n, two_cam):
        k = 2 if two_cam else 1
        z = lambda dt: np.zeros((k, n), dt)
        return cls(z(np.uint8), z(np.float32), z(np.float32), z(np.float32), z(np.float32), z(np.int32),
                   None if two_cam else np.zeros(n, np.float32))

    def fill(self, s):
        for k in range(self.status.shape[0]):
            for name in ("status", "proj_x", "proj_y", "view_cos", "depth", "level"):
                getattr(s, name)[k] = _p(getattr(self, name)[k])
        s.proj_xr = _p(self.proj_xr)

    @property
    def in_view(self):
        return self.status == _abi.FRUSTUM_IN_VIEW


def check(frame: FrustumFrame, points: LocalPoints) -> int:
    """The argument checks of osg_frustum alone (host only)."""
    from . import load_library

    fs, ps = frame.struct(), _abi.OsgFrustumPoints()
    points.fill(ps)
    return int(load_library().osg_frustum_check(C.byref(fs), C.byref(ps)))


def frustum(ctx: Context, frame: FrustumFrame, points: LocalPoints, view_cos_limit: float = 0.5) -> FrustumOutput:
    fs, ps, rs = frame.struct(), _abi.OsgFrustumPoints(), _abi.OsgFrustumResult()
    points.fill(ps)
    out = FrustumOutput.empty(points.n, frame.two_cam)
    out.fill(rs)
    out.n_to_match = ctx.check(ctx.lib.osg_frustum(ctx.handle, C.byref(fs), C.byref(ps), float(view_cos_limit),
                                                   C.byref(rs)), "osg_frustum")
    return out


def frustum_batch(ctx: Context, frames, points, view_cos_limit: float = 0.5) -> list:
    B = len(frames)
    assert len(points) == B
    fa, pa, ra = (_abi.OsgFrustumFrame * B)(), (_abi.OsgFrustumPoints * B)(), (_abi.OsgFrustumResult * B)()
    outs = [FrustumOutput.empty(p.n, f.two_cam) for f, p in zip(frames, points)]
    for b in range(B):
        frames[b].fill(fa[b])
        points[b].fill(pa[b])
        outs[b].fill(ra[b])
    ctx.check(ctx.lib.osg_frustum_batch(ctx.handle, C.addressof(fa), C.addressof(pa), B, float(view_cos_limit),
                                        C.addressof(ra)), "osg_frustum_batch")
    for b in range(B):
        outs[b].n_to_match = int(ra[b].n_to_match)
    return outs


def mp_queries(points: LocalPoints, out: FrustumOutput) -> MPQueries:
    """What the caller's MapPoints hold after the frustum's writes, as SearchByProjection reads them."""
    two = out.status.shape[0] == 2
    q = dict(mp_id=points.mp_id, desc=points.desc, usable=points.candidate, has_obs=points.has_obs,
             in_view=out.in_view[0].astype(np.uint8), proj_x=out.proj_x[0], proj_y=out.proj_y[0],
             proj_xr=out.proj_x[1] if two else out.proj_xr, view_cos=out.view_cos[0], pred_level=out.level[0],
             track_depth=out.depth[0])
    if two:
        q.update(in_view_r=out.in_view[1].astype(np.uint8), proj_yr=out.proj_y[1], view_cos_r=out.view_cos[1],
                 pred_level_r=out.level[1])
    return MPQueries(**q)


def search_local_points(ctx: Context, F: FrameSoA, frame: FrustumFrame, points: LocalPoints, th: float = 1.0,
                        nnratio: float = 0.8, far_points: bool = False, th_far_points: float = 50.0,
                        view_cos_limit: float = 0.5, slot_mp=None, slot_taken=None):
    """isInFrustum + SearchByProjection in one call; returns (nmatches, FrustumOutput); slot_mp in place."""
    if slot_mp is None:
        slot_mp = np.full(F.n, -1, np.int32)
    assert slot_mp.dtype == np.int32 and slot_mp.flags["C_CONTIGUOUS"] and len(slot_mp) == F.n
    taken = np.ascontiguousarray(slot_taken if slot_taken is not None else np.zeros(F.n), np.uint8)
    fs, ff, lp, rs = F.struct(), frame.struct(), _abi.OsgLocalPoints(), _abi.OsgFrustumResult()
    points.fill_local(lp)
    out = FrustumOutput.empty(points.n, frame.two_cam)
    out.fill(rs)
    n = ctx.check(ctx.lib.osg_search_local_points(ctx.handle, C.byref(fs), C.byref(ff), C.byref(lp),
                                                  float(view_cos_limit), float(nnratio), float(th),
                                                  int(bool(far_points)), float(th_far_points), slot_mp.ctypes.data,
                                                  taken.ctypes.data, C.byref(rs)), "osg_search_local_points")
    out.n_to_match = int(rs.n_to_match)
    return n, out


def search_local_points_batch(ctx: Context, Fs, frames, points, th: float = 1.0, nnratio: float = 0.8,
                              far_points: bool = False, th_far_points: float = 50.0, view_cos_limit: float = 0.5,
                              slot_mps=None, slot_takens=None):
    """B frames in one call; returns (nmatches[B], [FrustumOutput]); each slot_mps[b] is updated in place."""
    B = len(Fs)
    assert len(frames) == B and len(points) == B
    sizes = [F.n for F in Fs]
    if slot_mps is None:
        slot_mps = [np.full(n, -1, np.int32) for n in sizes]
    if slot_takens is None:
        slot_takens = [np.zeros(n, np.uint8) for n in sizes]
    slot = np.ascontiguousarray(np.concatenate(slot_mps) if B else np.zeros(0), np.int32)
    taken = np.ascontiguousarray(np.concatenate(slot_takens) if B else np.zeros(0), np.uint8)
    fa, ffa = (_abi.OsgFrame * max(B, 1))(), (_abi.OsgFrustumFrame * max(B, 1))()
    la, ra = (_abi.OsgLocalPoints * max(B, 1))(), (_abi.OsgFrustumResult * max(B, 1))()
    outs = [FrustumOutput.empty(p.n, f.two_cam) for f, p in zip(frames, points)]
    for b in range(B):
        fa[b] = Fs[b].struct()
        frames[b].fill(ffa[b])
        points[b].fill_local(la[b])
        outs[b].fill(ra[b])
    nm = np.zeros(max(B, 1), np.int32)
    ctx.check(ctx.lib.osg_search_local_points_batch(ctx.handle, C.addressof(fa), C.addressof(ffa), C.addressof(la), B,
                                                    float(view_cos_limit), float(nnratio), float(th),
                                                    int(bool(far_points)), float(th_far_points), slot.ctypes.data,
                                                    taken.ctypes.data, nm.ctypes.data, C.addressof(ra)),
              "osg_search_local_points_batch")
    off = 0
    for b in range(B):
        slot_mps[b][:] = slot[off:off + sizes[b]]
        off += sizes[b]
        outs[b].n_to_match = int(ra[b].n_to_match)
    return nm[:B], outs
