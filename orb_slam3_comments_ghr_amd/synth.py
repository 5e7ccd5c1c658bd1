"""Seeded synthetic workloads for the benchmark configs.

EuRoC / TUM-VI images, yaml files and ORBvoc.txt are not available, so every config runs on
synthetic data of the documented shape.  All generators are deterministic in their seed.
"""
from __future__ import annotations

import numpy as np

SEED_C2 = 0x0B5EED01
SEED_C2_STREAM = 0x0B5EED02
SEED_C3 = 0x0B5EED03
SEED_C4 = 0x0B5EED04

# EuRoC cam0 intrinsics (upstream ORB-SLAM3 Examples/Stereo/EuRoC.yaml; not in the fork)
EUROC_W, EUROC_H = 752, 480
EUROC_FX, EUROC_FY, EUROC_CX, EUROC_CY = 458.654, 457.296, 367.215, 248.375
EUROC_BF = 47.9
EUROC_K = (EUROC_FX, EUROC_FY, EUROC_CX, EUROC_CY)


def _flip_bits(rng: np.random.Generator, rows: np.ndarray, p: float) -> np.ndarray:
    bits = np.unpackbits(rows, axis=1)
    flips = (rng.random(bits.shape) < p).astype(np.uint8)
    return np.packbits(bits ^ flips, axis=1)


def descriptors_c2(nq: int = 2000, nt: int = 2000, seed: int = SEED_C2):
    """C2: queries uniform; 60 % of train rows are noisy copies (flip p = 0.08, d ~ 20) of a
    random query, the rest uniform (d ~ 128); 5 % of train rows exactly duplicate another train
    row (tie-breaking on the first index)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    n_plant = int(0.6 * nt)
    plant_rows = rng.choice(nt, size=n_plant, replace=False)
    src = rng.integers(0, nq, size=n_plant)
    t[plant_rows] = _flip_bits(rng, q[src], 0.08)
    n_dup = int(0.05 * nt)
    if nt > 1 and n_dup > 0:
        dst = rng.choice(nt, size=n_dup, replace=False)
        srcr = rng.integers(0, nt, size=n_dup)
        t[dst] = t[srcr]
    return q, t


def descriptors_stream(nq: int = 4, nt: int = 1 << 24, seed: int = SEED_C2_STREAM):
    """C2': a few queries against a train set far larger than the 256 MiB Infinity Cache."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, size=(nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, size=(nt, 32), dtype=np.uint8)
    # plant a few near-duplicates so the answer is not arbitrary
    for j in range(nq):
        rows = rng.integers(0, nt, size=3)
        t[rows] = _flip_bits(rng, np.repeat(q[j:j + 1], 3, axis=0), 0.05)
    return q, t


def two_view_scene(rng, n=100, scene="general", noise_px=0.5, outlier_frac=0.0, extra1=37, extra2=23, n_hyp=200,
                   baseline=0.5, rot_deg=4.0, K=EUROC_K, depth=(2.0, 8.0)):
    """Two monocular frames of one synthetic scene as the initialiser sees them: ``n`` matched keypoints (pixel
    noise ``noise_px`` in both frames, ``outlier_frac`` of them with an unrelated frame-2 position) among
    ``extra1`` / ``extra2`` unmatched ones, frame 2's keypoints in shuffled order.  ``scene``: "general" (points
    at 2 .. 8 m), "planar" (a slanted plane), "rotation" (no baseline).  The sets are drawn as the reference
    draws them, from a seeded stream."""
    from .optimizer import small_rotation
    from .twoview import TwoViewProblem, seeded_sets

    fx, fy, cx, cy = K
    R = small_rotation(rng, rot_deg)
    t = np.zeros(3) if scene == "rotation" else baseline * np.array([1.0, 0.15, 0.1]) / np.linalg.norm([1.0, 0.15, 0.1])
    k1, k2 = [], []
    while len(k1) < n:
        u = rng.uniform(20, EUROC_W - 20)
        v = rng.uniform(20, EUROC_H - 20)
        x, y = (u - cx) / fx, (v - cy) / fy
        z = 5.0 / (1.0 + 0.3 * x + 0.2 * y) if scene == "planar" else rng.uniform(*depth)
        X2 = R @ np.array([x * z, y * z, z]) + t
        if X2[2] <= 0.1:
            continue
        u2, v2 = fx * X2[0] / X2[2] + cx, fy * X2[1] / X2[2] + cy
        if not (20 < u2 < EUROC_W - 20 and 20 < v2 < EUROC_H - 20):
            continue
        k1.append((u, v))
        k2.append((u2, v2))
    k1 = np.array(k1).reshape(-1, 2) + rng.normal(0, noise_px, (n, 2))
    k2 = np.array(k2).reshape(-1, 2) + rng.normal(0, noise_px, (n, 2))
    out = rng.random(n) < outlier_frac
    wrong = np.stack([rng.uniform(20, EUROC_W - 20, n), rng.uniform(20, EUROC_H - 20, n)], 1)
    k2 = np.where(out[:, None], wrong, k2)
    rand_keys = lambda m: np.stack([rng.uniform(0, EUROC_W, m), rng.uniform(0, EUROC_H, m)], 1)  # noqa: E731
    n1, n2 = n + extra1, n + extra2
    slot1 = np.sort(rng.choice(n1, n, replace=False))  # where the matched keypoints sit in frame 1
    slot2 = rng.choice(n2, n, replace=False)
    keys1, keys2 = rand_keys(n1), rand_keys(n2)
    keys1[slot1], keys2[slot2] = k1, k2
    m12 = np.full(n1, -1, np.int32)
    m12[slot1] = slot2
    sets = seeded_sets(n, n_hyp, int(rng.integers(1 << 30)))
    return TwoViewProblem(keys1, keys2, m12, sets, K=tuple(K), truth=(R, t, out))


def reloc_scene(rng, n=200, outlier_frac=0.3, noise_px=0.5, planar=False, kb8=False, behind_frac=0.0, n_levels=8):
    """One relocalisation candidate as Tracking::Relocalization hands it to MLPnPsolver: a camera, its pose
    Tcw, ``n`` world MapPoints (float32) and the keypoints they were matched to, with octaves drawn as the
    pyramid populates them.  ``outlier_frac`` of the matches are wrong associations: the keypoint belongs to
    another, unrelated point.  ``planar`` puts every MapPoint on the world plane z == 0 exactly;  ``kb8`` uses
    a KannalaBrandt8 camera with rays out to ~70 degrees;  ``behind_frac`` of the MapPoints are mirrored to
    the back of the camera (MLPnPsolver has no depth test).
    -> dict(cam, R, t, Xw, kp, octave, outlier)."""
    from . import optimizer as O

    cam = O.kb8_camera() if kb8 else O.pinhole_camera()
    n = int(n)

    def rays(m):
        if kb8:
            th = rng.uniform(0.05, 1.25, m)
            ps = rng.uniform(-np.pi, np.pi, m)
            return np.stack([np.tan(th) * np.cos(ps), np.tan(th) * np.sin(ps), np.ones(m)], 1)
        u = rng.uniform(40, EUROC_W - 40, m)
        v = rng.uniform(40, EUROC_H - 40, m)
        return np.stack([(u - EUROC_CX) / EUROC_FX, (v - EUROC_CY) / EUROC_FY, np.ones(m)], 1)

    R = O.small_rotation(rng, 25.0)
    t = rng.normal(0, 0.5, 3)
    if planar:
        # look at the plane z = 0 from 3 .. 5 m up, the optical axis 50 .. 58 degrees off the plane's normal (the
        # reference takes the planar translation scale from rows of the rotation estimate, which fails for a
        # camera that faces the plane squarely)
        C = np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), rng.uniform(3.0, 5.0)])
        tilt = np.deg2rad(rng.uniform(50.0, 58.0))
        az = rng.uniform(-np.pi, np.pi)
        target = C + C[2] * np.array([np.tan(tilt) * np.cos(az), np.tan(tilt) * np.sin(az), -1.0])
        R, t = O.look_at(C, target, up=(0, 0, -1))
        R = O.small_rotation(rng, 3.0) @ R
        t = -R @ C

    def cloud(m):
        d = rays(m)
        if planar:
            # intersect the rays with the world plane z = 0
            dw = d @ R  # R^T d
            C = -R.T @ t
            lam = -C[2] / dw[:, 2]
            Xc = d * lam[:, None]
        else:
            Xc = d * rng.uniform(2.0, 8.0, m)[:, None]
        return Xc

    Xc = cloud(n)
    Xw = ((Xc - t) @ R).astype(np.float32)  # R^T (Xc - t)
    if planar:
        Xw[:, 2] = 0.0
    Xc = Xw.astype(np.float64) @ R.T + t
    def proj(X):
        if kb8:
            return np.stack(O.kb8_project(cam, X), 1)
        return np.stack([EUROC_FX * X[:, 0] / X[:, 2] + EUROC_CX, EUROC_FY * X[:, 1] / X[:, 2] + EUROC_CY], 1)

    pr = proj(Xc)
    lev_p = np.array([1.2 ** -i for i in range(n_levels)])
    lev_p /= lev_p.sum()
    octave = rng.choice(n_levels, n, p=lev_p).astype(np.int32)
    kp = pr + rng.normal(0, noise_px, (n, 2)) * (1.2 ** octave)[:, None]
    out = rng.random(n) < outlier_frac
    kp = np.where(out[:, None], proj(cloud(n)), kp).astype(np.float32)
    if behind_frac > 0:
        back = rng.random(n) < behind_frac
        C = -R.T @ t
        Xw = np.where(back[:, None], (2 * C - Xw.astype(np.float64)), Xw).astype(np.float32)
    return dict(cam=cam, R=R, t=t, Xw=Xw, kp=kp, octave=octave, outlier=out)
