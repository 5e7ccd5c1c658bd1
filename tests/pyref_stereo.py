"""Pure-Python restatements of the two stereo matchers, written apart from the oracle to pin it.  Test
infrastructure only (small frames).

compute_stereo_matches: Frame::ComputeStereoMatches (ref:src/Frame.cc:1117-1373) against oracle/oracle_stereo.c:
Python lists for vRowIndices, numpy bit counts for DescriptorDistance, numpy slices for the SAD, Python's tuple
sort for vDistIdx, float32 scalars for the reference's float arithmetic.

compute_stereo_fisheye_matches: Frame::ComputeStereoFishEyeMatches (ref:src/Frame.cc:1546-1603) against
oracle_stereo_fisheye_matches: knnMatch(k = 2) as a serial insertion into a two-element Python list per query,
the ratio test as float times double, the triangulation verdict from the separately pinned
oracle_kb8_epipolar_constrain (tests/test_oracle_triang.py).

One-decision variants ("Matcher decisions"): ``flip="<name>"`` evaluates exactly one named decision in
its nearest wrong form, ``"<name>:<variant>"`` in another wrong form, so that tests/test_stereo_boundaries.py can
prove that a fixture sits on that decision.  ``flip=None`` is the reference."""
import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50

FLIPS = {
    # vRowIndices
    "rows.radius": "r = 2 * scale[octave of the left keypoint with the right keypoint's index]",
    "rows.radius:one": "r = 2",
    "rows.span": "int(y - r) .. int(y + r): truncation",
    "rows.span:exclusive": "yi < maxr",
    "rows.clip": "a right keypoint whose rows leave the image is indexed on none",
    "stereo.row": "vRowIndices[round(vL)]",
    # coarse search
    "stereo.window": "uR > minU",
    "stereo.window:max": "uR < maxU",
    "stereo.level": "octave in [levelL - 2, levelL + 2]",
    "stereo.level:narrow": "octave in [levelL, levelL]",
    "stereo.high": "bestDist starts at TH_LOW",
    "stereo.tie": "dist <= bestDist: the last candidate wins",
    "stereo.accept": "bestDist <= thOrbDist",
    # block match
    "sad.round": "rint (half to even)",
    "sad.level": "uR0 scaled by, and the strip read at, the right keypoint's level",
    "sad.bound": "endu > cols",
    "sad.inside": "scaledvL - w > 0",
    "sad.inside:bottom": "scaledvL + w < rows - 1 of the left level",
    "sad.inside:bottom_r": "scaledvL + w < rows - 1 of the right level",
    "sad.inside:right": "scaleduL + w < cols - 1 of the left level",
    "sad.inside:strip": "scaleduR0 - L - w > 0",
    "sad.first": "dist <= bestDist: the last minimum",
    "sad.edge": "bestincR == -L kept (the missing neighbour taken as the other one)",
    "sad.edge:hi": "bestincR == L kept (the missing neighbour taken as the other one)",
    # disparity
    "disp.min": "disparity > minD",
    "disp.min:open": "no lower bound: a negative disparity is clamped too",
    "disp.max": "disparity <= maxD",
    "disp.clamp": "disparity < 0 clamps",
    # median cut
    "median.index": "element (size - 1) / 2: the lower middle",
    "median.cut": "first <= thDist kept",
    # ComputeStereoFishEyeMatches
    "fish.second": "a distance equal to the first neighbour's is not the second",
    "fish.ratio": "d0 <= d1 * 0.7",
    "fish.two": "a single right stereo row is matched without a second neighbour",
    "fish.mono": "left rows below monoLeft query too",
    "fish.mono:right": "right rows below monoRight answer too",
    "fish.octave": "sigma1 from the right keypoint's octave, sigma2 from the left's",
    "fish.last": "the first accepted query keeps mvRightToLeftMatch",
}


def _chk(flip, family):
    assert flip is None or (flip in FLIPS and (flip.startswith("fish.") == (family == "fish"))), flip


def _cround(v):
    """C round() on a float value: half away from zero."""
    v = float(v)
    return f32(np.floor(v + 0.5) if v >= 0 else np.ceil(v - 0.5))


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def row_table(F, flip=None):
    """vRowIndices (:1147-1170): the right keypoints of every image row, in index order."""
    nRows = F.left.levels[0].shape[0]
    vRowIndices = [[] for _ in range(nRows)]
    for iR in range(F.n_right):
        o = F.octave[iR % F.n] if flip == "rows.radius" else F.octave_r[iR]
        r = f32(2.0) if flip == "rows.radius:one" else f32(2.0) * F.scale[o]
        hi, lo = f32(F.yr[iR] + r), f32(F.yr[iR] - r)
        maxr = int(hi) if flip == "rows.span" else int(np.ceil(hi))
        minr = int(lo) if flip == "rows.span" else int(np.floor(lo))
        if flip == "rows.clip" and (minr < 0 or maxr >= nRows):
            continue
        for yi in range(minr, maxr if flip == "rows.span:exclusive" else maxr + 1):
            if 0 <= yi < nRows:  # (the reference indexes past vRowIndices here: undefined)
                vRowIndices[yi].append(iR)
    return vRowIndices


def compute_stereo_matches(F, stats=False, flip=None):
    """(mvuRight, mvDepth, kept) [+ accepted before the median cut]."""
    _chk(flip, "stereo")
    N = F.n
    ur = np.full(N, -1, f32)
    depth = np.full(N, -1, f32)
    nRows = F.left.levels[0].shape[0]
    vRowIndices = row_table(F, flip) if N else []
    minZ = f32(F.mb)
    minD = f32(0)
    maxD = f32(f32(F.mbf) / minZ)
    rnd = (lambda v: f32(np.rint(v))) if flip == "sad.round" else _cround
    vDistIdx = []
    for iL in range(N):
        levelL = int(F.octave[iL])
        vL, uL = F.y[iL], F.x[iL]
        row = int(_cround(vL)) if flip == "stereo.row" else int(vL)
        if not vL >= 0 or row >= nRows:
            continue
        cands = vRowIndices[row]
        if not cands:
            continue
        minU, maxU = f32(uL - maxD), f32(uL - minD)
        if maxU < 0:
            continue
        wide = {"stereo.level": 2, "stereo.level:narrow": 0}.get(flip, 1)
        bestDist, bestIdxR = (TH_LOW if flip == "stereo.high" else TH_HIGH), 0
        for iR in cands:
            if F.octave_r[iR] < levelL - wide or F.octave_r[iR] > levelL + wide:
                continue
            uR = F.xr[iR]
            if (uR > minU if flip == "stereo.window" else uR >= minU) and (
                    uR < maxU if flip == "stereo.window:max" else uR <= maxU):
                d = _hamming(F.desc[iL], F.desc_r[iR])
                if d <= bestDist if flip == "stereo.tie" else d < bestDist:
                    bestDist, bestIdxR = d, iR
        thOrbDist = (TH_HIGH + TH_LOW) // 2
        if not (bestDist <= thOrbDist if flip == "stereo.accept" else bestDist < thOrbDist):
            continue
        levelR = int(F.octave_r[bestIdxR]) if flip == "sad.level" else levelL
        sf = F.inv_scale[levelL]
        suL, svL, suR0 = rnd(f32(uL * sf)), rnd(f32(vL * sf)), rnd(f32(F.xr[bestIdxR] * F.inv_scale[levelR]))
        ImL, ImR = F.left.levels[levelL], F.right.levels[levelR]
        if suR0 < 0 or (suR0 + 11 > ImR.shape[1] if flip == "sad.bound" else suR0 + 11 >= ImR.shape[1]):
            continue  # iniu / endu, :1280-1284
        pu, pv, pr = int(suL), int(svL), int(suR0)
        tight = {"sad.inside": "top", "sad.inside:bottom": "bottom", "sad.inside:bottom_r": "bottom_r",
                 "sad.inside:right": "right", "sad.inside:strip": "strip"}.get(flip)
        if (pv - 5 < (tight == "top") or pv + 5 >= ImL.shape[0] - (tight == "bottom")
                or pv + 5 >= ImR.shape[0] - (tight == "bottom_r") or pu - 5 < 0
                or pu + 5 >= ImL.shape[1] - (tight == "right") or pr - 10 < (tight == "strip")
                or pr + 10 >= ImR.shape[1]):
            continue  # the reference's rowRange / colRange would throw
        IL = ImL[pv - 5:pv + 6, pu - 5:pu + 6].astype(np.int64)
        dists = [f32(np.abs(IL - ImR[pv - 5:pv + 6, pr + inc - 5:pr + inc + 6].astype(np.int64)).sum())
                 for inc in range(-5, 6)]
        k = dists.index(min(dists))  # the first minimum
        if flip == "sad.first":
            k = 10 - dists[::-1].index(min(dists))
        inc = k - 5
        if (inc == -5 and flip != "sad.edge") or (inc == 5 and flip != "sad.edge:hi"):
            continue
        d2 = dists[k]
        d1 = dists[k - 1] if k > 0 else dists[k + 1]
        d3 = dists[k + 1] if k < 10 else dists[k - 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if deltaR < -1 or deltaR > 1:  # unreachable (ComputeStereoMatches, "Dead code")
            continue
        bestuR = f32(F.scale[levelL] * f32(f32(suR0 + f32(inc)) + deltaR))
        disparity = f32(uL - bestuR)
        low = {"disp.min": disparity > minD, "disp.min:open": True}.get(flip, disparity >= minD)
        if low and (disparity <= maxD if flip == "disp.max" else disparity < maxD):
            if disparity < 0 if flip == "disp.clamp" else disparity <= 0:
                disparity = f32(0.01)
                bestuR = f32(float(uL) - 0.01)
            with np.errstate(divide="ignore"):
                depth[iL] = f32(f32(F.mbf) / disparity)
            ur[iL] = bestuR
            vDistIdx.append((int(dists[k]), iL))
    kept = len(vDistIdx)
    if vDistIdx:
        vDistIdx.sort()
        mid = (len(vDistIdx) - 1) // 2 if flip == "median.index" else len(vDistIdx) // 2
        thDist = f32(f32(f32(1.5) * f32(1.4)) * f32(vDistIdx[mid][0]))
        for dist, iL in vDistIdx:
            if not (f32(dist) <= thDist if flip == "median.cut" else f32(dist) < thDist):
                ur[iL] = depth[iL] = -1
                kept -= 1
    return (ur, depth, kept, len(vDistIdx)) if stats else (ur, depth, kept)


_oracle = None


def _verdict(cl, cr, kl, kr, R, t, sigma1, sigma2):
    """KannalaBrandt8::TriangulateMatches(...) > 0.0001f through the oracle's pinned epipolarConstrain."""
    global _oracle
    if _oracle is None:
        from tests import oracle_calls
        _oracle = oracle_calls.load()
    return bool(_oracle.oracle_kb8_epipolar_constrain(cl.ctypes.data, cr.ctypes.data, float(kl[0]), float(kl[1]),
                                                      float(kr[0]), float(kr[1]), R.ctypes.data, t.ctypes.data,
                                                      float(sigma1), float(sigma2)))


def compute_stereo_fisheye_matches(F, flip=None):
    """(mvLeftToRightMatch, mvRightToLeftMatch, nMatches, rows that carry a depth)."""
    _chk(flip, "fish")
    kl, ol, dl, kr, orr, dr, s2, cl, cr, R, t = F.args()
    nl, nr = len(kl), len(kr)
    l2r, r2l, has_depth = [-1] * nl, [-1] * nr, [False] * nl
    monoLeft = 0 if flip == "fish.mono" else F.mono_left
    monoRight = 0 if flip == "fish.mono:right" else F.mono_right
    nMatches = 0
    for q in range(nl - monoLeft):  # queryIdx
        knn = []  # [(distance, trainIdx)], ascending, at most two
        for tr in range(nr - monoRight):
            d = _hamming(dl[q + monoLeft], dr[tr + monoRight])
            if not knn or d < knn[0][0]:
                knn.insert(0, (d, tr))
            elif len(knn) < 2 or d < knn[1][0]:
                if flip == "fish.second" and d == knn[0][0]:
                    continue
                knn[1:] = [(d, tr)]
            del knn[2:]
        if flip == "fish.two" and len(knn) == 1:
            knn.append((float("inf"), -1))
        if len(knn) < 2:
            continue
        d0, d1 = float(f32(knn[0][0])), float(f32(knn[1][0])) * 0.7  # float, and float times double
        if not (d0 <= d1 if flip == "fish.ratio" else d0 < d1):
            continue
        i, j = q + monoLeft, knn[0][1] + monoRight  # frame indices
        sigma1, sigma2 = s2[ol[i]], s2[orr[j]]
        if flip == "fish.octave":
            sigma1, sigma2 = sigma2, sigma1
        if _verdict(cl, cr, kl[i], kr[j], R, t, sigma1, sigma2):
            l2r[i] = j
            if not (flip == "fish.last" and r2l[j] >= 0):
                r2l[j] = i
            has_depth[i] = True
            nMatches += 1
    return np.array(l2r, np.int32), np.array(r2l, np.int32), nMatches, np.array(has_depth, bool)
