"""Second, independent restatement of the reference matchers in pure Python (float32 scalars for
the reference's float arithmetic).  Slow — small inputs only.  Used to pin the C oracle
(tests/test_oracle_match.py); never used by the product."""
import math

import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW, HISTO = 100, 50, 30

# One-decision variants ("Matcher decisions"): ``flip="<name>"`` evaluates exactly one
# named decision of the reference in a wrong form, so that tests/test_matcher_boundaries.py can prove
# that a fixture sits on that decision.  ``name`` is the decision's nearest wrong form; ``name:variant``
# another wrong form of the same decision.  ``flip=None`` is the reference.
FLIPS = {
    "area.window": "|dx| <= r && |dy| <= r",
    "area.order": "iy outer, ix inner",
    "area.clamp": "max cell clamped to COLS - 2 / ROWS - 2",
    "fuse.level": "octave in [pred - 1, pred + 1]",
    "fuse.level:narrow": "octave in [pred, pred]",
    "fuse.chi2_mono": "e2 * inv_sigma2 in double against 5.99",
    "fuse.chi2_stereo": "e2 * inv_sigma2 in double against 7.8",
    "fuse.chi2_stereo:kpr": "stereo gate iff u_right > 0",
    "fuse.tie": "dist <= best: the last candidate wins",
    "fuse.accept": "best < TH_LOW",
    "fuse.right_index": "mvuRight read at idx + nleft",
    "sim3.accept": "best < TH_LOW * ratio",
    "sim3.accept:double": "TH_LOW * ratio in double",
    "sim3.taken": "a slot claimed by any other MapPoint is skipped",
    "sim3.taken:never": "taken slots are not skipped",
    "sim3.tie": "dist <= best",
    "sim3.level": "octave in [pred - 1, pred + 1]",
    "sim3.level:narrow": "octave in [pred, pred]",
    "bysim3.accept": "best < TH_HIGH",
    "bysim3.mutual": "one-way matches kept",
    "tri.tie": "the first of equal distances wins",
    "tri.accept": "dist >= TH_LOW skips",
    "tri.epipole": "dist^2 <= 100 * scale skips",
    "tri.epipole:always": "epipole test with a stereo side or a two-camera rig too",
    "tri.epipolar": "3.84 * sigma2 in float",
    "tri.filters": "KF2 keypoints with a MapPoint kept",
    "tri.filters:mp1": "KF1 keypoints with a MapPoint kept",
    "tri.filters:stereo1": "bOnlyStereo not applied to KF1",
    "tri.filters:stereo2": "bOnlyStereo not applied to KF2",
    "tri.filters:coarse": "bCoarse does not bypass the epipolar test",
    "rot.round": "rintf (half to even)",
    "rot.round:wrap": "rot <= 0 wraps",
    "maxima.order": ">=: the later of two equal bins ranks higher",
    "maxima.tenth": "max < 0.1f * max1 as <=",
    "init.level0": "F1 keypoints of every level",
    "init.level0:f2": "F2 candidates of every level",
    "init.md": "vMatchedDistance < dist skips",
    "init.top2": "a distance equal to the best is not the second best",
    "init.accept": "b1 < TH_LOW",
    "init.accept:ratio": "b1 <= b2 * nnratio",
    "init.steal_hist": "only live matches counted in the histogram",
    # SearchByProjection(Frame, MapPoints)
    "mps.far": "depth >= thFar skips",
    "mps.bad": "bad MapPoints searched",
    "mps.radius": "viewCos > 0.998 compared in float",
    "mps.level": "octave in [lvl - 1, lvl + 1]",
    "mps.level:narrow": "octave in [lvl, lvl]",
    "mps.taken": "a slot with any MapPoint is skipped, whatever its Observations",
    "mps.taken:never": "taken slots are not skipped",
    "mps.stereo": "|proj_xr - u_right| >= R skips",
    "mps.stereo:kpr": "stereo gate iff u_right >= 0",
    "mps.tie": "dist <= best: the last candidate wins",
    "mps.top2": "a distance equal to the best is not the second best",
    "mps.accept": "best < TH_HIGH",
    "mps.ratio": "best >= nn * best2 rejects",
    "mps.ratio:level": "ratio test whatever the two levels",
    "mps.ratio:double": "nn * best2 in double",
    "mps.skip_right": "the right pass runs after a left ratio failure",
    "mps.partner": "left_to_right partner slot not written",
    "mps.partner:r2l": "right_to_left partner slot not written",
    "mps.own": "the query's own partner slot always blocks its right pass",
    "mps.own:never": "the query's own partner slot never blocks its right pass",
    "mps.level_r": "pred_level_r == -1 does not skip the right pass",
    "mps.radius_r": "the right pass radius takes the th factor",
    # SearchByProjection(Frame, LastFrame)
    "last.invz": "invz <= 0 skips",
    "last.bounds": "u <= min_x || u >= max_x, likewise v",
    "last.forward": "tlc_z >= mb",
    "last.backward": "-tlc_z >= mb",
    "last.mono": "bMono does not disable forward / backward",
    "last.level": "octave in [o - 2, o + 2]",
    "last.level:narrow": "octave in [o, o]",
    "last.level:fwd": "forward: octave in [o - 1, inf)",
    "last.level:fwd_narrow": "forward: octave in [o + 1, inf)",
    "last.level:bwd": "backward: octave in [0, o + 1]",
    "last.level:bwd_narrow": "backward: octave in [0, o - 1]",
    "last.taken": "a slot with any MapPoint is skipped, whatever its Observations",
    "last.taken:never": "taken slots are not skipped",
    "last.stereo": "|ur - u_right| >= radius skips",
    "last.stereo:kpr": "stereo gate iff u_right >= 0",
    "last.tie": "dist <= best: the last candidate wins",
    "last.accept": "best < TH_HIGH",
    "last.empty_left": "the right pass runs after an empty left window",
    "last.hist_right": "right matches are left out of the histogram",
    "last.hist_stale": "a match overwritten by a later one leaves the histogram",
    # SearchByProjection(Frame, KeyFrame)
    "kf.level": "octave in [lvl - 2, lvl + 2]",
    "kf.level:narrow": "octave in [lvl - 1, lvl]",
    "kf.taken": "slots with a MapPoint are not skipped",
    "kf.tie": "dist <= best: the last candidate wins",
    "kf.accept": "best < ORBdist",
    "kf.accept:high": "best <= TH_HIGH, not the parameter",
    # SearchByBoW(KF, F)
    "bow.good": "KeyFrame features without a good MapPoint kept",
    "bow.taken": "frame features already matched are not skipped",
    "bow.tie": "dist <= best: the last candidate wins",
    "bow.top2": "a distance equal to the best is not the second best",
    "bow.accept": "best < TH_LOW",
    "bow.ratio": "best <= nn * best2 accepts",
    "bow.ratio:double": "nn * best2 in double",
    "bow.side": "index == nleft goes to the left top-2",
    "bow.right_gate": "the right match is looked at whatever the left best",
    "bow.right_gate:ratio": "the right match is looked at only after a left ratio success",
    "bow.right_ratio": "ratio test on the right match",
    "bow.nodes": "nodes paired by position, not by id",
    # SearchByBoW(KF, KF)
    "bowkk.accept": "best <= TH_LOW",
    "bowkk.ratio": "best <= nn * best2 accepts",
    "bowkk.ratio:double": "nn * best2 in double",
    "bowkk.matched2": "KF2 features already matched are not skipped",
    "bowkk.mp2": "KF2 features without a MapPoint kept",
    "bowkk.mp2:bad": "KF2 features with a bad MapPoint kept",
    "bowkk.right": "KF1 indices >= nleft kept",
    "bowkk.right:k2": "KF2 indices >= nleft kept",
    "bowkk.tie": "dist <= best: the last candidate wins",
    "bowkk.top2": "a distance equal to the best is not the second best",
}


def _chk(flip):
    assert flip is None or flip in FLIPS, flip


def dist(a, b):
    return int(np.bitwise_count(np.bitwise_xor(a, b)).sum())


def features_in_area(F, x, y, r, minL=-1, maxL=-1, right=False, flip=None):
    """Frame::GetFeaturesInArea; ``right`` walks mGridRight (indices relative to Nleft)."""
    x, y, r = f32(x), f32(y), f32(r)
    out = []
    minCX = max(0, int(math.floor(f32(f32(x - f32(F.min_x)) - r) * F.inv_w)))
    if minCX >= 64:
        return out
    maxCX = min(63, int(math.ceil(f32(f32(x - f32(F.min_x)) + r) * F.inv_w)))
    if maxCX < 0:
        return out
    minCY = max(0, int(math.floor(f32(f32(y - f32(F.min_y)) - r) * F.inv_h)))
    if minCY >= 48:
        return out
    maxCY = min(47, int(math.ceil(f32(f32(y - f32(F.min_y)) + r) * F.inv_h)))
    if maxCY < 0:
        return out
    chk = (minL > 0) or (maxL >= 0)
    gs, gi = (F.grid_start_r, F.grid_idx_r) if right else (F.grid_start, F.grid_idx)
    off = F.nleft if right else 0
    if flip == "area.clamp":
        maxCX, maxCY = min(maxCX, 62), min(maxCY, 46)
    cells = [(ix, iy) for ix in range(minCX, maxCX + 1) for iy in range(minCY, maxCY + 1)]
    if flip == "area.order":
        cells.sort(key=lambda c: (c[1], c[0]))
    for ix, iy in cells:
        c = ix * 48 + iy
        for j in range(gs[c], gs[c + 1]):
            idx = int(gi[j])
            k = idx + off
            o = int(F.kp_octave[k])
            if chk:
                if o < minL:
                    continue
                if maxL >= 0 and o > maxL:
                    continue
            dx, dy = abs(f32(F.kp_x[k] - x)), abs(f32(F.kp_y[k] - y))
            if (dx <= r and dy <= r) if flip == "area.window" else (dx < r and dy < r):
                out.append(idx)
    return out


def rot_bin(a, b, flip=None):
    rot = f32(f32(a) - f32(b))
    if rot <= 0.0 if flip == "rot.round:wrap" else rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(f32(1.0) / f32(30))))
    b_ = int(math.floor(v + 0.5))  # round half away from zero, v >= 0
    if flip == "rot.round":
        b_ = int(np.rint(v))
    return 0 if b_ == 30 else b_


def three_maxima(sizes, flip=None):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    gt = (lambda a, b: a >= b) if flip == "maxima.order" else (lambda a, b: a > b)
    lt = (lambda a, b: a <= b) if flip == "maxima.tenth" else (lambda a, b: a < b)
    for i, s in enumerate(sizes):
        if gt(s, m1):
            m3, m2, m1 = m2, m1, s
            i3, i2, i1 = i2, i1, i
        elif gt(s, m2):
            m3, m2 = m2, s
            i3, i2 = i2, i
        elif gt(s, m3):
            m3, i3 = s, i
    if lt(m2, f32(0.1) * f32(m1)):
        i2 = i3 = -1
    elif lt(m3, f32(0.1) * f32(m1)):
        i3 = -1
    return i1, i2, i3


def apply_hist(hist, slots, nm, flip=None):
    keep = three_maxima([len(h) for h in hist], flip)
    for i in range(HISTO):
        if i in keep:
            continue
        for s in hist[i]:
            slots[s] = -1
            nm -= 1
    return nm


class _Top2:
    """bestDist / bestLevel / bestDist2 / bestLevel2 / bestIdx of the reference loops; ``tie``: the last of
    equal distances wins, ``top2``: a distance equal to the best is not the second best (wrong forms)."""

    def __init__(self, tie=False, top2=False):
        self.b, self.bl, self.b2, self.bl2, self.bi = 256, -1, 256, -1, -1
        self.tie, self.top2 = tie, top2

    def push(self, d, lvl, idx):
        if (d <= self.b and d < 256) if self.tie else d < self.b:
            self.b2, self.bl2, self.b, self.bl, self.bi = self.b, self.bl, d, lvl, idx
        elif d < self.b2 and not (self.top2 and d == self.b):
            self.b2, self.bl2 = d, lvl


def _ratio_gt(b, nn, b2, flip, name):
    """(float)best > nnratio * (float)best2 and its wrong forms ``name`` (>=) and ``name:double``."""
    if flip == name + ":double":
        return float(b) > float(nn) * float(b2)
    return f32(b) >= nn * f32(b2) if flip == name else f32(b) > nn * f32(b2)


def _ratio_lt(b, nn, b2, flip, name):
    """(float)best < nnratio * (float)best2 and its wrong forms ``name`` (<=) and ``name:double``."""
    if flip == name + ":double":
        return float(b) < float(nn) * float(b2)
    return f32(b) <= nn * f32(b2) if flip == name else f32(b) < nn * f32(b2)


def search_mps(F, Q, nn, th, far, thfar, slot_mp, slot_taken, flip=None):
    _chk(flip)
    slots = slot_mp.copy()
    taken = slot_taken.copy()
    nm = 0
    nn = f32(nn)
    two = F.nleft != -1

    def assign(s, i):
        slots[s] = Q.mp_id[i]
        taken[s] = Q.has_obs[i]

    def radius(c):
        if flip == "mps.radius":
            return f32(2.5) if f32(c) > f32(0.998) else f32(4.0)
        return f32(2.5) if float(c) > 0.998 else f32(4.0)

    def blocked(s):
        if flip == "mps.taken:never":
            return False
        return slots[s] >= 0 and (bool(taken[s]) or flip == "mps.taken")

    def levels(lvl):
        if lvl < 0:
            return lvl - 1, lvl  # only under mps.level_r: no level check at all (Frame.cc:919)
        if flip == "mps.level":
            return lvl - 1, lvl + 1
        return (lvl, lvl) if flip == "mps.level:narrow" else (lvl - 1, lvl)

    def top2():
        return _Top2(tie=flip == "mps.tie", top2=flip == "mps.top2")

    def rejected(t):
        same = t.bl == t.bl2 or flip == "mps.ratio:level"
        return same and _ratio_gt(t.b, nn, t.b2, flip, "mps.ratio")

    def accepted(t):
        return t.b < TH_HIGH if flip == "mps.accept" else t.b <= TH_HIGH

    for i in range(len(Q.mp_id)):
        in_r = Q.in_view_r is not None and bool(Q.in_view_r[i])
        if not Q.in_view[i] and not in_r:
            continue
        if far and (Q.track_depth[i] >= f32(thfar) if flip == "mps.far" else Q.track_depth[i] > f32(thfar)):
            continue
        if not Q.usable[i] and flip != "mps.bad":
            continue
        own = -1
        if Q.in_view[i]:
            lvl = int(Q.pred_level[i])
            r = radius(Q.view_cos[i])
            if f32(th) != f32(1.0):
                r = f32(r * f32(th))
            R = f32(r * F.scale[lvl])
            t = top2()
            for idx in features_in_area(F, Q.proj_x[i], Q.proj_y[i], R, *levels(lvl), flip=flip):
                if blocked(idx):
                    continue
                kpr = F.u_right[idx] if not two and F.u_right is not None else f32(-1)
                if kpr >= 0 if flip == "mps.stereo:kpr" else kpr > 0:
                    er = abs(f32(Q.proj_xr[i] - kpr))
                    if er >= R if flip == "mps.stereo" else er > R:
                        continue
                t.push(dist(Q.desc[i], F.desc[idx]), int(F.kp_octave[idx]), idx)
            if accepted(t):
                if rejected(t):
                    if flip != "mps.skip_right":
                        continue  # skips the right-camera pass too
                else:
                    assign(t.bi, i)
                    nm += 1
                    if two and F.left_to_right is not None and F.left_to_right[t.bi] != -1 and flip != "mps.partner":
                        own = F.left_to_right[t.bi] + F.nleft
                        assign(own, i)
                        nm += 1
        if two and in_r:
            lvl = int(Q.pred_level_r[i])
            if lvl == -1 and flip != "mps.level_r":
                continue
            r = radius(Q.view_cos_r[i])
            if flip == "mps.radius_r" and f32(th) != f32(1.0):
                r = f32(r * f32(th))
            R = f32(r * F.scale[max(lvl, 0)])
            t = top2()
            for idx in features_in_area(F, Q.proj_xr[i], Q.proj_yr[i], R, *levels(lvl), right=True, flip=flip):
                s_ = idx + F.nleft
                if s_ == own and flip in ("mps.own", "mps.own:never"):
                    if flip == "mps.own":
                        continue
                elif blocked(s_):
                    continue
                t.push(dist(Q.desc[i], F.desc[s_]), int(F.kp_octave[s_]), idx)
            if accepted(t):
                if rejected(t):
                    continue
                if F.right_to_left is not None and F.right_to_left[t.bi] != -1 and flip != "mps.partner:r2l":
                    assign(F.right_to_left[t.bi], i)
                    nm += 1
                assign(t.bi + F.nleft, i)
                nm += 1
    return nm, slots


def search_last(F, L, th, mono, ori, slot_mp, slot_taken, flip=None):
    _chk(flip)
    slots = slot_mp.copy()
    taken = slot_taken.copy()
    hist = [[] for _ in range(HISTO)]
    nm = 0
    two = F.nleft != -1
    tz, mb = f32(L.tlc_z), f32(F.mb)
    owner = {}  # slot -> the last query that wrote it
    not_mono = not mono or flip == "last.mono"
    fwd = (tz >= mb if flip == "last.forward" else tz > mb) and not_mono
    bwd = (-tz >= mb if flip == "last.backward" else -tz > mb) and not_mono
    wide = {"last.level": (1, 1), "last.level:narrow": (-1, -1), "last.level:fwd": (1, 0),
            "last.level:fwd_narrow": (-1, 0), "last.level:bwd": (0, 1), "last.level:bwd_narrow": (0, -1)}
    lo_, hi_ = wide.get(flip, (0, 0))

    def window(u, v, rad, o, right):
        if fwd:
            lo_f = lo_ if flip in ("last.level:fwd", "last.level:fwd_narrow") else 0
            return features_in_area(F, u, v, rad, o - lo_f, -1, right, flip=flip)
        if bwd:
            hi_b = hi_ if flip in ("last.level:bwd", "last.level:bwd_narrow") else 0
            return features_in_area(F, u, v, rad, 0, o + hi_b, right, flip=flip)
        w = lo_ if flip in ("last.level", "last.level:narrow") else 0
        return features_in_area(F, u, v, rad, o - 1 - w, o + 1 + w, right, flip=flip)

    def blocked(s):
        if flip == "last.taken:never":
            return False
        return slots[s] >= 0 and (bool(taken[s]) or flip == "last.taken")

    def better(d, b):
        return (d <= b and d < 256) if flip == "last.tie" else d < b

    def accepted(b):
        return b < TH_HIGH if flip == "last.accept" else b <= TH_HIGH

    for i in range(len(L.mp_id)):
        if not L.valid[i]:
            continue
        invz = L.invz[i]
        if invz <= 0 if flip == "last.invz" else invz < 0:
            continue
        u, v = L.u[i], L.v[i]
        x0, x1, y0, y1 = f32(F.min_x), f32(F.max_x), f32(F.min_y), f32(F.max_y)
        if flip == "last.bounds":
            if u <= x0 or u >= x1 or v <= y0 or v >= y1:
                continue
        elif u < x0 or u > x1 or v < y0 or v > y1:
            continue
        o = int(L.octave[i])
        rad = f32(f32(th) * F.scale[o])
        c = window(u, v, rad, o, False)
        if not c and flip != "last.empty_left":
            continue
        b, bi = 256, -1
        for i2 in c:
            if blocked(i2):
                continue
            kpr = F.u_right[i2] if not two and F.u_right is not None else f32(-1)
            if kpr >= 0 if flip == "last.stereo:kpr" else kpr > 0:
                ur = f32(u - f32(f32(F.mbf) * invz))
                er = abs(f32(ur - kpr))
                if er >= rad if flip == "last.stereo" else er > rad:
                    continue
            d = dist(L.desc[i], F.desc[i2])
            if better(d, b):
                b, bi = d, i2
        if accepted(b):
            slots[bi] = L.mp_id[i]
            taken[bi] = L.has_obs[i]
            nm += 1
            owner[bi] = i
            if ori:
                hist[rot_bin(L.angle[i], F.kp_angle[bi], flip)].append((bi, i))
        if two:
            b, bi = 256, -1
            for i2 in window(L.u_r[i], L.v_r[i], rad, o, True):
                s_ = i2 + F.nleft
                if blocked(s_):
                    continue
                d = dist(L.desc[i], F.desc[s_])
                if better(d, b):
                    b, bi = d, s_
            if accepted(b):
                slots[bi] = L.mp_id[i]
                taken[bi] = L.has_obs[i]
                nm += 1
                owner[bi] = i
                if ori and flip != "last.hist_right":
                    hist[rot_bin(L.angle[i], F.kp_angle[bi], flip)].append((bi, i))
    if ori:
        # rotHist keeps every accepted match, also one whose slot a later query took again
        stale = flip == "last.hist_stale"
        nm = apply_hist([[s for s, i in h if not stale or owner[s] == i] for h in hist], slots, nm, flip)
    return nm, slots


def search_kf(F, K, th, orb, ori, slot_mp, flip=None):
    _chk(flip)
    slots = slot_mp.copy()
    hist = [[] for _ in range(HISTO)]
    nm = 0
    for i in range(len(K.mp_id)):
        if not K.valid[i]:
            continue
        lvl = int(K.pred_level[i])
        rad = f32(f32(th) * F.scale[lvl])
        lo, hi = lvl - 1, lvl + 1
        if flip == "kf.level":
            lo, hi = lvl - 2, lvl + 2
        elif flip == "kf.level:narrow":
            hi = lvl
        c = features_in_area(F, K.u[i], K.v[i], rad, lo, hi, flip=flip)
        if not c:
            continue
        b, bi = 256, -1
        for i2 in c:
            if slots[i2] >= 0 and flip != "kf.taken":
                continue
            d = dist(K.desc[i], F.desc[i2])
            if (d <= b and d < 256) if flip == "kf.tie" else d < b:
                b, bi = d, i2
        lim = TH_HIGH if flip == "kf.accept:high" else orb
        if b < lim if flip == "kf.accept" else b <= lim:
            slots[bi] = K.mp_id[i]
            nm += 1
            if ori:
                hist[rot_bin(K.angle[i], F.kp_angle[bi], flip)].append(bi)
    if ori:
        nm = apply_hist(hist, slots, nm, flip)
    return nm, slots


def _shared_nodes(A, B, by_position=False):
    ra = [(A.node_start[k], A.node_start[k + 1]) for k in range(len(A.node_id))]
    rb = [(B.node_start[k], B.node_start[k + 1]) for k in range(len(B.node_id))]
    if by_position:  # wrong form (bow.nodes): the k-th node of one side against the k-th of the other
        yield from zip(ra, rb)
        return
    ma = {int(n): r for n, r in zip(A.node_id, ra)}
    mb = {int(n): r for n, r in zip(B.node_id, rb)}
    for n in sorted(set(ma) & set(mb)):
        yield ma[n], mb[n]


def search_bow_kf_f(KF, F, nn, ori, flip=None):
    _chk(flip)
    out = np.full(F.n, -1, np.int32)
    hist = [[] for _ in range(HISTO)]
    nm = 0
    nn = f32(nn)
    for (a0, a1), (b0, b1) in _shared_nodes(KF, F, flip == "bow.nodes"):
        for a in range(a0, a1):
            ik = int(KF.feat[a])
            if not KF.mp_good[ik] and flip != "bow.good":
                continue
            tl, tr = (_Top2(tie=flip == "bow.tie", top2=flip == "bow.top2") for _ in range(2))
            for j in range(b0, b1):
                jf = int(F.feat[j])
                if out[jf] >= 0 and flip != "bow.taken":
                    continue
                d = dist(KF.desc[ik], F.desc[jf])
                left = F.nleft == -1 or (jf <= F.nleft if flip == "bow.side" else jf < F.nleft)
                (tl if left else tr).push(d, 0, jf)
            gate = tl.b < TH_LOW if flip == "bow.accept" else tl.b <= TH_LOW
            ratio = gate and _ratio_lt(tl.b, nn, tl.b2, flip, "bow.ratio")
            if ratio:
                out[tl.bi] = KF.mp_id[ik]
                nm += 1
                if ori:
                    hist[rot_bin(KF.angle[ik], F.angle[tl.bi], flip)].append(tl.bi)
            if flip == "bow.right_gate":
                gate = True
            elif flip == "bow.right_gate:ratio":
                gate = ratio
            # right match: ratio test disabled ('|| true')
            if gate and tr.b <= TH_LOW and (flip != "bow.right_ratio" or f32(tr.b) < nn * f32(tr.b2)):
                out[tr.bi] = KF.mp_id[ik]
                nm += 1
                if ori:
                    hist[rot_bin(KF.angle[ik], F.angle[tr.bi], flip)].append(tr.bi)
    if ori:
        nm = apply_hist(hist, out, nm, flip)
    return nm, out


def search_bow_kf_kf(K1, K2, nn, ori, flip=None):
    """Two-camera keyframes: indices >= mvKeysUn.size() == NLeft are skipped on both sides."""
    _chk(flip)
    out = np.full(K1.n, -1, np.int32)
    matched2 = np.zeros(K2.n, bool)
    hist = [[] for _ in range(HISTO)]
    nm = 0
    nn = f32(nn)
    for (a0, a1), (b0, b1) in _shared_nodes(K1, K2):
        for a in range(a0, a1):
            i1 = int(K1.feat[a])
            if K1.nleft != -1 and i1 >= K1.nleft and flip != "bowkk.right":
                continue
            if not K1.mp_good[i1]:
                continue
            t = _Top2(tie=flip == "bowkk.tie", top2=flip == "bowkk.top2")
            for j in range(b0, b1):
                i2 = int(K2.feat[j])
                if K2.nleft != -1 and i2 >= K2.nleft and flip != "bowkk.right:k2":
                    continue
                if matched2[i2] and flip != "bowkk.matched2":
                    continue
                if K2.mp_id[i2] < 0 and flip != "bowkk.mp2":
                    continue
                if not K2.mp_good[i2] and flip != "bowkk.mp2:bad":
                    continue
                t.push(dist(K1.desc[i1], K2.desc[i2]), 0, i2)
            if (t.b <= TH_LOW if flip == "bowkk.accept" else t.b < TH_LOW) and \
                    _ratio_lt(t.b, nn, t.b2, flip, "bowkk.ratio"):
                out[i1] = K2.mp_id[t.bi]
                matched2[t.bi] = True
                nm += 1
                if ori:
                    hist[rot_bin(K1.angle[i1], K2.angle[t.bi], flip)].append(i1)
    if ori:
        nm = apply_hist(hist, out, nm, flip)
    return nm, out


def _level_window(lvl, flip, name):
    if flip == name:
        return lvl - 1, lvl + 1
    if flip == name + ":narrow":
        return lvl, lvl
    return lvl - 1, lvl


def fuse_search(F, Q, th, right=False, gated=True, flip=None):
    """Search half of ORBmatcher::Fuse (both overloads): KeyFrame::GetFeaturesInArea (no levels),
    level window [pred-1, pred], chi2 gate (gated), strict '<' best, accept <= TH_LOW."""
    _chk(flip)
    n = len(Q.valid)
    bi = np.full(n, -1, np.int32)
    bd = np.full(n, 256, np.int32)
    off = F.nleft if right else 0
    nf = 0
    for i in range(n):
        if not Q.valid[i]:
            continue
        lvl = int(Q.pred_level[i])
        rad = f32(f32(th) * F.scale[lvl])
        u, v = f32(Q.u[i]), f32(Q.v[i])
        best, besti = (256 if gated else 2 ** 31 - 1), -1
        lo, hi = _level_window(lvl, flip, "fuse.level")
        for idx in features_in_area(F, u, v, rad, -1, -1, right=right, flip=flip):
            k = idx + off
            o = int(F.kp_octave[k])
            if o < lo or o > hi:
                continue
            if gated:
                ex, ey = f32(u - F.kp_x[k]), f32(v - F.kp_y[k])
                inv = f32(Q.inv_level_sigma2[o])
                kr = F.u_right[k if flip == "fuse.right_index" else idx] if F.u_right is not None else f32(-1)
                if kr > 0 if flip == "fuse.chi2_stereo:kpr" else kr >= 0:
                    er = f32(f32(Q.ur[i]) - f32(kr))
                    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                    chi2 = float(e2) * float(inv) if flip == "fuse.chi2_stereo" else float(f32(e2 * inv))
                    if chi2 > 7.8:
                        continue
                else:
                    e2 = f32(f32(ex * ex) + f32(ey * ey))
                    chi2 = float(e2) * float(inv) if flip == "fuse.chi2_mono" else float(f32(e2 * inv))
                    if chi2 > 5.99:
                        continue
            d = dist(Q.desc[i], F.desc[k])
            if d <= best if flip == "fuse.tie" else d < best:
                best, besti = d, k
        bd[i] = min(best, 256)
        if best < TH_LOW if flip == "fuse.accept" else best <= TH_LOW:
            bi[i] = besti
            nf += 1
    return nf, bi, bd


def search_for_triangulation(K1, K2, geom, only_stereo=False, coarse=False, ori=True, flip=None):
    """ORBmatcher::SearchForTriangulation (ref:src/ORBmatcher.cc:1045-1328) with
    Pinhole::epipolarConstrain (ref:src/CameraModels/Pinhole.cpp:189-219).  Node pairing by set
    intersection (not the reference's lower_bound walk); returns (nmatches, pairs)."""
    nodes1 = {int(K1.node_id[k]): K1.feat[K1.node_start[k]:K1.node_start[k + 1]] for k in range(len(K1.node_id))}
    nodes2 = {int(K2.node_id[k]): K2.feat[K2.node_start[k]:K2.node_start[k + 1]] for k in range(len(K2.node_id))}
    _chk(flip)
    m12 = [-1] * K1.n
    hist = [[] for _ in range(HISTO)]
    nm = 0
    F = geom.F12

    def stereo(K, i):
        return (not K.two_cam) and K.u_right is not None and K.u_right[i] >= 0

    def right(K, i):
        return not (K.nleft == -1 or i < K.nleft)

    for node in sorted(set(nodes1) & set(nodes2)):
        for idx1 in nodes1[node]:
            idx1 = int(idx1)
            if K1.has_mp[idx1] and flip != "tri.filters:mp1":
                continue
            s1 = stereo(K1, idx1)
            if only_stereo and not s1 and flip != "tri.filters:stereo1":
                continue
            x1, y1 = f32(K1.kp_x[idx1]), f32(K1.kp_y[idx1])
            best_d, best = TH_LOW, -1
            for idx2 in nodes2[node]:
                idx2 = int(idx2)
                if K2.has_mp[idx2] and flip != "tri.filters":
                    continue
                s2 = stereo(K2, idx2)
                if only_stereo and not s2 and flip != "tri.filters:stereo2":
                    continue
                d = dist(K1.desc[idx1], K2.desc[idx2])
                if flip == "tri.accept" and d >= TH_LOW:
                    continue
                if flip == "tri.tie" and best >= 0 and d == best_d:
                    continue
                if d > TH_LOW or d > best_d:
                    continue
                x2, y2 = f32(K2.kp_x[idx2]), f32(K2.kp_y[idx2])
                o2 = int(K2.kp_octave[idx2])
                if (not s1 and not s2 and not K1.two_cam) or flip == "tri.epipole:always":
                    ex, ey = f32(f32(geom.ep[0]) - x2), f32(f32(geom.ep[1]) - y2)
                    e2, lim = f32(f32(ex * ex) + f32(ey * ey)), f32(f32(100) * K2.scale[o2])
                    if e2 <= lim if flip == "tri.epipole" else e2 < lim:
                        continue
                k = (2 * right(K1, idx1) + right(K2, idx2)) if (K1.two_cam and K2.two_cam) else 0
                ok = coarse and flip != "tri.filters:coarse"
                if not ok and flip == "tri.epipolar":
                    Fk = F[k]
                    a = f32(f32(f32(x1 * Fk[0, 0]) + f32(y1 * Fk[1, 0])) + Fk[2, 0])
                    b = f32(f32(f32(x1 * Fk[0, 1]) + f32(y1 * Fk[1, 1])) + Fk[2, 1])
                    c = f32(f32(f32(x1 * Fk[0, 2]) + f32(y1 * Fk[1, 2])) + Fk[2, 2])
                    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
                    den = f32(f32(a * a) + f32(b * b))
                    ok = den != 0 and f32(f32(num * num) / den) < f32(f32(3.84) * K2.level_sigma2[o2])
                elif not ok:
                    Fk = F[k]
                    a = f32(f32(f32(x1 * Fk[0, 0]) + f32(y1 * Fk[1, 0])) + Fk[2, 0])
                    b = f32(f32(f32(x1 * Fk[0, 1]) + f32(y1 * Fk[1, 1])) + Fk[2, 1])
                    c = f32(f32(f32(x1 * Fk[0, 2]) + f32(y1 * Fk[1, 2])) + Fk[2, 2])
                    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
                    den = f32(f32(a * a) + f32(b * b))
                    ok = den != 0 and float(f32(f32(num * num) / den)) < 3.84 * float(K2.level_sigma2[o2])
                if ok:
                    best, best_d = idx2, d
            if best >= 0:
                m12[idx1] = best
                nm += 1
                if ori:
                    hist[rot_bin(K1.kp_angle[idx1], K2.kp_angle[best], flip)].append(idx1)
    if ori:
        nm = apply_hist(hist, m12, nm, flip)
    pairs = [(i, j) for i, j in enumerate(m12) if j >= 0]
    return nm, np.array(pairs, np.int64).reshape(-1, 2)


def distinctive(desc_lists):
    """MapPoint::ComputeDistinctiveDescriptors (ref:src/MapPoint.cc:444-535) with numpy: the distance
    matrix by bitwise_count, per-row sorted median at int(0.5 * (N - 1)), first minimum."""
    out = []
    for d in desc_lists:
        d = np.asarray(d, np.uint8).reshape(-1, 32)
        n = len(d)
        if n == 0:
            out.append(-1)
            continue
        M = np.bitwise_count(d[:, None, :] ^ d[None, :, :]).sum(axis=2)
        med = np.sort(M, axis=1)[:, int(0.5 * (n - 1))]
        out.append(int(np.argmin(med)))
    return np.array(out, np.int32)


def search_sim3(F, Q, th, ratio, slot_query, flip=None):
    """SearchByProjection(KeyFrame*, Sim3f&, ...) (ref:src/ORBmatcher.cc:498-621) from the area walk on:
    vpMatched written as soon as a MapPoint is accepted.  slot_query: -2 taken, -1 free."""
    _chk(flip)
    s = np.array(slot_query, np.int32).copy()
    thr = float(f32(f32(TH_LOW) * f32(ratio)))
    if flip == "sim3.accept:double":
        thr = float(TH_LOW) * float(f32(ratio))

    def choose(q, blocked):
        lvl = int(Q.pred_level[q])
        r = f32(f32(th) * F.scale[lvl])
        lo, hi = _level_window(lvl, flip, "sim3.level")
        bd, bi = 256, -1
        for idx in features_in_area(F, Q.u[q], Q.v[q], r, flip=flip):
            if blocked(idx):
                continue
            o = int(F.kp_octave[idx])
            if o < lo or o > hi:
                continue
            d = dist(Q.desc[q], F.desc[idx])
            if d <= bd if flip == "sim3.tie" else d < bd:
                bd, bi = d, idx
        return bi if (float(bd) < thr if flip == "sim3.accept" else float(bd) <= thr) else -1

    if flip == "sim3.taken":
        # the wrong rule has no sequential form: iterate it as the kernel's rounds would (every MapPoint
        # against the lowest-indexed claimant of each slot in the previous round) until nothing changes
        best = [-1] * Q.n
        for _ in range(2 * Q.n + 4):
            claim = {}
            for q, b in enumerate(best):
                if b >= 0:
                    claim[b] = min(claim.get(b, q), q)
            new = [choose(q, lambda idx: s[idx] != -1 or claim.get(idx, q) != q) if Q.valid[q] else -1
                   for q in range(Q.n)]
            if new == best:
                break
            best = new
        for q, b in enumerate(best):
            if b >= 0:
                s[b] = q
        return sum(1 for b in best if b >= 0), s
    n = 0
    for q in range(Q.n):
        if not Q.valid[q]:
            continue
        bi = choose(q, (lambda idx: False) if flip == "sim3.taken:never" else (lambda idx: s[idx] != -1))
        if bi >= 0:
            s[bi] = q
            n += 1
    return n, s


def search_by_sim3(F1, F2, Q12, Q21, th, flip=None):
    """ORBmatcher::SearchBySim3 (ref:src/ORBmatcher.cc:1696-1939) from the area walk on: each direction's
    strict-'<' minimum from INT_MAX, accepted iff <= TH_HIGH; the mutual pairs in KF1 order."""
    _chk(flip)

    def direction(F, Q):
        out = [-1] * Q.n
        for q in range(Q.n):
            if not Q.valid[q]:
                continue
            lvl = int(Q.pred_level[q])
            r = f32(f32(th) * F.scale[lvl])
            bd, bi = 2147483647, -1
            for idx in features_in_area(F, Q.u[q], Q.v[q], r, flip=flip):
                o = int(F.kp_octave[idx])
                if o < lvl - 1 or o > lvl:
                    continue
                d = dist(Q.desc[q], F.desc[idx])
                if d < bd:
                    bd, bi = d, idx
            if bd < TH_HIGH if flip == "bysim3.accept" else bd <= TH_HIGH:
                out[q] = bi
        return out
    m1, m2 = direction(F2, Q12), direction(F1, Q21)
    m12 = [(i2 if i2 >= 0 and (m2[i2] == i1 or flip == "bysim3.mutual") else -1) for i1, i2 in enumerate(m1)]
    return sum(1 for x in m12 if x >= 0), np.array(m12, np.int32)


def search_for_initialization(F1, F2, prev, window=100, nn=0.9, ori=True, flip=None):
    """ORBmatcher::SearchForInitialization (ref:src/ORBmatcher.cc:735-878): (nmatches, vnMatches12, prev)."""
    _chk(flip)
    INT_MAX = 2147483647
    n1, n2 = F1.n, F2.n
    m12 = [-1] * n1
    md = [INT_MAX] * n2
    m21 = [-1] * n2
    hist = [[] for _ in range(HISTO)]
    nm = 0
    lv = (-1, -1) if flip == "init.level0:f2" else (0, 0)
    for i1 in range(n1):
        if F1.kp_octave[i1] > 0 and flip != "init.level0":
            continue
        cand = features_in_area(F2, prev[i1, 0], prev[i1, 1], float(window), lv[0], lv[1], flip=flip)
        if not cand:
            continue
        b1 = b2 = INT_MAX
        bi = -1
        for i2 in cand:
            d = dist(F1.desc[i1], F2.desc[i2])
            if md[i2] < d if flip == "init.md" else md[i2] <= d:
                continue
            if d < b1:
                b1, b2, bi = d, b1, i2
            elif d < b2 and not (flip == "init.top2" and d == b1):
                b2 = d
        r1, r2 = float(f32(b1)), float(f32(f32(b2) * f32(nn)))
        if (b1 < TH_LOW if flip == "init.accept" else b1 <= TH_LOW) and \
                (r1 <= r2 if flip == "init.accept:ratio" else r1 < r2):
            if m21[bi] >= 0:
                m12[m21[bi]] = -1
                nm -= 1
            m12[i1] = bi
            m21[bi] = i1
            md[bi] = b1
            nm += 1
            if ori:
                hist[rot_bin(F1.kp_angle[i1], F2.kp_angle[bi], flip)].append(i1)
    if ori:
        if flip == "init.steal_hist":
            hist = [[i1 for i1 in h if m12[i1] >= 0] for h in hist]
        keep = three_maxima([len(h) for h in hist], flip)
        for i in range(HISTO):
            if i in keep:
                continue
            for i1 in hist[i]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nm -= 1
    p = np.array(prev, np.float32).copy()
    for i1 in range(n1):
        if m12[i1] >= 0:
            p[i1] = (F2.kp_x[m12[i1]], F2.kp_y[m12[i1]])
    return nm, np.array(m12, np.int32), p
