"""Hand-built boundary fixtures for the two stereo matchers: stereo.hip (Frame::ComputeStereoMatches) and
triang.hip's k_stereo_fisheye (Frame::ComputeStereoFishEyeMatches); DESIGN.md, "Matcher decisions".  Each case
puts named decisions of the reference on both sides of equality, or straddles a size at which a kernel changes
shape.  No RNG (but for the two hand cases that tests/test_stereo.py had before), bits(k) descriptors so that a
distance is a difference of two small integers, and every rounding fact a case rests on is asserted here in
float32.

Images are column profiles.  Every left level is the constant grey A0; a right level is A0 too but for the strips
written by Scene.strip, which takes the eleven SADs that the 11 x 11 block match is to find for incR = -5..5 and
writes the one image row that gives exactly these (and checks them).  A case can therefore say "the SADs are
[.., 30, 10, 10, 30, ..]: the first minimum is offset -1".

tests/test_stereo_boundaries.py proves on the CPU that every case is discriminating (the Python restatement with
that one decision flipped leaves the oracle); tests/test_stereo_boundaries_gpu.py runs the kernels on them."""
from dataclasses import dataclass, replace

import numpy as np

from orb_slam3_comments_ghr_amd import stereo as st
from orb_slam3_comments_ghr_amd.frames import KB8_TRIANG, kb8_project, scale_factors
from tests.matcher_boundary_fixtures import bits, down, up

f32 = np.float32
A0 = 100   # every left pixel, and every right pixel outside a strip
MBF = 47.9  # the hand cases'


@dataclass
class Case:
    name: str
    kind: str      # stereo | fish
    frame: object  # st.StereoFrame | st.FishEyeStereoFrame
    flips: tuple   # the decisions (pyref_stereo.FLIPS) the case discriminates; () for the far side of one, and
                   # for the cases that straddle a kernel's structure
    structure: bool = False  # named after the kernel structure it straddles: may exceed 64 keypoints / 64 x 96 pixels

    @property
    def id(self):
        return f"{self.kind}-{self.name}"


# ---- float facts (numpy float32 scalars; each asserted where it is used, these are shared)

TH_FACTOR = f32(1.5) * f32(1.4)
assert TH_FACTOR == f32(2.1) and float(TH_FACTOR) == 2.0999999046325684
assert f32(TH_FACTOR * f32(10)) == 21.0 and f32(TH_FACTOR * f32(20)) == 42.0  # so a SAD of 21 sits on '<' at median 10
assert f32(TH_FACTOR * f32(30)) < 63.0                                         # (63 is removed either way at median 30)
S3 = scale_factors(3)
I3 = (f32(1.0) / S3).astype(f32)
assert S3[1] == f32(1.2) and S3[2] == f32(f32(1.2) * f32(1.2))


def cround(v):
    return int(np.floor(float(v) + 0.5))


def vee(k0, lo=10, step=10):
    """SADs with the one minimum `lo` at incR = k0 - 5 and equal slopes (deltaR = 0)."""
    return [lo + step * abs(k - k0) for k in range(11)]


class Scene:
    """One stereo frame under construction: constant left levels, right levels with strips, keypoints."""

    def __init__(self, rows=64, cols=96, n_levels=1, mbf=16.0, mb=2.0, shapes=None):
        self.scale = scale_factors(n_levels)
        self.inv = (f32(1.0) / self.scale).astype(f32)
        self.mbf, self.mb = mbf, mb
        if shapes is None:  # level sizes as ORBextractor's cvRound(size / scale)
            shapes = [((cround(rows * i), cround(cols * i)),) * 2 for i in self.inv]
        self.L = [np.full(s[0], A0, np.uint8) for s in shapes]
        self.R = [np.full(s[1], A0, np.uint8) for s in shapes]
        self.used = [np.zeros(s[1], bool) for s in shapes]
        self.kl, self.kr = [], []

    def left(self, x, y, octave=0, k=0):
        self.kl.append((x, y, octave, bits(k)))
        return len(self.kl) - 1

    def right(self, x, y, octave=0, k=5):
        self.kr.append((x, y, octave, bits(k)))
        return len(self.kr) - 1

    def strip(self, pv, pr, sads, level=0):
        """Row pv of the right level, columns pr - 10 .. pr + 10: the SAD of the constant left patch against the
        patch centred (pv, pr + incR) is sads[incR + 5].  The patch rows and strip columns must be free."""
        S = [int(s) for s in sads]
        assert len(S) == 11
        R = self.R[level]
        assert pv - 5 >= 0 and pv + 5 < R.shape[0] and pr - 10 >= 0 and pr + 10 < R.shape[1], (pv, pr, R.shape)
        box = (slice(pv - 5, pv + 6), slice(pr - 10, pr + 11))
        assert not self.used[level][box].any(), "strips overlap"
        self.used[level][box] = True
        # window sums: S[k] = sum g[k .. k + 10], so g[k + 11] = g[k] + S[k + 1] - S[k]
        g = np.zeros(21, np.int64)
        for k in range(10):
            g[k] = max(0, S[k] - S[k + 1])
        slack = S[0] - int(g[:10].sum())
        assert slack >= 0, "the first SAD is too small for the descent that follows"
        g[:11] += slack // 11
        g[10] += slack % 11
        for k in range(10):
            g[k + 11] = g[k] + S[k + 1] - S[k]
        assert (g >= 0).all() and (g <= 255 - A0).all(), g
        R[pv, pr - 10:pr + 11] = A0 + g
        assert sads_at(self.L[level], R, pv, pr, pr) == S
        return self

    def probe(self, uL, vL, uR, sads, level=0, yr=None, oct_r=None, kl=0, kr=5, strip=True):
        """A left keypoint, the right keypoint it is to find, and the strip under that one at the left level
        (strip=False where the patch leaves the image and is never read)."""
        self.left(uL, vL, level, kl)
        self.right(uR, vL if yr is None else yr, level if oct_r is None else oct_r, kr)
        if strip:
            self.strip(cround(f32(f32(vL) * self.inv[level])), cround(f32(f32(uR) * self.inv[level])), sads,
                       level)
        return self

    def frame(self):
        def col(kps, i, dt):
            return np.array([k[i] for k in kps], dt)
        dl = np.stack([k[3] for k in self.kl]) if self.kl else np.zeros((0, 32), np.uint8)
        dr = np.stack([k[3] for k in self.kr]) if self.kr else np.zeros((0, 32), np.uint8)
        return st.StereoFrame(desc=dl, x=col(self.kl, 0, f32), y=col(self.kl, 1, f32), octave=col(self.kl, 2, np.int32),
                              desc_r=dr, xr=col(self.kr, 0, f32), yr=col(self.kr, 1, f32),
                              octave_r=col(self.kr, 2, np.int32), left=st.ImagePyramid(self.L),
                              right=st.ImagePyramid(self.R), scale=self.scale, mb=self.mb, mbf=self.mbf)


def sads_at(L, R, pv, pu, pr):
    """The eleven SADs of the left patch centred (pv, pu) against the right patches centred (pv, pr - 5 .. pr + 5)."""
    IL = L[pv - 5:pv + 6, pu - 5:pu + 6].astype(np.int64)
    return [int(np.abs(IL - R[pv - 5:pv + 6, pr + i - 5:pr + i + 6].astype(np.int64)).sum()) for i in range(-5, 6)]


def one(name, flips, uL=20.0, vL=16.0, uR=14.0, sads=None, **kw):
    """A frame of one probe.  maxD = 16 / 2 = 8 unless mbf / mb say otherwise."""
    scene = {k: kw.pop(k) for k in ("rows", "cols", "n_levels", "mbf", "mb", "shapes") if k in kw}
    return Case(name, "stereo", Scene(**scene).probe(uL, vL, uR, vee(5) if sads is None else sads, **kw).frame(), flips)


def several(name, flips, minima):
    """One probe per minimum SAD, 11 rows apart (no probe is another's candidate): the accepted SADs are `minima`."""
    S = Scene()
    assert len(minima) <= 5
    for i, m in enumerate(minima):
        S.probe(20.0, 5.0 + 11 * i, 14.0, vee(5, lo=m, step=10 if m < 100 else 100))
    return Case(name, "stereo", S.frame(), flips)


# ---- the hand cases of tests/test_stereo.py

def hand_frame(noisy):
    """40 x 80 single-level pair.  Columns < 44 of the right image are the left image shifted 4 px
    (plus +-6 noise when `noisy`); columns >= 44 are identical and mirror-symmetric about column 60.
    Keypoints (16, 10), (22, 20), (28, 30) match right keypoints 4 px to the left; keypoint (60, 20)
    matches (60, 20) at zero disparity (noisy case only)."""
    rng = np.random.default_rng(4242)
    L = rng.integers(0, 256, (40, 80)).astype(np.int64)
    for k in range(1, 16):
        L[:, 60 + k] = L[:, 60 - k]
    R = L.copy()
    R[:, :44] = L[:, 4:48] + (rng.integers(-6, 7, (40, 44)) if noisy else 0)
    L, R = (np.clip(a, 0, 255).astype(np.uint8) for a in (L, R))
    u = [16.0, 22.0, 28.0] + ([60.0] if noisy else [])
    v = [10.0, 20.0, 30.0] + ([20.0] if noisy else [])
    ur = [x - 4 for x in u[:3]] + ([60.0] if noisy else [])
    desc = rng.integers(0, 256, (len(u), 32), dtype=np.uint8)
    one = st.ImagePyramid
    return st.StereoFrame(desc=desc, x=u, y=v, octave=np.zeros(len(u)), desc_r=desc.copy(), xr=ur, yr=v,
                          octave_r=np.zeros(len(u)), left=one([L]), right=one([R]), scale=[1.0], mbf=MBF)


def check_hand(res):
    """noise-free: every SAD minimum is 0, so the median is 0 and `dist < 0` never holds — the
    reference's cut removes every match.  Noisy: the three shifted matches land within half a pixel
    of 4 px, the zero-disparity one takes the 0.01 clamp (bestuR = uL - 0.01 in double)."""
    (ur0, d0, n0), (ur1, d1, n1) = res
    assert n0 == 0 and (ur0 == -1).all() and (d0 == -1).all()
    assert n1 == 4
    np.testing.assert_allclose(ur1[:3], [12, 18, 24], atol=0.5)
    np.testing.assert_array_equal(d1[:3], (np.float32(MBF) / (np.float32([16, 22, 28]) - ur1[:3])).astype(np.float32))
    assert ur1[3] == np.float32(60.0 - 0.01) and d1[3] == np.float32(np.float32(MBF) / np.float32(0.01))


# ---- ComputeStereoMatches: the decisions

def _row_table_cases():
    out = []
    # a right keypoint of octave 1 at y = 10: r = 2.4, rows 7 .. 13; with r = 2 (the left keypoint's octave 0, or
    # no scale at all) they end at 12.  The left keypoint on row 13 finds it only under the reference.
    assert int(np.ceil(f32(f32(10) + f32(2) * S3[1]))) == 13 and int(np.ceil(f32(f32(10) + f32(2) * S3[0]))) == 12
    out.append(one("rows_radius", ("rows.radius", "rows.radius:one", "rows.span"), vL=13.0, yr=10.0, oct_r=1,
                   n_levels=3))
    # y = 10.5, r = 2: rows floor(8.5) = 8 .. ceil(12.5) = 13; truncation ends at 12
    out.append(one("rows_span_ceil", ("rows.span",), vL=13.0, yr=10.5))
    out.append(one("rows_span_floor", (), vL=8.0, yr=10.5))
    out.append(one("rows_span_below", (), vL=7.0, yr=10.5))
    # y = 10, r = 2: rows 8 .. 12, the last one included
    out.append(one("rows_span_last", ("rows.span:exclusive",), vL=12.0, yr=10.0))
    out.append(one("rows_span_past", (), vL=13.0, yr=10.0))
    # octave 1 at y = 2: rows floor(-0.4) = -1 .. 5, indexed on 0 .. 5.  A left keypoint above row 5 cannot pass the
    # patch guard, so row 5 is the one row on which the clipped band shows.
    assert int(np.floor(f32(f32(2) - f32(2) * S3[1]))) == -1 and int(np.ceil(f32(f32(2) + f32(2) * S3[1]))) == 5
    out.append(one("rows_clip_top", ("rows.clip",), vL=5.0, yr=2.0, oct_r=1, n_levels=3))
    # octave 2 at y = 61.5 of 64 rows: rows 58 .. 65, indexed on 58 .. 63; the left keypoint of level 1 on the last
    # row has its patch at row 53 of a level-1 image that is as tall as level 0 here
    assert int(np.floor(f32(f32(61.5) - f32(2) * S3[2]))) == 58 and int(np.ceil(f32(f32(61.5) + f32(2) * S3[2]))) == 65
    assert f32(f32(63) * I3[1]) == f32(52.5)  # (rounds to 53; the patch of row 52 would hold the strip too)
    out.append(one("rows_clip_bottom", ("rows.clip",), uL=24.0, vL=63.0, uR=18.0, yr=61.5, level=1, oct_r=2, n_levels=3,
                   shapes=[((64, 96), (64, 96))] * 3))
    # vRowIndices[vL] truncates: 16.7 is row 16, which the right keypoint's rows 12 .. 16 reach; row 17 they do not
    assert int(f32(16.7)) == 16 and cround(f32(16.7)) == 17
    out.append(one("stereo_row", ("stereo.row",), vL=16.7, yr=14.0))
    return out


def _coarse_cases():
    out = []
    # maxD = 8, uL = 30: the window is [22, 30].  At uR = minU the refined position has to come back inside
    # disparity < maxD (the minimum at incR = +2: disparity 6); at uR = maxU it moves left (incR = -2: disparity 2).
    assert f32(f32(30) - f32(f32(16) / f32(2))) == 22.0
    out.append(one("window_min", ("stereo.window",), uL=30.0, uR=22.0, sads=vee(7)))
    out.append(one("window_below", (), uL=30.0, uR=down(22.0), sads=vee(7)))
    out.append(one("window_max", ("stereo.window:max",), uL=30.0, uR=30.0, sads=vee(3)))
    out.append(one("window_above", (), uL=30.0, uR=up(30.0), sads=vee(3)))
    # octave +-1: the left keypoint of level 0 has a right keypoint of octave 1 at distance 10 and one of octave 2 at
    # distance 5 (maxD = 64); the left keypoint of level 2 one of octave 1 at 10 and one of octave 0 at 5
    S = Scene(n_levels=3, mbf=128.0)
    S.left(60.0, 16.0, 0, 0)
    S.right(14.0, 16.0, 1, 10), S.strip(16, 14, vee(4))
    S.right(40.0, 16.0, 2, 5), S.strip(16, 40, vee(6))
    out.append(Case("level_up", "stereo", S.frame(), ("stereo.level", "stereo.level:narrow")))
    S = Scene(n_levels=3, mbf=128.0)
    assert cround(f32(f32(72) * I3[2])) == 50 and cround(f32(f32(28.8) * I3[2])) == 20 and cround(f32(f32(60.5) * I3[2])) == 42
    S.left(72.0, 28.8, 2, 0)
    S.right(28.8, 28.8, 1, 10), S.strip(20, 20, vee(4), level=2)
    S.right(60.5, 28.8, 0, 5), S.strip(20, 42, vee(6), level=2)
    out.append(Case("level_down", "stereo", S.frame(), ("stereo.level", "stereo.level:narrow")))
    # bestDist starts at TH_HIGH and is accepted below 75: 60 and 74 match, 75 does not (whether 100 itself is a
    # candidate cannot show: nothing from 75 on is accepted; a start at TH_LOW is the wrong form that can: no
    # candidate).  The right keypoint is index 1: index 0, which bestIdxR starts at, stands where no strip fits.
    for d in (60, 74):
        S = Scene()
        S.right(8.0, 40.0, 0, 200)
        out.append(Case(f"dist_{d}", "stereo", S.probe(20.0, 16.0, 14.0, vee(5), kr=d).frame(), ("stereo.high",)))
    out.append(one("dist_75", ("stereo.accept",), kr=75))
    # two right keypoints at distance 5, 26 px apart: the lower index wins, wherever it stands
    for name, xs in (("tie", (14.0, 40.0)), ("tie_reversed", (40.0, 14.0))):
        S = Scene(mbf=128.0)
        S.left(60.0, 16.0)
        S.right(xs[0], 16.0), S.right(xs[1], 16.0)
        S.strip(16, 14, vee(4)), S.strip(16, 40, vee(6))
        out.append(Case(name, "stereo", S.frame(), ("stereo.tie",)))
    return out


def _block_cases():
    out = []
    # round(): half away from zero, on x * invScale.  x.5 with x even separates it from rint.  Level 0 (the factor is
    # 1): vL = 4.5 is patch row 5 (inside) not 4; uL = 90.5 of 96 columns is patch column 91 (outside) not 90;
    # uR0 = 20.5 is 21, where the minimum five columns on is incR = +4 and not the dropped +5.
    assert cround(f32(4.5) * I3[0]) == 5 and np.rint(f32(4.5) * I3[0]) == 4
    out.append(one("round_v", ("sad.round", "sad.inside"), vL=4.5, yr=5.0))
    out.append(one("round_u", ("sad.round",), uL=90.5, uR=84.0))
    out.append(one("round_r", ("sad.round",), uL=26.0, uR=20.5, sads=vee(9)))
    # level 1: 5.4f * (1 / 1.2f) is 4.5 exactly
    assert f32(f32(5.4) * I3[1]) == f32(4.5)
    out.append(one("round_v_level1", ("sad.round", "sad.inside"), uL=24.0, vL=5.4, uR=18.0, level=1, n_levels=3))
    # the left keypoint's level serves both images: uR0 = 24 of an octave-1 right keypoint is column 24 of level 0,
    # not column 20 of level 1 (a constant image: first minimum at -5, dropped)
    out.append(one("sad_level", ("sad.level",), uL=30.0, uR=24.0, oct_r=1, n_levels=3))
    # endu = scaleduR0 + 11 >= cols: of 96 columns, 85 is dropped with its strip inside the image, 84 is kept
    out.append(one("bound_at", ("sad.bound",), uL=88.0, uR=85.0))
    out.append(one("bound_inside", (), uL=88.0, uR=84.0))
    # the patch guard, each observable term just inside and just outside (scaleduL - w >= 0 cannot show: uR0 <= uL
    # puts the strip outside first; scaleduR0 + L + w < cols cannot: endu >= cols is stricter)
    out.append(one("inside_top", ("sad.inside",), vL=5.0))
    out.append(one("outside_top", (), vL=4.0, yr=5.0, strip=False))
    tall, short = ((64, 96), (65, 96)), ((64, 96), (63, 96))
    out.append(one("inside_bottom", ("sad.inside:bottom",), vL=58.0, shapes=[tall]))
    out.append(one("outside_bottom", (), vL=59.0, yr=58.0, shapes=[tall], strip=False))
    out.append(one("inside_bottom_right", ("sad.inside:bottom_r",), vL=57.0, shapes=[short]))
    out.append(one("outside_bottom_right", (), vL=58.0, yr=57.0, shapes=[short], strip=False))
    out.append(one("inside_right", ("sad.inside:right",), uL=90.0, uR=84.0))
    out.append(one("outside_right", (), uL=91.0, uR=84.0))
    out.append(one("inside_strip", ("sad.inside:strip",), uL=16.0, uR=10.0))
    S = Scene()
    S.left(15.0, 16.0), S.right(9.0, 16.0)
    out.append(Case("outside_strip", "stereo", S.frame(), ()))
    # SADs 10 at incR = -2 and 0: the first minimum is -2 (deltaR = 0.25: 12.25; the last would give 13.75).  Two
    # equal minima next to each other cannot show: the parabola puts -1 + 0.5 and 0 - 0.5 on the same spot.
    out.append(one("first_minimum", ("sad.first",), sads=[60, 50, 40, 10, 20, 10, 40, 50, 60, 70, 80]))
    out.append(one("first_minimum_adjacent", (), sads=[60, 50, 40, 30, 10, 10, 30, 40, 50, 60, 70]))
    # a best offset of -5 or +5 is dropped, -4 and +4 are kept
    out.append(one("edge_low", ("sad.edge",), uL=16.0, sads=vee(0)))
    out.append(one("edge_low_inside", (), uL=16.0, sads=vee(1)))
    out.append(one("edge_high", ("sad.edge:hi",), sads=vee(10)))
    out.append(one("edge_high_inside", (), sads=vee(9)))
    return out


def _tail_cases():
    out = []
    # disparity 0 is clamped to 0.01 (bestuR = uL - 0.01 in double), -1 is dropped, maxD = 8 is dropped, and the
    # next float below 8 (deltaR = 2 / 76 to the right) is kept
    out.append(one("disparity_zero", ("disp.min", "disp.clamp"), uL=30.0, uR=30.0))
    out.append(one("disparity_negative", ("disp.min:open",), uL=30.0, uR=30.0, sads=vee(6)))
    out.append(one("disparity_max", ("disp.max",), uL=30.0, uR=22.0))
    out.append(one("disparity_below_max", (), uL=30.0, uR=22.0, sads=[60, 50, 40, 30, 30, 10, 28, 40, 50, 60, 70]))
    return out


def _median_cases():
    out = []
    # accepted counts 0 .. 4; element size / 2 is the upper middle of an even count; '<' against 2.1f * median
    out.append(several("median_m1", (), [10]))
    out.append(several("median_m2", ("median.index",), [30, 10]))        # median 30: both kept
    out.append(several("median_m3_cut", ("median.cut",), [10, 21, 10]))  # thDist 21.0: 21 is removed
    out.append(several("median_m3_keep", (), [10, 20, 10]))
    out.append(several("median_m4", ("median.index",), [50, 10, 30, 20]))  # median 30: 50 kept (at 20 it would go)
    out.append(several("median_equal", (), [10, 10, 10]))                # nothing is removed
    out.append(one("median_empty", (), kr=90))                           # no accepted match: nothing to remove
    # the radix select's first pass has bins of 128: 127 | 128, the median first and last in its bin
    out.append(several("bins_128_first", (), [128, 127, 128]))
    out.append(several("bins_127_last", (), [127, 128, 127]))
    out.append(several("bins_255_last", (), [256, 128, 255]))
    out.append(several("bins_three", (), [300, 100, 128, 127]))  # median 128: 300 > 268.8 is removed
    return out


# ---- ComputeStereoMatches: the kernels' structure

def row_case(name, n_cand, strips, lefts, flips=()):
    """One image row with n_cand right keypoints in every left keypoint's window (maxD = 80).  All but the `strips`
    = {list position: 0 | 1 | 2} stand at uR = 8 with descriptor bits(70), where the strip would leave the image: a
    left keypoint that takes one of them gets no match.  The three strips are centred at columns 25, 47 and 69 and
    differ in their offset.  `lefts` = [(k of the left descriptor, {list position: k of that right descriptor})]:
    all left keypoints stand at (85, 16)."""
    S = Scene(mbf=160.0)
    centre = (25.0, 47.0, 69.0)
    rk = {}
    for k, pos in lefts:
        for p, v in pos.items():
            assert rk.setdefault(p, v) == v
    assert set(rk) == set(strips)
    for p in range(n_cand):
        S.right(centre[strips[p]] if p in strips else 8.0, 16.0, 0, rk.get(p, 70))
    for s in set(strips.values()):
        S.strip(16, int(centre[s]), vee(3 + s))
    for k, _ in lefts:
        S.left(85.0, 16.0, 0, k)
    return Case(name, "stereo", S.frame(), flips, structure=True)


def _match_structure_cases():
    """k_stereo_match: 64 lanes stride over a row's candidates and a wave minimum of (dist << 24 | index) picks the
    winner; four waves per workgroup.  The in-window losers of lower index have a higher distance (30 .. 70 from
    the left descriptors bits(9) .. bits(41)) and must lose to it."""
    out = []
    # 63 candidates (n = 3): winners at list positions 0, 62 and 31
    out.append(row_case("row_63", 63, {0: 0, 62: 1, 31: 2}, [(9, {0: 10}), (31, {62: 30}), (21, {31: 20})]))
    # 64 candidates (n = 4): winners at 0, 63 and 32; 0 and 63 tie for the fourth (the ends of one pass)
    out.append(row_case("row_64", 64, {0: 0, 63: 1, 32: 2},
                        [(9, {0: 10}), (41, {32: 40}), (21, {63: 20}), (15, {0: 10, 63: 20})], ("stereo.tie",)))
    # 65 candidates (n = 5): winners at 0, 63 and 64 (the second pass's only candidate); ties between 0 and 64 (one
    # lane, two passes) and between 63 and 64 (neighbouring lanes... of different passes)
    out.append(row_case("row_65", 65, {0: 0, 63: 1, 64: 2},
                        [(9, {0: 10}), (41, {63: 40}), (21, {64: 20}), (15, {0: 10, 64: 20}), (30, {63: 40, 64: 20})],
                        ("stereo.tie",)))
    # 129 candidates (n = 5): winners at 128 (the third pass's only candidate), 64 and 0; ties between 0 and 64 and
    # between 64 and 128 (one lane, passes one to three)
    out.append(row_case("row_129", 129, {0: 0, 64: 1, 128: 2},
                        [(41, {128: 40}), (15, {0: 10, 64: 20}), (30, {64: 20, 128: 40}), (21, {64: 20}),
                         (9, {0: 10})], ("stereo.tie",)))
    return out


def rows_case(height, probes, extra):
    """A narrow one-level image of `height` rows: probes (left row = right row) far enough apart not to see each other,
    and right keypoints without a partner on the rows `extra` (the image's first and last among them), whose counts
    every later row's start carries."""
    S = Scene(rows=height, cols=32)
    for y in extra:
        S.right(15.0, float(y), 0, 200)
    for y in probes:
        S.probe(20.0, float(y), 15.0, vee(4 + y % 3))
    return Case(f"rows_{height}", "stereo", S.frame(), (), structure=True)


def _rows_structure_cases():
    """k_stereo_rows: 1024 threads scan the per-row counts; a thread's segment is one row up to 1024 rows and two
    from 1025 on."""
    return [rows_case(1024, (6, 500, 511, 1018), (0, 100, 101, 700, 1023)),
            rows_case(1025, (6, 500, 511, 1019), (0, 100, 101, 700, 1023, 1024))]


def tall_frame(height):
    """The row limit of k_stereo_rows' LDS counters: 8192 rows run, 8193 are refused."""
    return rows_case(height, (6, 4096, height - 6), (0, height - 1)).frame


# ---- ComputeStereoFishEyeMatches

FISH_X = np.array([0.3, -0.2, 3.0])  # the one 3-D point every keypoint pair of a fish case triangulates to


def block(q, n):
    """Query q's descriptor is block(q, 32): the 32 bits of block q.  A right row block(q, n) is at distance 32 - n
    from query q and 32 + n from every other query; the all-zero row is at 32 from every query."""
    b = np.zeros(256, np.uint8)
    b[32 * q:32 * q + n] = 1
    return np.packbits(b)


def fish(name, flips, left, right, mono_left=0, mono_right=0, oct_left=None, oct_right=None, cam_right=None,
         left_dy=0.0):
    """left / right: one descriptor per frame row, the mono rows first.  Every left keypoint is the projection of
    FISH_X (moved down by left_dy px), every right keypoint its projection into the right camera of a 10 cm rig, so
    any pair triangulates alike."""
    cam = KB8_TRIANG.astype(f32)
    cam_r = cam.copy() if cam_right is None else np.asarray(cam_right, f32)
    a = np.deg2rad(1.5)
    Rlr = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    tlr = np.array([0.10, 0.002, -0.001])
    pl = kb8_project(cam.astype(np.float64), FISH_X[None])[0] + [0.0, left_dy]
    pr = kb8_project(cam_r.astype(np.float64), ((FISH_X - tlr) @ Rlr)[None])[0]
    nl, nr = len(left), len(right)
    F = st.FishEyeStereoFrame(
        kp_left=np.tile(pl, (nl, 1)).astype(f32), oct_left=np.zeros(nl, np.int32) if oct_left is None else oct_left,
        desc_left=np.stack(left), mono_left=mono_left, kp_right=np.tile(pr, (nr, 1)).astype(f32),
        oct_right=np.zeros(nr, np.int32) if oct_right is None else oct_right, desc_right=np.stack(right),
        mono_right=mono_right, level_sigma2=(S3 * S3).astype(f32), cam_left=cam, cam_right=cam_r,
        Rlr=Rlr.astype(f32), tlr=tlr.astype(f32))
    return Case(name, "fish", F, flips)


# the right camera at half the focal length, the left keypoint 6 px off the epipolar plane: the left reprojection
# error squared lies between 5.991 sigma2[0] and 5.991 sigma2[2], the right one below 5.991 sigma2[0]
HALF_F = KB8_TRIANG.astype(f32) * np.array([0.5, 0.5, 1, 1, 1, 1, 1, 1], f32)
OCTAVE_DY = 6.0


def _fish_decision_cases():
    out = []
    q = bits(0)
    # second equal to first: 6, 6, 20 fails the ratio (6 < 4.2 is false); not counted, 6 < 14 would pass
    out.append(fish("second_equals_first", ("fish.second",), [q], [bits(6), bits(6), bits(20)]))
    # 7 against 10 * 0.7: the double product is 7.0 exactly (asserted), so '<' fails; 6 passes
    assert float(f32(10)) * 0.7 == 7.0
    out.append(fish("ratio_equal", ("fish.ratio",), [q], [bits(7), bits(10)]))
    out.append(fish("ratio_below", (), [q], [bits(6), bits(10)]))
    out.append(fish("ratio_zero", ("fish.ratio",), [q], [bits(0), bits(0)]))
    # one right stereo row (after two mono rows): nothing is matched
    out.append(fish("one_right_row", ("fish.two", "fish.mono:right"), [q], [bits(40), bits(50), bits(5)], mono_right=2))
    out.append(fish("no_right_row", (), [q], [bits(40), bits(50)], mono_right=2))
    # two mono rows on the left that would match if they asked; two on the right that would be nearer
    out.append(fish("mono_left", ("fish.mono",), [bits(0), bits(1), q], [bits(2), bits(20)], mono_left=2))
    out.append(fish("mono_right", ("fish.mono:right",), [q], [bits(0), bits(50), bits(3), bits(20)], mono_right=2))
    # sigma1 is the left octave's (2: 2.0736), sigma2 the right's (0: 1)
    out.append(fish("octave_left_coarse", ("fish.octave",), [q], [bits(2), bits(20)], oct_left=np.array([2], np.int32),
                    cam_right=HALF_F, left_dy=OCTAVE_DY))
    out.append(fish("octave_both_fine", (), [q], [bits(2), bits(20)], cam_right=HALF_F, left_dy=OCTAVE_DY))
    # queries 0 and 5 (two workgroups) both accept right stereo row 3; the four between them tie at 100 and fail.
    # One mono row on each side: the frame rows are 1 and 6, and 4.
    left = [bits(200), bits(0), bits(140), bits(140), bits(140), bits(140), bits(1)]
    right = [bits(200), bits(40), bits(40), bits(40), bits(0), bits(40)]
    out.append(fish("last_query_wins", ("fish.last",), left, right, mono_left=1, mono_right=1))
    return out


def fish_rows(name, n_right, queries, mono_left=2, mono_right=3):
    """n_right right stereo rows, all zero but for the rows a query names: queries[q] = {stereo row: distance}."""
    right = [block(0, 0) for _ in range(mono_right + n_right)]
    named = set()
    for q, rows in enumerate(queries):
        for r, d in rows.items():
            assert r not in named and 0 <= r < n_right and d < 32
            named.add(r)
            right[mono_right + r] = block(q, 32 - d)
    left = [block(7, 32)] * mono_left + [block(q, 32) for q in range(len(queries))]
    assert len(queries) <= 7
    return replace(fish(name, (), left, right, mono_left, mono_right), structure=True)


def near(a, b):
    """Two queries' rows: first neighbour at row a, second at row b.  7 and 9 fail the ratio (7 < 6.3 is false) and
    would pass with any later second (32); 6 and 10 pass (6 < 7) and would fail with the first taken twice."""
    return {a: 7, b: 9}, {a + 2: 6, b + 2: 10}


def _fish_structure_cases():
    """k_stereo_fisheye: 64 lanes stride over the right stereo rows (row j is lane j % 64), each keeps its own first
    and second, and a six-step butterfly merges them: the loser's first against the winner's second."""
    out = []
    out.append(fish_rows("rows_2", 2, [{0: 7, 1: 9}]))
    out.append(fish_rows("rows_2_pass", 2, [{0: 6, 1: 10}]))
    out.append(fish_rows("rows_2_second_first", 2, [{1: 7, 0: 9}]))
    out.append(fish_rows("rows_2_equal", 2, [{0: 6, 1: 6}]))
    out.append(fish_rows("rows_3", 3, [{0: 7, 2: 9}]))
    out.append(fish_rows("rows_3_pass", 3, [{2: 6, 1: 10}]))
    # 64 rows: one pass, the last lane; lanes that meet at the first (j ^ 1) and the last (j ^ 32) butterfly step
    out.append(fish_rows("rows_64", 64, [*near(0, 59), *near(11, 10), *near(20, 52), {63: 7, 31: 9}]))
    # 65 rows: row 64 is lane 0's second row
    out.append(fish_rows("rows_65", 65, [{0: 7, 64: 9}, {5: 6, 6: 6}, {10: 6, 12: 10}]))
    out.append(fish_rows("rows_65_first", 65, [{64: 7, 1: 9}]))
    out.append(fish_rows("rows_65_pass", 65, [{64: 6, 63: 10}]))
    # 129 rows: first and second in one lane (j and j + 64, either order), in lanes j ^ 1 and j ^ 32, a tie for first
    # between rows 1 and 64 (second equal to first: no match), row 128 alone in the third pass
    out.append(fish_rows("rows_129", 129, [*near(5, 69), {73: 7, 9: 9}, {20: 7, 21: 9}, {30: 7, 62: 9}, {1: 6, 64: 6},
                                          {128: 6, 0: 10}], mono_right=1))
    out.append(fish_rows("rows_129_tail", 129, [{127: 7, 128: 9}, {2: 6, 66: 6}], mono_left=0, mono_right=0))
    out.append(fish_rows("rows_129_tail_first", 129, [{128: 7, 64: 9}], mono_left=0, mono_right=0))
    return out


def _build():
    out = [Case("hand_median_zero", "stereo", hand_frame(False), ()),
           Case("hand_clamp", "stereo", hand_frame(True), ("disp.min", "disp.clamp"))]
    out += _row_table_cases() + _coarse_cases() + _block_cases() + _tail_cases() + _median_cases()
    out += _match_structure_cases() + _rows_structure_cases()
    out += _fish_decision_cases() + _fish_structure_cases()
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _build()


def of_kind(kind):
    return [c for c in CASES if c.kind == kind]


def sizes(case):
    """(keypoints on the larger side, level-0 rows, level-0 columns) of a stereo case; fish: rows of the larger side."""
    F = case.frame
    if case.kind == "fish":
        return (max(len(F.kp_left), len(F.kp_right)),)
    return (max(F.n, F.n_right),) + F.left.levels[0].shape


# ---- the same frame in another form (tests/test_stereo_boundaries_gpu.py)

def bordered(F, border=3, fill=7):
    """The frame with every level a view into a larger buffer (row step != cols), as the reference's levels are; the
    border is no grey of the image, so a wrong row step shows."""
    def pyr(P):
        out = []
        for lv in P.levels:
            buf = np.full((lv.shape[0] + 2 * border, lv.shape[1] + 2 * border), fill, np.uint8)
            buf[border:border + lv.shape[0], border:border + lv.shape[1]] = lv
            out.append(buf[border:border + lv.shape[0], border:border + lv.shape[1]])
        return st.ImagePyramid(out)
    return replace(F, left=pyr(F.left), right=pyr(F.right))


def without_left(F):
    """The frame with no left keypoint: nothing is packed for it, and it matches nothing."""
    return replace(F, desc=F.desc[:0], x=F.x[:0], y=F.y[:0], octave=F.octave[:0])
