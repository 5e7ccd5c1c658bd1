"""The OptimizeSim3 fixtures shared by tests/test_sim3opt.py, tests/test_sim3opt_gpu.py and
tools/sim3opt_margins.py: seeds of ``synth_sim3_problem`` chosen on the CPU so that the guard conditions
hold for tests/pyref_sim3opt.py alone and for 16 replicas nudged by +-1 ulp (every classified chi2 outside
th2 (1 +- 1e-3), the discrete outcome identical), at the reference's iteration counts and at
max_iterations = 1.  A seed that violates a guard is replaced here, never excluded from a comparison.

ORIGINAL names the twelve fixtures the kernel arrived with; their tolerances (full_max / cap1_max of
profiles/sim3opt_margins.json) are maxima over those twelve alone.  Every later fixture belongs to one
group of GROUPS and is held to that group's own maxima.

No fixture mixes a pinhole and a KannalaBrandt8 camera: pyref's discrete outcome is not stable under the
+-1 ulp nudges on such a problem."""
from dataclasses import dataclass

import numpy as np

from orb_slam3_comments_ghr_amd import optimizer as O

N_REPLICAS = 16


@dataclass(frozen=True)
class Fixture:
    n_pairs: int
    fix_scale: bool
    seed: int
    outlier_frac: float = 0.1
    out_of_kf2_frac: float = 0.0
    cam1: tuple = ("pinhole",)   # (model, *arguments of O.pinhole_camera / O.kb8_camera)
    cam2: tuple = ("pinhole",)
    th2: float = 10.0
    noise_px: float = 1.0
    noise_m: float = 0.01
    zero_weights: bool = False   # both weight arrays set to 0 after synth_sim3_problem: every solve fails
    group: str = "original"


PINHOLE_B = ("pinhole", 380.0, 395.0, 330.0, 250.0)
KB8 = ("kb8",)
KB8_B = ("kb8", 210.0, 205.0, 262.0, 248.0, (2.0e-3, 1.0e-3, -1.5e-3, 1.0e-4))
LOW_NOISE = dict(noise_px=0.25, noise_m=0.002)  # at the default noise an 8192-pair problem has a chi2 within 1e-5 of th2

FIXTURES = {
    "m0_free": Fixture(0, False, 1000),
    "m0_fixed": Fixture(0, True, 1001),
    "m9_free": Fixture(9, False, 1018),
    "m9_fixed": Fixture(9, True, 1019),
    "m12_free": Fixture(12, False, 1024),
    "m12_fixed": Fixture(12, True, 1025),
    "m70_free": Fixture(70, False, 1140),
    "m70_fixed": Fixture(70, True, 1145),
    "m150_free": Fixture(150, False, 1304),
    "m150_fixed": Fixture(150, True, 1305),
    "m70_nokf2": Fixture(70, False, 2072, out_of_kf2_frac=0.2),
    "m70_kb8": Fixture(70, False, 3070, cam1=KB8, cam2=KB8),
    # two different cameras: a kernel or an adapter that exchanges them gives another pair_state
    "m70_cam_ab": Fixture(70, False, 50, cam2=PINHOLE_B, group="cameras"),
    "m70_cam_ba": Fixture(70, False, 50, cam1=PINHOLE_B, group="cameras"),
    "m70_kb8_ab": Fixture(70, False, 60, cam1=KB8, cam2=KB8_B, group="cameras"),
    # a th2 whose float, Huber delta and float delta^2 are all inexact
    "m70_th599": Fixture(70, False, 31, th2=5.99, group="th2"),
    # around one and two full chunks of 128 lanes
    "m127_free": Fixture(127, False, 2127, group="chunk_edges"),  # seed 127 misses the guard at max_iterations = 1 (4e-4)
    "m128_free": Fixture(128, False, 128, group="chunk_edges"),
    "m129_free": Fixture(129, False, 129, group="chunk_edges"),
    "m256_free": Fixture(256, False, 256, group="chunk_edges"),
    "m257_free": Fixture(257, False, 257, group="chunk_edges"),
    # bit 32 and bit 63 of the per-lane mask of nulled pairs
    "m4097_fixed": Fixture(4097, True, 7, group="full_mask", **LOW_NOISE),  # seed 7: pair 4096, alone in chunk 32, is nulled
    "m8192_free": Fixture(8192, False, 2, group="full_mask", **LOW_NOISE),
    # H = 0: every solve fails, ten trials, terminate
    "m40_zero_w": Fixture(40, False, 40, zero_weights=True, group="failed_solve"),
}
ORIGINAL = [k for k, f in FIXTURES.items() if f.group == "original"]
GROUPS = sorted({f.group for f in FIXTURES.values()} - {"original"})
PINHOLE_CAMERA_PAIRS = ["m70_cam_ab", "m70_cam_ba"]
BATCH = ["m0_free", "m9_free", "m12_free", "m70_free", "m150_free"]
# (fixture, max_iterations) of the heterogeneous batch: scale, camera model, th2 and the cap all differ
MIXED_BATCH = [("m0_fixed", 0), ("m70_cam_ab", 0), ("m70_cam_ba", 0), ("m70_kb8_ab", 0), ("m70_th599", 0),
               ("m9_fixed", 0), ("m70_fixed", 0), ("m129_free", 0), ("m70_free", 1), ("m150_fixed", 0),
               ("m0_free", 0)]


def camera(spec):
    return (O.kb8_camera if spec[0] == "kb8" else O.pinhole_camera)(*spec[1:])


def build(name, max_iterations=0):
    f = FIXTURES[name]
    P = O.synth_sim3_problem(np.random.default_rng(f.seed), f.n_pairs, f.outlier_frac, f.out_of_kf2_frac, f.fix_scale,
                             camera(f.cam1), camera(f.cam2), noise_px=f.noise_px, noise_m=f.noise_m, th2=f.th2)
    if f.zero_weights:
        P.inv_sigma2_1[:] = 0
        P.inv_sigma2_2[:] = 0
    P.max_iterations = max_iterations
    return P


def replicas(name, P):
    """The 16 nudged replicas of a fixture (their own seeded stream)."""
    from tests import pyref_sim3opt as R
    rng = np.random.default_rng(FIXTURES[name].seed + 77777)
    return [R.nudged(P, rng) for _ in range(N_REPLICAS)]
