"""The lane arithmetic of k_top2_fp4q2's running top-2 with a second key that is never rebased
(csrc/top2_key.h), restated in numpy and compared with brute force.

Restated: the two lane halves of a query (accumulator element i of half h is row (i & 3) + 8 (i >> 2) + 4 h
of the 32-row tile), the order of the key pairs, the median / min3 update of key_push2f, the first key's
rebase by 32 after every tile, the pad key of rows past nt, the start sentinel and the final merge of the two
halves with its + 32 on the first key that becomes a second key.  Keys are written with MX_KEY0 removed.

The negative control drops the + 32: the restatement must then disagree with brute force at nt = 8192, where
a first key of rows 0-31 has been rebased 256 times (rho = row - 8192 < -8160)."""
import numpy as np
import pytest

SHIFT = 13
K2_OFFSET = 8160
PAD_KEY = 0x4E800000 - (0x4B000000 + (1 << 21))   # bits of 2^30 (MX_PAD swamps the row bias) - MX_KEY0
NTS = [1, 31, 32, 33, 257, 2000, 8160, 8161, 8191, 8192]


def _med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


def lanes_top2(H, pc, plus32=True):
    """H: (nq, nt) distances, pc: (nq,) |q|.  -> (idx, d1, d2) as the kernel writes them."""
    H = np.asarray(H, np.int64)
    nq, nt = H.shape
    pc = np.asarray(pc, np.int64)
    ntile = (nt + 31) // 32
    keys = np.full((nq, ntile * 32), PAD_KEY, np.int64)
    keys[:, :nt] = (H - pc[:, None]) << SHIFT
    keys = keys.reshape(nq, ntile, 32) + np.arange(32)
    k1 = np.repeat(((256 - pc) << SHIFT)[:, None], 2, axis=1)   # [query, lane half]
    k2 = k1.copy()
    elem_row = [(i & 3) + 8 * (i >> 2) for i in range(16)]
    pairs = [e for s in range(4) for e in ((2 * s, 2 * s + 1), (8 + 2 * s, 9 + 2 * s))]
    half = np.array([0, 4])
    for t in range(ntile):
        tk = keys[:, t]
        for ex, ey in pairs:
            x, y = tk[:, elem_row[ex] + half], tk[:, elem_row[ey] + half]
            m = _med3(k1, x, y)
            k1 = np.minimum(np.minimum(x, y), k1)
            k2 = np.minimum(m, k2)
        k1 = k1 - 32
    hi = k1.max(axis=1) + (32 if plus32 else 0)
    m2 = np.minimum(k2.min(axis=1), hi)
    m1 = k1.min(axis=1)
    t1 = m1 + 32 * ntile
    d1 = (t1 >> SHIFT) + pc
    d2 = ((m2 + K2_OFFSET) >> SHIFT) + pc
    idx = np.where(d1 < 256, t1 & ((1 << SHIFT) - 1), -1)
    return idx, np.minimum(d1, 256), np.minimum(d2, 256)


def brute_top2(H):
    H = np.asarray(H, np.int64)
    d1 = H.min(axis=1)
    idx = np.where(d1 < 256, H.argmin(axis=1), -1)
    if H.shape[1] > 1:
        d2 = np.partition(H, 1, axis=1)[:, 1]
    else:
        d2 = np.full(H.shape[0], 256, np.int64)
    return idx, np.minimum(d1, 256), np.minimum(d2, 256)


def cases(nt):
    """name -> (H, pc); |q| of 0 and of 256 in every case (D = H - |q| spans [-256, 256])."""
    rng = np.random.default_rng(1000 + nt)
    out = {}
    pcs = np.array([0, 256, 0, 256, 97, 128, 1, 255])
    out["ties"] = (rng.integers(100, 103, (8, nt)), pcs)
    out["ties_low"] = (rng.integers(0, 2, (8, nt)), pcs)
    out["random"] = (rng.integers(0, 257, (8, nt)), pcs)
    for d in (0, 100, 254):
        a = np.full((8, nt), 256)
        a[:, 0] = d + 1
        if nt > 1:
            a[:, -1] = d
        a[4:, 1:-1] = 255   # half the queries with the others far but real
        out[f"first_d1_last_d_{d}"] = (a, pcs)
        b = np.full((8, nt), 256)
        b[:, 0] = d
        if nt > 1:
            b[:, -1] = d + 1
        b[4:, 1:-1] = 255
        out[f"first_d_last_d1_{d}"] = (b, pcs)
    for pos in sorted({0, nt // 2, nt - 1}):
        a = np.full((8, nt), 256)
        a[:, pos] = 255
        out[f"one_255_at_{pos}"] = (a, pcs)
    out["all_256"] = (np.full((8, nt), 256), pcs)
    return out


@pytest.mark.parametrize("nt", NTS)
def test_unrebased_second_key_equals_brute_force(nt):
    for name, (H, pc) in cases(nt).items():
        got, ref = lanes_top2(H, pc), brute_top2(H)
        for k, col in enumerate(("idx", "d1", "d2")):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"nt {nt} case {name} column {col}")


def test_negative_control_without_the_plus_32():
    """Row 0 at d + 1 and the last row at d are the first keys of the two lane halves; row 0's has been rebased
    256 times when it becomes the second key."""
    H, pc = cases(8192)["first_d1_last_d_100"]
    ref = brute_top2(H)
    assert (ref[2] == 101).all()
    good, bad = lanes_top2(H, pc), lanes_top2(H, pc, plus32=False)
    np.testing.assert_array_equal(good[2], ref[2])
    assert (bad[2] == 100).all()
    # and it is only the second distance that the + 32 touches
    np.testing.assert_array_equal(bad[0], ref[0])
    np.testing.assert_array_equal(bad[1], ref[1])


@pytest.mark.parametrize("nt", [8161, 8191, 8192])
def test_negative_control_fails_from_8161_rows(nt):
    """Row 0 at d + 1 and row 4 (the other lane half) at d: 256 tiles from 8161 rows on, 255 at 8160."""
    pc = cases(nt)["all_256"][1]
    H = np.full((8, nt), 256)
    H[:, 0], H[:, 4] = 101, 100
    np.testing.assert_array_equal(lanes_top2(H[:, :8160], pc, plus32=False)[2], brute_top2(H[:, :8160])[2])
    assert not np.array_equal(lanes_top2(H, pc, plus32=False)[2], brute_top2(H)[2])
    np.testing.assert_array_equal(lanes_top2(H, pc)[2], brute_top2(H)[2])


def test_key_header_clean_under_host_sanitizers(tmp_path):
    """tests/host/top2_key.cpp: the header's constants and decode functions, exhaustively, under ASan + UBSan."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "top2_key")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "orb_slam3_comments_ghr_amd", "csrc"),
                        os.path.join(root, "tests", "host", "top2_key.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])
