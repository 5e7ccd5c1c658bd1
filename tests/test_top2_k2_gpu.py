"""GPU parity of k_top2_fp4q2 with its never-rebased second key (csrc/top2_key.h) where the key's row field
is nearly or wholly used: nt in {8129, 8160, 8161, 8191, 8192} (255 tiles, and 256 tiles from 8161 rows on,
where a first key of rows 0-31 that ends as the second distance has been rebased past the second key's
range and takes 32 back in the final merge).  In-process on the default kernel, bit-exact against the oracle's
serial loop; 65 queries (a wave with both tiles, one with a single query) and three frames per launch."""
import numpy as np
import pytest

from tests.test_top2_gpu import _batch, otop2

pytestmark = pytest.mark.gpu

NQ = 65
NTS = [8129, 8160, 8161, 8191, 8192]


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _queries(base, rng):
    """NQ queries: base with 0-3 bits flipped among bits 128-255 (query 0 is base itself); the train rows of
    the structured frames differ from base only in bits 0-127, so every query keeps the frame's order."""
    return np.stack([_flip(base, rng.choice(np.arange(128, 256), i % 4, replace=False)) for i in range(NQ)])


def _two_rows(nt, base, near, second, d, rng):
    """Row `near` at d and row `second` at d + 1 from base, every other row base's complement."""
    t = np.repeat(~base[None], nt, axis=0)
    bits = rng.choice(128, d + 1, replace=False)
    t[near], t[second] = _flip(base, bits[:d]), _flip(base, bits)
    return _queries(base, rng), t


def _one_255(nt, rng):
    """Every row at 256 from the base query but one at 255."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    t = np.repeat(~base[None], nt, axis=0)
    t[int(rng.integers(0, nt))] = _flip(~base, [int(rng.integers(0, 128))])
    return _queries(base, rng), t


def _near_copies(nt, rng):
    """Random frame with an all-zero and an all-one query; every query has two near-copies (0-3 flipped bits
    each) in the first and the last tile or on the two sides of the chunk edge at row 4096, in either order."""
    q = rng.integers(0, 256, (NQ, 32), dtype=np.uint8)
    q[0], q[1] = 0, 255
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for i in range(NQ):
        s = i // 4
        ra, rb = [(s, nt - 1 - s), (17 + s, nt - 18 - s), (4095 - s, 4096 + s), (4078 - s, 4113 + s)][i % 4]
        if rng.integers(0, 2):
            ra, rb = rb, ra
        t[ra] = _flip(q[i], rng.choice(256, int(rng.integers(0, 4)), replace=False))
        t[rb] = _flip(q[i], rng.choice(256, int(rng.integers(0, 4)), replace=False))
    return q, t


def _launches(nt):
    rng = np.random.default_rng(8200 + nt)
    zero, ones = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    rnd = rng.integers(0, 256, 32, dtype=np.uint8)
    return {
        # row 0 at d + 1 and the last row at d (all-zero base: query 0 is the all-zero query), its mirror
        # (all-one base), and one row at 255
        "edges": [_two_rows(nt, zero, nt - 1, 0, 100, rng), _two_rows(nt, ones, 0, nt - 1, 3, rng), _one_255(nt, rng)],
        # near-copies, and row 0 at d + 1 with row 4 (the other lane half of the first tile) at d
        "copies": [_near_copies(nt, rng), _near_copies(nt, rng), _two_rows(nt, rnd, 4, 0, 0, rng)],
    }


@pytest.mark.parametrize("nt", NTS)
def test_unrebased_second_key_equals_serial_loop(ctx, oracle, nt):
    for name, frames in _launches(nt).items():
        qs, ts = zip(*frames)
        assert ctx.hamming_top2_batch_plan(NQ, nt, len(frames)) == f"k_top2_fp4q2<16,256> grid={len(frames)} x 1024"
        got = _batch(ctx, qs, ts)
        assert got.shape == (len(frames), NQ, 3)
        for b, (q, t) in enumerate(frames):
            for k, ref in enumerate(otop2(oracle, q, t)):
                np.testing.assert_array_equal(got[b, :, k], ref, err_msg=f"nt {nt} launch {name} frame {b} column {k}")


def test_the_edge_frames_hold_what_they_claim(oracle):
    """Frame 0 of "edges" at 8192 rows: best row nt - 1 at 100 + f and second distance 101 + f from row 0, f the
    query's own 0-3 flipped bits: the case that needs the + 32."""
    q, t = _launches(8192)["edges"][0]
    bi, bd, sd = otop2(oracle, q, t)
    f = np.arange(NQ) % 4
    np.testing.assert_array_equal(bi, 8191)
    np.testing.assert_array_equal(bd, 100 + f)
    np.testing.assert_array_equal(sd, 101 + f)
