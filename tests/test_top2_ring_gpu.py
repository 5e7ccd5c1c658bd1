"""GPU parity of k_top2_fp4q2 with its three-slot chunk ring (csrc/top2_ring.h) and its pipeline that does not stop
at a chunk's end: 1-10 chunks of 256 rows (the first and the second wrap of the ring), with a remainder that is
none, a partial tile only, full tiles only, or both.  In-process on the default kernel, bit-exact against the
oracle's serial loop on all queries and all three columns; three frames per launch; 65 queries (a wave with both
query tiles and a wave with one query) at every nt, 1057 (two workgroups per frame) at two.

The frames are random rows with each query's two nearest rows planted: copies of query i with i % 3 and
i % 3 + 1 flipped bits, the nearer in chunk i mod nch and the other in chunk (i + 1) mod nch; for about a quarter
of the queries (every fourth run of nch queries) on the two sides of a chunk seam instead (rows 256 k - 1 and
256 k, the nearer on either side in turn).  So every chunk holds some query's best row, and a slot read stale or
too early changes an output.  The second-nearest copies are written first, so that where rows are few the
nearest ones are what stays."""
import numpy as np
import pytest

from tests.test_top2_gpu import otop2

CR = 256
NB = 3
NTS = [1, 32, 33, 255, 256, 257, 288, 511, 512, 513, 768, 769, 800, 1024, 1025, 1296, 2000, 2305]
CASES = [(65, nt) for nt in NTS] + [(1057, 769), (1057, 2000)]


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _frame(nq, nt, rng):
    nch = (nt + CR - 1) // CR
    nseam = (nt - 1) // CR                     # seams at rows 256 k, k = 1..nseam
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    near, other = [], []
    for i in range(nq):
        if nseam and (i // nch) % 4 == 3:
            k = 1 + i % nseam
            ra, rb = (CR * k - 1, CR * k) if (i // nch) % 8 == 3 else (CR * k, CR * k - 1)
        else:
            ca, cb = i % nch, (i + 1) % nch
            ra = CR * ca + int(rng.integers(0, min(CR, nt - CR * ca)))
            rb = CR * cb + int(rng.integers(0, min(CR, nt - CR * cb)))
        fa = i % 3
        bits = rng.choice(256, fa + 1, replace=False)
        near.append((ra, _flip(q[i], bits[:fa])))
        other.append((rb, _flip(q[i], bits)))
    for r, d in other + near:
        t[r] = d
    return q, t


def _launch(ctx, qs, ts):
    """The frames in one launch -> (nb, nq, 3).  The context launches on a stream of its own that does not wait for
    torch's, so the uploads and the fill of the output are finished before the launch."""
    import torch
    nb, nq, nt = len(qs), qs[0].shape[0], ts[0].shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(np.concatenate(qs))).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(np.concatenate(ts))).cuda()
    do = torch.full((nb * nq, 3), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.hamming_top2_batch_dev(dq, nq, dt, nt, nb, do)
    torch.cuda.synchronize()
    return do.cpu().numpy().reshape(nb, nq, 3)


_cache = {}


def _case(oracle, nq, nt):
    """-> (frames, oracle results), computed once per shape and shared by the tests."""
    if (nq, nt) not in _cache:
        rng = np.random.default_rng(31000 + 7 * nq + nt)
        frames = [_frame(nq, nt, rng) for _ in range(NB)]
        refs = [otop2(oracle, q, t) for q, t in frames]
        for q, t in frames:
            q.setflags(write=False)
            t.setflags(write=False)
        _cache[(nq, nt)] = (frames, refs)
    return _cache[(nq, nt)]


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nt", CASES)
def test_ring_equals_serial_loop(ctx, oracle, nq, nt):
    frames, refs = _case(oracle, nq, nt)
    qs, ts = zip(*frames)
    assert ctx.hamming_top2_batch_plan(nq, nt, NB) == f"k_top2_fp4q2<16,256> grid={NB * ((nq + 1023) // 1024)} x 1024"
    got = _launch(ctx, qs, ts)
    assert got.shape == (NB, nq, 3)
    for b in range(NB):
        for k, ref in enumerate(refs[b]):
            np.testing.assert_array_equal(got[b, :, k], ref, err_msg=f"nq {nq} nt {nt} frame {b} column {k}")


def test_every_chunk_holds_some_best_row(oracle):
    """From the oracle alone: in every frame of every case each chunk of 256 rows holds the best row of some query,
    and, where there is a seam, some query's two nearest rows lie on its two sides."""
    for nq, nt in CASES:
        frames, refs = _case(oracle, nq, nt)
        nch = (nt + CR - 1) // CR
        for b, (bi, bd, sd) in enumerate(refs):
            assert (bi >= 0).all() and (sd >= bd).all() and (bd <= 2).sum() >= nch, (nq, nt, b)
            assert set(np.unique(bi // CR)) == set(range(nch)), (nq, nt, b, sorted(set(bi // CR)))
            if nt > CR:
                assert ((bi % CR == CR - 1) | (bi % CR == 0)).sum() > 0, (nq, nt, b)
