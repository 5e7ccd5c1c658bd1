"""GPU parity of k_top2_fp4q2 at the ends of its chunk ring: the last chunk that exists in each ring slot, exact and
cut, with the two blocks behind it that have no chunk left to expand; and frames with no full chunk at all, where
every block is the tail.  The packed rows come through a buffer descriptor that ends at row nt, the staging and
fragment offsets are held through the blocks, and the last two blocks of a workgroup only pass the barrier: a wrong
offset in the last real chunk, a row past nt that is not zero, or a slot left over from an earlier chunk that is
taken for real changes an output here.

In-process on the default kernel, bit-exact against the oracle's serial loop on all queries and all three columns;
three frames per launch; 65 queries (a wave with both query tiles and a wave with one) at every nt, 1057 (two
workgroups per frame, most of their waves only staging) at two.  nt = 255 .. 1040 is 1 .. 5 chunks of 256 rows, so
the last chunk lies in slots 0, 1, 2, 0, 1.

The frames are random rows with each query's two nearest rows planted as in tests/test_top2_ring_gpu.py (copies
of query i with i % 3 and i % 3 + 1 flipped bits, in chunks i mod nch and (i + 1) mod nch).  Of every eight
queries one has its nearest row at nt - 1 and one at the first row of the last chunk; those rows are written last.
The last two queries of every frame are all zeros and all ones and have nothing planted: a row past nt is zero
nibbles, at distance |q| from a query, so at distance 0 from the all-zero query, whose best distance in the frame
is above 0 because no train row is all zero."""
import numpy as np
import pytest

from tests.test_top2_gpu import otop2

CR = 256
NB = 3
NTS = [1, 16, 33, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1040]
CASES = [(65, nt) for nt in NTS] + [(1057, 257), (1057, 769)]


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _frame(nq, nt, rng):
    nch = (nt + CR - 1) // CR
    last0 = CR * (nch - 1)                     # the first row of the last chunk
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q[nq - 2] = 0
    q[nq - 1] = 0xFF
    near, other, ends = [], [], []
    for i in range(nq - 2):
        ca, cb = i % nch, (i + 1) % nch
        ra = CR * ca + int(rng.integers(0, min(CR, nt - CR * ca)))
        rb = CR * cb + int(rng.integers(0, min(CR, nt - CR * cb)))
        fa = i % 3
        bits = rng.choice(256, fa + 1, replace=False)
        other.append((rb, _flip(q[i], bits)))
        if i % 8 == 5:
            ends.append((nt - 1, _flip(q[i], bits[:fa])))
        elif i % 8 == 6:
            ends.append((last0, _flip(q[i], bits[:fa])))
        else:
            near.append((ra, _flip(q[i], bits[:fa])))
    for r, d in other + near + ends:
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
        rng = np.random.default_rng(47000 + 7 * nq + nt)
        frames = [_frame(nq, nt, rng) for _ in range(NB)]
        refs = [otop2(oracle, q, t) for q, t in frames]
        for q, t in frames:
            q.setflags(write=False)
            t.setflags(write=False)
        _cache[(nq, nt)] = (frames, refs)
    return _cache[(nq, nt)]


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nt", CASES)
def test_ring_ends_equal_serial_loop(ctx, oracle, nq, nt):
    frames, refs = _case(oracle, nq, nt)
    qs, ts = zip(*frames)
    assert ctx.hamming_top2_batch_plan(nq, nt, NB) == f"k_top2_fp4q2<16,256> grid={NB * ((nq + 1023) // 1024)} x 1024"
    got = _launch(ctx, qs, ts)
    assert got.shape == (NB, nq, 3)
    for b in range(NB):
        for k, ref in enumerate(refs[b]):
            np.testing.assert_array_equal(got[b, :, k], ref, err_msg=f"nq {nq} nt {nt} frame {b} column {k}")


def test_fixtures_reach_the_last_chunk_and_the_pad_rows(oracle):
    """From the oracle alone: in every frame of every case some query's best row is nt - 1, some query's best row
    is the first row of the last chunk, no train row is all zero, and the all-zero query's best distance is
    above 0 (and the all-ones query is there)."""
    for nq, nt in CASES:
        frames, refs = _case(oracle, nq, nt)
        last0 = CR * ((nt + CR - 1) // CR - 1)
        for b, ((q, t), (bi, bd, sd)) in enumerate(zip(frames, refs)):
            assert not q[nq - 2].any() and (q[nq - 1] == 0xFF).all(), (nq, nt, b)
            assert t.any(axis=1).all(), (nq, nt, b)
            assert (bi[:nq - 2] == nt - 1).any(), (nq, nt, b)
            assert (bi[:nq - 2] == last0).any(), (nq, nt, b)
            assert bd[nq - 2] > 0 and bi[nq - 2] >= 0, (nq, nt, b, int(bd[nq - 2]))
            assert (bd[(bi == nt - 1) | (bi == last0)] <= 2).any(), (nq, nt, b)
