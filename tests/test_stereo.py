"""Frame::ComputeStereoMatches (ref:src/Frame.cc:1117-1373): the C oracle pinned by the pure-Python
restatement and two hand cases (CPU); the GPU path bit-exact against the oracle (mvuRight / mvDepth bit
patterns and match counts) on EuRoC-shaped stereo pairs, batches, device-resident pyramids and edges."""
import numpy as np
import pytest

from orb_slam3_comments_ghr_amd import stereo as st
from tests import oracle_calls as oc
from tests import pyref_stereo as ps
from tests.stereo_boundary_fixtures import check_hand, hand_frame


def same(a, b):
    np.testing.assert_array_equal(np.asarray(a[0]).view(np.int32), np.asarray(b[0]).view(np.int32))
    np.testing.assert_array_equal(np.asarray(a[1]).view(np.int32), np.asarray(b[1]).view(np.int32))
    assert int(a[2]) == int(b[2])


@pytest.mark.parametrize("seed", range(3))
def test_oracle_vs_python(oracle, seed):
    F = st.synth_stereo_frame(np.random.default_rng(9900 + seed), n=300, bordered=seed == 2)
    ref = oc.stereo(oracle, F)
    ur, d, n, accepted = ps.compute_stereo_matches(F, stats=True)
    same(ref, (ur, d, n))
    assert n > 150 and accepted > n  # the median cut removed some
    assert (np.abs(ur[ur >= 0] - np.round(ur[ur >= 0])) > 1e-3).mean() > 0.5  # sub-pixel positions


def test_oracle_hand_cases(oracle):
    res = [oc.stereo(oracle, hand_frame(False)), oc.stereo(oracle, hand_frame(True))]
    check_hand(res)
    for noisy, r in zip((False, True), res):
        same(r, ps.compute_stereo_matches(hand_frame(noisy)))


def test_oracle_empty_and_edges(oracle):
    F = st.synth_stereo_frame(np.random.default_rng(9910), n=200, edge=0.0)
    same(oc.stereo(oracle, F), ps.compute_stereo_matches(F))  # patches leaving the image: no match
    E = st.StereoFrame(desc=F.desc[:0], x=[], y=[], octave=[], desc_r=F.desc_r, xr=F.xr, yr=F.yr,
                       octave_r=F.octave_r, left=F.left, right=F.right)
    assert oc.stereo(oracle, E)[2] == 0
    R0 = st.StereoFrame(desc=F.desc, x=F.x, y=F.y, octave=F.octave, desc_r=F.desc_r[:0], xr=[], yr=[], octave_r=[],
                        left=F.left, right=F.right)
    ur, d, n = oc.stereo(oracle, R0)
    assert n == 0 and (ur == -1).all() and (d == -1).all()


# ----------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_vs_oracle(ctx, oracle, seed):
    """EuRoC stereo shape: 752 x 480, 8 levels x 1.2, 1200 keypoints per side (nFeatures 1200)."""
    F = st.synth_stereo_frame(np.random.default_rng(9950 + seed), n=1200, bordered=bool(seed % 2))
    ref = oc.stereo(oracle, F)
    same(st.ComputeStereoMatches(ctx, F), ref)
    assert ref[2] > 500


@pytest.mark.gpu
def test_gpu_batch_and_device_pyramids(ctx, oracle):
    rng = np.random.default_rng(9970)
    frames = [st.synth_stereo_frame(rng, n=int(rng.integers(200, 1500)), bordered=bool(i % 3 == 0)) for i in range(10)]
    F = frames[0]
    frames.append(st.StereoFrame(desc=F.desc[:0], x=[], y=[], octave=[], desc_r=F.desc_r, xr=F.xr, yr=F.yr,
                                 octave_r=F.octave_r, left=F.left, right=F.right))
    frames.append(st.StereoFrame(desc=F.desc, x=F.x, y=F.y, octave=F.octave, desc_r=F.desc_r[:0], xr=[], yr=[],
                                 octave_r=[], left=F.left, right=F.right))
    refs = [oc.stereo(oracle, f) for f in frames]
    outs, nm = st.ComputeStereoMatchesBatch(ctx, frames)
    for (ur, d), k, r in zip(outs, nm, refs):
        same((ur, d, k), r)
    # the same frames with both pyramids resident in HBM (read in place, torch row strides)
    dev = [f.to_device() for f in frames[:6]]
    outs, nm = st.ComputeStereoMatchesBatch(ctx, dev)
    for (ur, d), k, r in zip(outs, nm, refs[:6]):
        same((ur, d, k), r)
    assert st.ComputeStereoMatchesBatch(ctx, [])[1].size == 0


@pytest.mark.gpu
def test_gpu_hand_cases_and_edges(ctx, oracle):
    check_hand([st.ComputeStereoMatches(ctx, hand_frame(False)), st.ComputeStereoMatches(ctx, hand_frame(True))])
    rng = np.random.default_rng(9980)
    F = st.synth_stereo_frame(rng, n=600, edge=0.0)  # patches leaving the level images
    same(st.ComputeStereoMatches(ctx, F), oc.stereo(oracle, F))
    # one dense row band: every left keypoint on row 200 sees all 700 right keypoints (> 64 per lane pass)
    F = st.synth_stereo_frame(rng, n=500, n_right=700)
    D = st.StereoFrame(desc=F.desc, x=F.x, y=np.full(F.n, 200.3, np.float32), octave=F.octave, desc_r=F.desc_r,
                       xr=F.xr, yr=np.full(F.n_right, 200.6, np.float32), octave_r=F.octave_r, left=F.left,
                       right=F.right)
    ref = oc.stereo(oracle, D)
    same(st.ComputeStereoMatches(ctx, D), ref)
    assert ref[2] > 50


@pytest.mark.gpu
def test_gpu_device_row_index(ctx, oracle):
    """vRowIndices built on the device (k_stereo_rows: LDS counts, block scan, atomic fill in any order):
    * a 1100-row image (more rows than the workgroup's 1024 threads: two rows per scan segment);
    * keypoints 2 px from the top and bottom, whose row bands the reference would index past (clipped);
    * 30 % exact duplicates on the same row: Hamming ties resolve to the lowest right index, as the
      reference's ascending candidate vector does."""
    rng = np.random.default_rng(9995)
    F = st.synth_stereo_frame(rng, n=900, width=800, height=1100, edge=2.0, dup=0.3)
    yr = np.array(F.yr, np.float32)
    yr[:20] = rng.uniform(0.0, 1.5, 20)
    yr[20:40] = 1099.0 - rng.uniform(0.0, 1.5, 20)
    F = st.StereoFrame(desc=F.desc, x=F.x, y=F.y, octave=F.octave, desc_r=F.desc_r, xr=F.xr, yr=yr,
                       octave_r=F.octave_r, left=F.left, right=F.right)
    ref = oc.stereo(oracle, F)
    same(st.ComputeStereoMatches(ctx, F), ref)
    assert ref[2] > 200
    outs, nm = st.ComputeStereoMatchesBatch(ctx, [F, F])
    for (ur, d), k in zip(outs, nm):
        same((ur, d, k), ref)


@pytest.mark.gpu
def test_gpu_batch_of_three_and_one_pyramid_on_the_device(ctx, oracle):
    """64 keypoints per side.  A batch whose middle frame has no left keypoint (nothing packed) equals the single
    calls and the oracle; then each side's pyramid alone on the device, the other packed from the host (strided
    levels of bordered buffers included): a device level's address must reach the kernel as given."""
    from dataclasses import replace
    rng = np.random.default_rng(9990)
    frames = [st.synth_stereo_frame(rng, n=64, bordered=bool(i == 2)) for i in range(3)]
    F = frames[1]
    frames[1] = st.StereoFrame(desc=F.desc[:0], x=[], y=[], octave=[], desc_r=F.desc_r, xr=F.xr, yr=F.yr,
                               octave_r=F.octave_r, left=F.left, right=F.right)
    refs = [oc.stereo(oracle, f) for f in frames]
    outs, nm = st.ComputeStereoMatchesBatch(ctx, frames)
    for f, (ur, d), k, r in zip(frames, outs, nm, refs):
        same((ur, d, k), r)
        same(st.ComputeStereoMatches(ctx, f), r)
    assert refs[0][2] > 0 and refs[1][2] == 0 and refs[2][2] > 0
    for f, r in ((frames[0], refs[0]), (frames[2], refs[2])):
        same(st.ComputeStereoMatches(ctx, replace(f, left=f.left.to_device())), r)
        same(st.ComputeStereoMatches(ctx, replace(f, right=f.right.to_device())), r)
