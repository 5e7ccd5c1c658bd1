// tracking_driver.cpp — Tracking::SearchLocalPoints through the ORB-SLAM3-side adapter on mock objects (test-only;
// tests/test_adapter_frustum.py).  Builds the same world twice from an array file (the current Frame "F.*" with its
// slot occupants "S.*", the local MapPoints "P.*", the frame's frustum constants) and runs
//   A: TrackingMock::SearchLocalPoints, the body of adapters/orbslam3/Tracking_osg.cc (one fused call);
//   B: a literal copy of the reference's loop (ref:src/Tracking.cc:4097-4182 with Frame::isInFrustum[Checks],
//      ref:src/Frame.cc:676-782, 1608-1705, and MapPoint::PredictScale, ref:src/MapPoint.cc:722-738) in host
//      float arithmetic, followed by the adapter's existing SearchByProjection(Frame&, vector<MapPoint*>&),
// then dumps every field the step touches of both worlds.  Built with -ffp-contract=off.
// With a third argument <reps> it times instead (tools/frustum_bench.py): the literal isInFrustum loop alone, the
// SearchByProjection adapter call that follows it, and the adapter's fused SearchLocalPoints, each over the same
// world with the slots put back before every repetition; medians in microseconds.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "driver_common.h"
#include "mock_tracking.h"

namespace {

struct World {
    TrackingMock tr;
    std::vector<std::unique_ptr<TrMapPoint>> pool;
    std::vector<TrMapPoint *> occupants;
};

void build_world(const Arrays &in, World &w)
{
    TrFrame &F = w.tr.mCurrentFrame;
    build_frame(in, F, "F.");
    const int32_t *pr = get(in, "params").p<int32_t>();  // th, bFarPoints, frame id
    w.tr.th = pr[0], w.tr.mbFarPoints = pr[1] != 0, F.mnId = (unsigned long)pr[2];
    w.tr.mThFarPoints = get(in, "th_far").p<float>()[0];
    const Arr &fr = get(in, "frustum");
    if (fr.b.size() != sizeof(osg_frustum_frame)) {
        std::fprintf(stderr, "osg_frustum_frame size %zu, expected %zu\n", fr.b.size(), sizeof(osg_frustum_frame));
        std::exit(2);
    }
    std::memcpy(&F.frustum, fr.b.data(), sizeof(osg_frustum_frame));
    F.mfLogScaleFactor = F.frustum.log_scale_factor;
    // slot occupants: id, Observations(), isBad()
    F.mvpMapPoints.assign(F.N, nullptr);
    const int32_t *sm = get(in, "S.slot_mp").p<int32_t>();
    const uint8_t *st = get(in, "S.slot_taken").p<uint8_t>(), *sb = get(in, "S.slot_bad").p<uint8_t>();
    for (int i = 0; i < F.N; i++)
        if (sm[i] >= 0) {
            w.pool.emplace_back(new TrMapPoint());
            TrMapPoint *p = w.pool.back().get();
            p->mnId = (unsigned long)sm[i], p->nobs = st[i], p->bad = sb[i] != 0;
            p->mbTrackInView = p->mbTrackInViewR = true;  // stale: step 1 clears them
            F.mvpMapPoints[i] = p;
            w.occupants.push_back(p);
        }
    // local MapPoints with stale track fields, as tests/pyref_frustum.py's MapPoints start
    const int n = (int)get(in, "P.mp_id").n;
    const float *pos = get(in, "P.pos").p<float>(), *nrm = get(in, "P.normal").p<float>();
    for (int i = 0; i < n; i++) {
        w.pool.emplace_back(new TrMapPoint());
        TrMapPoint *p = w.pool.back().get();
        p->mnId = (unsigned long)get(in, "P.mp_id").p<int32_t>()[i];
        std::memcpy(p->desc.buf.data(), get(in, "P.desc").p<uint8_t>() + 32 * i, 32);
        p->bad = get(in, "P.bad").p<uint8_t>()[i] != 0;
        p->mnLastFrameSeen = get(in, "P.seen").p<uint8_t>()[i] ? F.mnId : F.mnId - 1;
        p->nobs = get(in, "P.has_obs").p<uint8_t>()[i];
        for (int k = 0; k < 3; k++) p->world[k] = pos[3 * i + k], p->normal[k] = nrm[3 * i + k];
        p->mfMaxDistance = get(in, "P.max_dist").p<float>()[i];
        p->mfMinDistance = get(in, "P.min_dist").p<float>()[i];
        // a MapPoint this frame already holds had its flags cleared by step 1; a bad one is given clear flags too
        // (SearchByProjection skips it either way, but the matcher's ABI checks the stale level of a flagged point)
        const bool candidate = !p->bad && p->mnLastFrameSeen != F.mnId;
        p->mbTrackInView = candidate && i % 2 == 0, p->mbTrackInViewR = candidate && i % 3 == 0;
        p->mTrackProjX = 1000.f + i, p->mTrackProjY = 2000.f + i, p->mTrackProjXR = 3000.f + i, p->mTrackProjYR = 4000.f + i;
        p->mnTrackScaleLevel = i % 5 + 20, p->mnTrackScaleLevelR = i % 7 + 30;
        p->mTrackViewCos = 0.25f + i % 4, p->mTrackViewCosR = 0.75f + i % 4;
        p->mTrackDepth = get(in, "P.prev_depth").p<float>()[i], p->mTrackDepthR = 6000.f + i;
        w.tr.mvpLocalMapPoints.push_back(p);
    }
}

// ---- the reference, literally ------------------------------------------------------------------------------

void project(const osg_frustum_camera &c, const float Pc[3], float uv[2])
{
    if (c.cam_type == 0) {  // ref:src/CameraModels/Pinhole.cpp:64-71
        uv[0] = c.cam[0] * Pc[0] / Pc[2] + c.cam[2];
        uv[1] = c.cam[1] * Pc[1] / Pc[2] + c.cam[3];
        return;
    }
    // ref:src/CameraModels/KannalaBrandt8.cpp:87-104
    const float x2_plus_y2 = Pc[0] * Pc[0] + Pc[1] * Pc[1];
    const float theta = std::atan2(std::sqrt(x2_plus_y2), Pc[2]);
    const float psi = std::atan2(Pc[1], Pc[0]);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = theta + c.cam[4] * theta3 + c.cam[5] * theta5 + c.cam[6] * theta7 + c.cam[7] * theta9;
    uv[0] = c.cam[0] * r * std::cos(psi) + c.cam[2];
    uv[1] = c.cam[1] * r * std::sin(psi) + c.cam[3];
}

float norm3(const float a[3]) { return std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

int predict_scale(const TrMapPoint *pMP, float currentDist, const TrFrame *pF)
{
    const float ratio = pMP->mfMaxDistance / currentDist;
    int nScale = (int)std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
    if (nScale < 0)
        nScale = 0;
    else if (nScale >= pF->mnScaleLevels)
        nScale = pF->mnScaleLevels - 1;
    return nScale;
}

void to_camera(const osg_frustum_camera &c, const float P[3], float Pc[3])
{
    for (int r = 0; r < 3; r++) Pc[r] = ((c.R[3 * r] * P[0] + c.R[3 * r + 1] * P[1]) + c.R[3 * r + 2] * P[2]) + c.t[r];
}

bool isInFrustumChecks(TrFrame &F, TrMapPoint *pMP, float viewingCosLimit, bool bRight)
{
    const osg_frustum_camera &c = F.frustum.cam[bRight ? 1 : 0];
    const float *P = pMP->world;
    float Pc[3];
    to_camera(c, P, Pc);
    const float Pc_dist = norm3(Pc);
    const float PcZ = Pc[2];
    if (PcZ < 0.0f) return false;
    float uv[2];
    project(c, Pc, uv);
    if (uv[0] < F.mnMinX || uv[0] > F.mnMaxX) return false;
    if (uv[1] < F.mnMinY || uv[1] > F.mnMaxY) return false;
    const float maxDistance = 1.2f * pMP->mfMaxDistance;
    const float minDistance = 0.8f * pMP->mfMinDistance;
    const float PO[3] = {P[0] - c.c[0], P[1] - c.c[1], P[2] - c.c[2]};
    const float dist = norm3(PO);
    if (dist < minDistance || dist > maxDistance) return false;
    const float *Pn = pMP->normal;
    const float viewCos = ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) / dist;
    if (viewCos < viewingCosLimit) return false;
    const int nPredictedLevel = predict_scale(pMP, dist, &F);
    if (bRight) {
        pMP->mTrackProjXR = uv[0];
        pMP->mTrackProjYR = uv[1];
        pMP->mnTrackScaleLevelR = nPredictedLevel;
        pMP->mTrackViewCosR = viewCos;
        pMP->mTrackDepthR = Pc_dist;
    } else {
        pMP->mTrackProjX = uv[0];
        pMP->mTrackProjY = uv[1];
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        pMP->mTrackDepth = Pc_dist;
    }
    return true;
}

bool isInFrustum(TrFrame &F, TrMapPoint *pMP, float viewingCosLimit)
{
    if (F.Nleft == -1) {
        const osg_frustum_camera &c = F.frustum.cam[0];
        pMP->mbTrackInView = false;
        pMP->mTrackProjX = -1;
        pMP->mTrackProjY = -1;
        const float *P = pMP->world;
        float Pc[3];
        to_camera(c, P, Pc);
        const float Pc_dist = norm3(Pc);
        const float PcZ = Pc[2];
        const float invz = 1.0f / PcZ;
        if (PcZ < 0.0f) return false;
        float uv[2];
        project(c, Pc, uv);
        if (uv[0] < F.mnMinX || uv[0] > F.mnMaxX) return false;
        if (uv[1] < F.mnMinY || uv[1] > F.mnMaxY) return false;
        pMP->mTrackProjX = uv[0];
        pMP->mTrackProjY = uv[1];
        const float maxDistance = 1.2f * pMP->mfMaxDistance;
        const float minDistance = 0.8f * pMP->mfMinDistance;
        const float PO[3] = {P[0] - c.c[0], P[1] - c.c[1], P[2] - c.c[2]};
        const float dist = norm3(PO);
        if (dist < minDistance || dist > maxDistance) return false;
        const float *Pn = pMP->normal;
        const float viewCos = ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) / dist;
        if (viewCos < viewingCosLimit) return false;
        const int nPredictedLevel = predict_scale(pMP, dist, &F);
        pMP->mbTrackInView = true;
        pMP->mTrackProjX = uv[0];
        pMP->mTrackProjXR = uv[0] - F.mbf * invz;
        pMP->mTrackDepth = Pc_dist;
        pMP->mTrackProjY = uv[1];
        pMP->mnTrackScaleLevel = nPredictedLevel;
        pMP->mTrackViewCos = viewCos;
        return true;
    }
    pMP->mbTrackInView = false;
    pMP->mbTrackInViewR = false;
    pMP->mnTrackScaleLevel = -1;
    pMP->mnTrackScaleLevelR = -1;
    pMP->mbTrackInView = isInFrustumChecks(F, pMP, viewingCosLimit, false);
    pMP->mbTrackInViewR = isInFrustumChecks(F, pMP, viewingCosLimit, true);
    return pMP->mbTrackInView || pMP->mbTrackInViewR;
}

int reference_search_local_points(TrackingMock &t)
{
    TrFrame &mCurrentFrame = t.mCurrentFrame;
    for (auto vit = mCurrentFrame.mvpMapPoints.begin(), vend = mCurrentFrame.mvpMapPoints.end(); vit != vend; vit++) {
        TrMapPoint *pMP = *vit;
        if (pMP) {
            if (pMP->isBad()) {
                *vit = static_cast<TrMapPoint *>(NULL);
            } else {
                pMP->IncreaseVisible();
                pMP->mnLastFrameSeen = mCurrentFrame.mnId;
                pMP->mbTrackInView = false;
                pMP->mbTrackInViewR = false;
            }
        }
    }
    int nToMatch = 0;
    for (auto vit = t.mvpLocalMapPoints.begin(), vend = t.mvpLocalMapPoints.end(); vit != vend; vit++) {
        TrMapPoint *pMP = *vit;
        if (pMP->mnLastFrameSeen == mCurrentFrame.mnId) continue;
        if (pMP->isBad()) continue;
        if (isInFrustum(mCurrentFrame, pMP, 0.5)) {
            pMP->IncreaseVisible();
            nToMatch++;
        }
        if (pMP->mbTrackInView) {
            cv::Point2f pt;
            pt.x = pMP->mTrackProjX, pt.y = pMP->mTrackProjY;
            mCurrentFrame.mmProjectPoints[pMP->mnId] = pt;
        }
    }
    int matches = 0;
    if (nToMatch > 0)  // ORBmatcher matcher(0.8); matcher.SearchByProjection(...)
        matches = osg_orbslam3::search_by_projection_mps<TrHooks>(mCurrentFrame, t.mvpLocalMapPoints, (float)t.th,
                                                                  t.mbFarPoints, t.mThFarPoints, 0.8f);
    return matches;
}

void dump(Arrays &out, const std::string &pre, const World &w, int rc)
{
    const std::vector<TrMapPoint *> &v = w.tr.mvpLocalMapPoints;
    std::vector<uint8_t> in_view, in_view_r;
    std::vector<float> f[8];
    std::vector<int32_t> level, level_r, visible, seen, proj_ids, slots, occ;
    for (const TrMapPoint *p : v) {
        in_view.push_back(p->mbTrackInView), in_view_r.push_back(p->mbTrackInViewR);
        const float vals[8] = {p->mTrackProjX, p->mTrackProjY, p->mTrackProjXR, p->mTrackProjYR,
                               p->mTrackViewCos, p->mTrackViewCosR, p->mTrackDepth, p->mTrackDepthR};
        for (int k = 0; k < 8; k++) f[k].push_back(vals[k]);
        level.push_back(p->mnTrackScaleLevel), level_r.push_back(p->mnTrackScaleLevelR);
        visible.push_back(p->mnVisible), seen.push_back(p->mnLastFrameSeen == w.tr.mCurrentFrame.mnId);
    }
    const char *names[8] = {"proj_x", "proj_y", "proj_xr", "proj_yr", "view_cos", "view_cos_r", "depth", "depth_r"};
    for (int k = 0; k < 8; k++) out[pre + names[k]] = make('f', f[k]);
    out[pre + "in_view"] = make('b', in_view), out[pre + "in_view_r"] = make('b', in_view_r);
    out[pre + "level"] = make('i', level), out[pre + "level_r"] = make('i', level_r);
    out[pre + "visible"] = make('i', visible), out[pre + "seen"] = make('i', seen);
    std::vector<float> proj_xy;
    for (const auto &kv : w.tr.mCurrentFrame.mmProjectPoints) {
        proj_ids.push_back((int32_t)kv.first);
        proj_xy.push_back(kv.second.x), proj_xy.push_back(kv.second.y);
    }
    out[pre + "proj_ids"] = make('i', proj_ids), out[pre + "proj_xy"] = make('f', proj_xy);
    for (const TrMapPoint *p : w.tr.mCurrentFrame.mvpMapPoints) slots.push_back(p ? (int32_t)p->mnId : -1);
    out[pre + "slots"] = make('i', slots);
    for (const TrMapPoint *p : w.occupants) {  // step 1 on the slot occupants
        occ.push_back(p->mnVisible), occ.push_back(p->mnLastFrameSeen == w.tr.mCurrentFrame.mnId);
        occ.push_back(p->mbTrackInView), occ.push_back(p->mbTrackInViewR);
    }
    out[pre + "occupants"] = make('i', occ);
    out[pre + "rc"] = make('i', std::vector<int32_t>{rc});
}

double median_us(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2] * 1e6;
}

template <class F>
double seconds(F &&f)
{
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int bench(World &a, World &b, int reps, const char *path)
{
    const std::vector<TrMapPoint *> slots_a = a.tr.mCurrentFrame.mvpMapPoints, slots_b = b.tr.mCurrentFrame.mvpMapPoints;
    std::vector<double> t_loop, t_mps, t_fused;
    int sink = 0;
    for (int r = 0; r < reps + 3; r++) {  // three warm-up repetitions
        // the state a new frame meets: the slots as built (a matched local MapPoint sits in a slot afterwards, and
        // step 1 would mark it as seen in the next repetition)
        a.tr.mCurrentFrame.mvpMapPoints = slots_a, b.tr.mCurrentFrame.mvpMapPoints = slots_b;
        TrFrame &F = b.tr.mCurrentFrame;
        const double tl = seconds([&] {
            for (TrMapPoint *pMP : b.tr.mvpLocalMapPoints) {
                if (pMP->mnLastFrameSeen == F.mnId) continue;
                if (pMP->isBad()) continue;
                if (isInFrustum(F, pMP, 0.5)) sink++;
            }
        });
        const double tm = seconds([&] {
            sink += osg_orbslam3::search_by_projection_mps<TrHooks>(F, b.tr.mvpLocalMapPoints, (float)b.tr.th, b.tr.mbFarPoints,
                                                                    b.tr.mThFarPoints, 0.8f);
        });
        const double tf = seconds([&] { sink += a.tr.SearchLocalPoints(); });
        if (r >= 3) t_loop.push_back(tl), t_mps.push_back(tm), t_fused.push_back(tf);
    }
    Arrays out;
    out["bench_us"] = make('f', std::vector<float>{(float)median_us(t_loop), (float)median_us(t_mps), (float)median_us(t_fused)});
    out["sink"] = make('i', std::vector<int32_t>{sink});
    write_arrays(path, out);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: tracking_driver <in> <out> [reps]\n");
        return 2;
    }
    const Arrays in = read_arrays(argv[1]);
    World a, b;
    build_world(in, a);
    build_world(in, b);
    if (argc == 4) {
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        return bench(a, b, std::atoi(argv[3]), argv[2]);
    }
    const int rc_a = a.tr.SearchLocalPoints();
    if (osg_orbslam3::thread_ctx() == nullptr) {
        std::fprintf(stderr, "no device context\n");
        return 3;
    }
    const int rc_b = reference_search_local_points(b.tr);
    Arrays out;
    dump(out, "A.", a, rc_a);
    dump(out, "B.", b, rc_b);
    write_arrays(argv[2], out);
    return 0;
}
