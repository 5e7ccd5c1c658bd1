// preintegration_driver.cpp — Tracking::PreintegrateIMU, the reintegration of InertialOptimization's write-back and
// MergePrevious through the ORB-SLAM3-side adapter on mock objects (test-only; tests/test_adapter_preintegration.py).
//   list        <in> <out>   imu_frame_list alone (host code, no device): the queue after the call,
//                            mvImuFromLastFrame, the integrables, setIntegrated
//   todo        <in> <out>   keyframes_to_reintegrate alone (host code): which KeyFrames pass the 0.01 test, the
//                            biases SetNewBias left
//   track       <in> <out>   preintegrate_imu: both hand-overs as the caller sees them
//   reintegrate <in> <out>   reintegrate_keyframes
//   merge       <in> <out>   merge_previous
#include "driver_common.h"
#include "mock_preintegration.h"

namespace {

using mockimu::Hooks;
using mockimu::Preintegrated;

std::vector<float> state_row(const Preintegrated &p)
{
    const float *f = reinterpret_cast<const float *>(&p.st);
    std::vector<float> v(f, f + sizeof p.st / sizeof(float));
    v.insert(v.end(), p.bu, p.bu + 6), v.insert(v.end(), p.db, p.db + 6);
    return v;
}

// a preintegration from "<pre>.state" (osg_imu_preintegrated as floats), "<pre>.bu" and "<pre>.meas"
Preintegrated *load(const Arrays &in, const std::string &pre, const float *nga, const float *walk)
{
    const float zero[6] = {};
    auto *p = new Preintegrated(zero, nga, walk);
    std::memcpy(&p->st, get(in, pre + ".state").p<float>(), sizeof p->st);
    p->SetNewBias(get(in, pre + ".bu").p<float>());
    const Arr &m = get(in, pre + ".meas");
    p->meas.assign(m.p<float>(), m.p<float>() + m.n);
    return p;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: preintegration_driver list|todo|track|reintegrate|merge <in> <out>\n");
        return 2;
    }
    static_assert(sizeof(osg_imu_preintegrated) == sizeof(float) * 298, "packed float fields");
    const std::string mode = argv[1];
    const Arrays in = read_arrays(argv[2]);
    const float *noise = get(in, "noise").p<float>();  // nga, nga_walk
    Arrays out;
    if (mode == "list" || mode == "track") {
        mockimu::Tracking T;
        mockimu::Frame prev;
        mockimu::KeyFrame KF;
        const double *ts = get(in, "frames").p<double>();  // t_prev, t_cur, has a previous frame
        prev.mTimeStamp = ts[0];
        T.mCurrentFrame.mTimeStamp = ts[1];
        T.mCurrentFrame.mpPrevFrame = ts[2] != 0 ? &prev : nullptr;
        std::memcpy(T.mCurrentFrame.nga, noise, 24), std::memcpy(T.mCurrentFrame.walk, noise + 6, 24);
        std::memcpy(T.mLastFrame.bias, get(in, "last_bias").p<float>(), 24);
        T.mpLastKeyFrame = &KF;
        const Arr &qa = get(in, "queue.aw");
        const double *qt = get(in, "queue.t").p<double>();
        for (size_t i = 0; i < qa.n / 6; i++) {
            mockimu::Point m;
            std::memcpy(m.a, qa.p<float>() + 6 * i, 12), std::memcpy(m.w, qa.p<float>() + 6 * i + 3, 12);
            m.t = qt[i];
            T.mlQueueImuData.push_back(m);
        }
        T.mvImuFromLastFrame.resize(3);  // stale content the call must clear
        T.mpImuPreintegratedFromLastKF = load(in, "from_kf", noise, noise + 6);
        std::vector<float> meas;
        const int ret = mode == "list" ? osg_orbslam3::imu_frame_list<Hooks>(T, meas)
                                       : osg_orbslam3::preintegrate_imu<Hooks>(T);
        if (mode == "track" && osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        std::vector<double> left, took;
        for (const auto &m : T.mlQueueImuData) left.push_back(m.t);
        for (const auto &m : T.mvImuFromLastFrame) took.push_back(m.t);
        const mockimu::Frame &F = T.mCurrentFrame;
        out["ret"] = make('i', std::vector<int32_t>{ret, F.integrated, F.mpImuPreintegratedFrame != nullptr,
                                                    F.mpImuPreintegrated == T.mpImuPreintegratedFromLastKF,
                                                    F.mpLastKeyFrame == &KF, Preintegrated::live});
        out["queue.t"] = make('d', left);
        out["taken.t"] = make('d', took);
        out["meas"] = make('f', meas);
        out["from_kf.state"] = make('f', state_row(*T.mpImuPreintegratedFromLastKF));
        out["from_kf.meas"] = make('f', T.mpImuPreintegratedFromLastKF->meas);
        if (F.mpImuPreintegratedFrame) {
            out["frame.state"] = make('f', state_row(*F.mpImuPreintegratedFrame));
            out["frame.meas"] = make('f', F.mpImuPreintegratedFrame->meas);
            delete F.mpImuPreintegratedFrame;
        }
        delete T.mpImuPreintegratedFromLastKF;
    } else if (mode == "todo" || mode == "reintegrate") {
        const int32_t n = get(in, "n_kf").p<int32_t>()[0];
        const float *kb = get(in, "kf.bias").p<float>();
        const int32_t *has_pre = get(in, "kf.has").p<int32_t>();
        std::vector<mockimu::KeyFrame> kfs(n);
        std::vector<mockimu::KeyFrame *> vp;
        for (int i = 0; i < n; i++) {
            std::memcpy(kfs[i].bias, kb + 6 * i, 24);
            if (has_pre[i]) {
                kfs[i].mpImuPreintegrated = load(in, "kf" + std::to_string(i), noise, noise + 6);
            }
            vp.push_back(&kfs[i]);
        }
        const float *b = get(in, "new_bias").p<float>();
        std::vector<int32_t> picked;
        int ret;
        if (mode == "todo") {
            const auto todo = osg_orbslam3::keyframes_to_reintegrate<Hooks>(vp, b);
            ret = (int)todo.size();
            for (auto *p : todo)
                for (int i = 0; i < n; i++)
                    if (kfs[i].mpImuPreintegrated == p) picked.push_back(i);
        } else {
            ret = osg_orbslam3::reintegrate_keyframes<Hooks>(vp, b);
            if (osg_orbslam3::thread_ctx() == nullptr) {
                std::fprintf(stderr, "no device context\n");
                return 3;
            }
        }
        out["ret"] = make('i', std::vector<int32_t>{ret});
        out["picked"] = make('i', picked);
        std::vector<float> biases;
        for (int i = 0; i < n; i++) {
            biases.insert(biases.end(), kfs[i].bias, kfs[i].bias + 6);
            if (!kfs[i].mpImuPreintegrated) continue;
            out["kf" + std::to_string(i) + ".state"] = make('f', state_row(*kfs[i].mpImuPreintegrated));
            out["kf" + std::to_string(i) + ".meas"] = make('f', kfs[i].mpImuPreintegrated->meas);
            delete kfs[i].mpImuPreintegrated;
        }
        out["kf.bias"] = make('f', biases);
    } else if (mode == "merge") {
        Preintegrated *prev = load(in, "prev", noise, noise + 6), *cur = load(in, "cur", noise, noise + 6);
        osg_orbslam3::merge_previous<Hooks>(cur, cur);  // pPrev == this: nothing happens
        out["self.state"] = make('f', state_row(*cur));
        osg_orbslam3::merge_previous<Hooks>(cur, prev);
        if (osg_orbslam3::thread_ctx() == nullptr) {
            std::fprintf(stderr, "no device context\n");
            return 3;
        }
        out["cur.state"] = make('f', state_row(*cur));
        out["cur.meas"] = make('f', cur->meas);
        out["prev.state"] = make('f', state_row(*prev));
        delete prev;
        delete cur;
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    write_arrays(argv[3], out);
    return 0;
}
