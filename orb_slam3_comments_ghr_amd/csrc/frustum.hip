// frustum.hip — Frame::isInFrustum over the local MapPoints of a frame on gfx950 (ref:src/Frame.cc:676-782,
// :1608-1705; the loop of Tracking::SearchLocalPoints, ref:src/Tracking.cc:4128-4151).
//
// k_frustum: grid (lanes, frame), one lane per (MapPoint, camera).  In a rig the two cameras of a MapPoint are
// the lanes 2 i and 2 i + 1, so the pair meets in one __shfl_xor for nToMatch ("in view in either camera") and
// both read the same coalesced SoA elements.  Every float expression is the reference's, in its order; the
// unit is built with -ffp-contract=off.  A 3-term sum runs left to right (Eigen's own association for fixed
// 3-vectors is unpinned: DESIGN.md §5).  The points' arrays are planes (x[n], y[n], z[n], ...): the host
// transposes pos / normal while it packs.
//
// The same kernel serves osg_frustum[_batch] here and osg_search_local_points[_batch] (match.hip), where its
// outputs are the query arrays k_match reads: frustum_common.h holds what the two share.
#include "batch_io.h"
#include "frustum_common.h"
#include "ransac_common.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void k_frustum(const FrProb *__restrict__ probs, int32_t *__restrict__ counts)
{
    const FrProb &P = probs[blockIdx.y];
    const int sh = P.two_cam ? 1 : 0;
    const int j = blockIdx.x * NT + threadIdx.x;
    const int i = j >> sh, cam = j & sh;
    const bool active = i < P.n;
    int st = OSG_FRUSTUM_NOT_CANDIDATE;
    if (active) {
        const FrCam &C = P.cam[cam];
        // what the reference leaves behind: -1 in the Nleft == -1 path's projection, nothing elsewhere
        float o_x = 0.f, o_y = 0.f, o_xr = 0.f, o_cos = 0.f, o_depth = 0.f;
        int o_lvl = -1;
        if (P.cand[i]) {
            const float X = P.px[i], Y = P.py[i], Z = P.pz[i];
            if (!sh) o_x = o_y = -1.f;  // :685-686
            const float pcx = ((C.R[0] * X + C.R[1] * Y) + C.R[2] * Z) + C.t[0];
            const float pcy = ((C.R[3] * X + C.R[4] * Y) + C.R[5] * Z) + C.t[1];
            const float pcz = ((C.R[6] * X + C.R[7] * Y) + C.R[8] * Z) + C.t[2];
            const float pc_dist = sqrtf((pcx * pcx + pcy * pcy) + pcz * pcz);
            const float invz = 1.0f / pcz;  // :699; read by the Nleft == -1 path only
            if (pcz < 0.0f) {
                st = OSG_FRUSTUM_NEG_DEPTH;
            } else {
                osg_camera cm;
                cm.type = C.type;
#pragma unroll
                for (int k = 0; k < 8; k++) cm.p[k] = C.p[k];
                float u, v;
                project_f(cm, pcx, pcy, pcz, u, v);
                if (u < P.min_x || u > P.max_x || v < P.min_y || v > P.max_y) {
                    st = OSG_FRUSTUM_OUTSIDE;
                } else {
                    if (!sh) o_x = u, o_y = v;  // :713-714, before the tests below
                    const float max_distance = 1.2f * P.maxd[i];
                    const float min_distance = 0.8f * P.mind[i];
                    const float pox = X - C.c[0], poy = Y - C.c[1], poz = Z - C.c[2];
                    const float dist = sqrtf((pox * pox + poy * poy) + poz * poz);
                    if (dist < min_distance || dist > max_distance) {
                        st = OSG_FRUSTUM_DISTANCE;
                    } else {
                        const float view_cos = ((pox * P.nx[i] + poy * P.ny[i]) + poz * P.nz[i]) / dist;
                        if (view_cos < P.limit) {
                            st = OSG_FRUSTUM_VIEW_COS;
                        } else {  // MapPoint::PredictScale, ref:src/MapPoint.cc:722-738
                            const float ratio = P.maxd[i] / dist;
                            int lvl = (int)ceilf(logf(ratio) / P.log_scale);
                            if (lvl < 0) lvl = 0;
                            else if (lvl >= P.n_levels) lvl = P.n_levels - 1;
                            st = OSG_FRUSTUM_IN_VIEW;
                            o_x = u, o_y = v, o_cos = view_cos, o_depth = pc_dist, o_lvl = lvl;
                            o_xr = u - P.mbf * invz;
                        }
                    }
                }
            }
        }
        // a rig's mTrackDepth keeps its earlier value where the left camera does not write it
        if (sh && cam == 0 && st != OSG_FRUSTUM_IN_VIEW) o_depth = P.prev_depth[i];
        if (P.status[cam]) P.status[cam][i] = (uint8_t)st;
        if (P.in_view[cam]) P.in_view[cam][i] = st == OSG_FRUSTUM_IN_VIEW;
        if (P.proj_x[cam]) P.proj_x[cam][i] = o_x;
        if (P.proj_y[cam]) P.proj_y[cam][i] = o_y;
        if (P.view_cos[cam]) P.view_cos[cam][i] = o_cos;
        if (P.depth[cam]) P.depth[cam][i] = o_depth;
        if (P.level[cam]) P.level[cam][i] = o_lvl;
        if (!sh && P.proj_xr) P.proj_xr[i] = o_xr;
    }
    // nToMatch: the MapPoints in view in either camera; every lane of the wave takes part in the exchange
    int seen = st == OSG_FRUSTUM_IN_VIEW;
    if (sh) seen |= __shfl_xor(seen, 1);
    const unsigned long long m = __ballot(active && cam == 0 && seen);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[blockIdx.y], (int32_t)__popcll(m));
}

int frustum_run(osg_ctx *ctx, const osg_frustum_frame *frames, const osg_frustum_points *points, int B, float limit,
                osg_frustum_result *results)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, B >= 0 && B <= 65535 && (B == 0 || (frames && points && results)), "batch size / null argument");
    std::vector<FrBlock> L(B);
    std::vector<size_t> in_off(B + 1, 0), out_off(B + 1, 0);
    int max_lanes = 0;
    for (int b = 0; b < B; b++) {
        OSG_RC(osg_frustum_check_args(ctx, &frames[b], &points[b], b));
        const bool rig = frames[b].two_cam != 0;
        L[b] = osg_frustum_block(points[b].n, rig);
        in_off[b + 1] = in_off[b] + L[b].in_end;
        out_off[b + 1] = out_off[b] + (L[b].total - L[b].in_end);
        max_lanes = std::max(max_lanes, points[b].n << (rig ? 1 : 0));
        results[b].n_to_match = 0;
    }
    ctx->last_kernel_ms = 0;
    if (max_lanes == 0) return OSG_OK;
    osg_batch_io io(ctx);
    const osg_seg s_prob = io.in(sizeof(FrProb), B), s_in = io.in(1, in_off[B]);
    const osg_seg s_cnt = io.out(sizeof(int32_t), B), s_out = io.out(1, out_off[B]);
    OSG_RC(io.stage());
    // the device blocks' addresses go into the kernel arguments, so they are taken before the upload
    char *din = nullptr, *dout = nullptr;
    OSG_ALLOC(ctx, din, SLOT_BA0, io.in_bytes);
    OSG_ALLOC(ctx, dout, SLOT_BA1, io.out_bytes);
    FrProb *hp = io.host_in<FrProb>(s_prob);
    for (int b = 0; b < B; b++) {
        osg_frustum_pack_inputs(io.host_in<char>(s_in, in_off[b]), L[b], &points[b]);
        hp[b] = osg_frustum_prob(&frames[b], points[b].n, limit, L[b], din + s_in.off + in_off[b],
                                 dout + s_out.off + out_off[b]);
    }
    OSG_RC(io.upload());
    OSG_RC(io.start());
    OSG_RC(osg_frustum_enqueue(ctx, io.dev_in<FrProb>(s_prob), io.dev_out<int32_t>(s_cnt), B, max_lanes, true));
    OSG_RC(io.finish(io.out_bytes));
    for (int b = 0; b < B; b++) {
        results[b].n_to_match = *io.result<int32_t>(s_cnt, b);
        osg_frustum_unpack(io.result<char>(s_out, out_off[b]), L[b], points[b].n, frames[b].two_cam != 0, &results[b]);
    }
    return OSG_OK;
}

}  // namespace

int osg_frustum_enqueue(osg_ctx *ctx, const FrProb *d_probs, int32_t *d_counts, int B, int max_lanes, bool zero_counts)
{
    if (zero_counts) OSG_HIP_CHECK(ctx, hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)B, ctx->stream));
    hipLaunchKernelGGL(k_frustum, dim3((max_lanes + NT - 1) / NT, B), dim3(NT), 0, ctx->stream, d_probs, d_counts);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    return OSG_OK;
}

extern "C" {

int osg_frustum(osg_ctx *ctx, const osg_frustum_frame *frame, const osg_frustum_points *points, float view_cos_limit,
                osg_frustum_result *result)
{
    const int rc = frustum_run(ctx, frame, points, 1, view_cos_limit, result);
    return rc < 0 ? rc : result->n_to_match;
}

int osg_frustum_batch(osg_ctx *ctx, const osg_frustum_frame *frames, const osg_frustum_points *points, int32_t B,
                      float view_cos_limit, osg_frustum_result *results)
{
    return frustum_run(ctx, frames, points, B, view_cos_limit, results);
}

int osg_frustum_check(const osg_frustum_frame *frame, const osg_frustum_points *points)
{
    return osg_frustum_check_args(nullptr, frame, points, 0);
}

}  // extern "C"
