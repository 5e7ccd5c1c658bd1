// frustum_common.h — what frustum.hip (k_frustum, osg_frustum[_batch]) and match.hip (osg_search_local_points,
// the fused step) share: the per-problem kernel arguments, the layout of a problem's SoA arrays inside a device
// block, the argument checks and the launch.  Host-side code here needs no device.
#pragma once
#include <cstring>

#include "osg_internal.h"

// one camera of k_frustum: Pc = R P + t, PO = P - c, uv = project(Pc)
struct FrCam {
    float R[9], t[3], c[3];
    int32_t type;
    float p[8];
};

// one problem (frame) of a k_frustum launch; every pointer is a device address, outputs may be null
struct FrProb {
    FrCam cam[2];
    float min_x, max_x, min_y, max_y, mbf, log_scale, limit;
    int32_t n_levels, two_cam, n;
    const float *px, *py, *pz, *nx, *ny, *nz, *maxd, *mind, *prev_depth;
    const uint8_t *cand;
    uint8_t *status[2], *in_view[2];
    float *proj_x[2], *proj_y[2], *proj_xr, *view_cos[2], *depth[2];
    int32_t *level[2];
};

// Where a problem's arrays lie inside one block, each 256-byte aligned: the inputs first ([0, in_end)), then the
// outputs.  The right camera's outputs exist only for a rig; proj_xr (u - mbf * invz) only without one.
struct FrBlock {
    size_t px, py, pz, nx, ny, nz, maxd, mind, prev_depth, cand, in_end;
    size_t status[2], in_view[2], proj_x[2], proj_y[2], proj_xr, view_cos[2], depth[2], level[2];
    size_t total;
};

inline FrBlock osg_frustum_block(int n, bool two_cam)
{
    FrBlock L{};
    size_t at = 0;
    auto take = [&](size_t elem) {
        const size_t o = at;
        at += (elem * (size_t)n + 255) & ~size_t(255);
        return o;
    };
    L.px = take(4), L.py = take(4), L.pz = take(4), L.nx = take(4), L.ny = take(4), L.nz = take(4);
    L.maxd = take(4), L.mind = take(4), L.prev_depth = take(4), L.cand = take(1);
    L.in_end = at;
    for (int c = 0; c < (two_cam ? 2 : 1); c++) {
        L.status[c] = take(1), L.in_view[c] = take(1);
        L.proj_x[c] = take(4), L.proj_y[c] = take(4), L.view_cos[c] = take(4), L.depth[c] = take(4), L.level[c] = take(4);
    }
    if (!two_cam) L.proj_xr = take(4);
    L.total = at;
    return L;
}

// the input part of a problem's block, from the caller's arrays (pos / normal transposed to planes)
inline void osg_frustum_pack_inputs(char *in_block, const FrBlock &L, const osg_frustum_points *pts)
{
    const int n = pts->n;
    float *px = (float *)(in_block + L.px), *py = (float *)(in_block + L.py), *pz = (float *)(in_block + L.pz);
    float *nx = (float *)(in_block + L.nx), *ny = (float *)(in_block + L.ny), *nz = (float *)(in_block + L.nz);
    for (int i = 0; i < n; i++) {
        px[i] = pts->pos[3 * i], py[i] = pts->pos[3 * i + 1], pz[i] = pts->pos[3 * i + 2];
        nx[i] = pts->normal[3 * i], ny[i] = pts->normal[3 * i + 1], nz[i] = pts->normal[3 * i + 2];
    }
    if (n == 0) return;
    std::memcpy(in_block + L.maxd, pts->max_dist, sizeof(float) * n);
    std::memcpy(in_block + L.mind, pts->min_dist, sizeof(float) * n);
    if (pts->prev_depth) std::memcpy(in_block + L.prev_depth, pts->prev_depth, sizeof(float) * n);
    else std::memset(in_block + L.prev_depth, 0, sizeof(float) * n);
    std::memcpy(in_block + L.cand, pts->candidate, n);
}

// the kernel arguments of one problem whose inputs start at d_in and whose outputs at d_out - L.in_end
// (so that d_out + (L.x - L.in_end) is output x); the two may be parts of different device buffers
inline FrProb osg_frustum_prob(const osg_frustum_frame *f, int n, float limit, const FrBlock &L, char *d_in, char *d_out)
{
    FrProb p{};
    const bool rig = f->two_cam != 0;
    for (int c = 0; c < 2; c++) {
        std::memcpy(p.cam[c].R, f->cam[c].R, sizeof p.cam[c].R);
        std::memcpy(p.cam[c].t, f->cam[c].t, sizeof p.cam[c].t);
        std::memcpy(p.cam[c].c, f->cam[c].c, sizeof p.cam[c].c);
        std::memcpy(p.cam[c].p, f->cam[c].cam, sizeof p.cam[c].p);
        p.cam[c].type = f->cam[c].cam_type;
    }
    p.min_x = f->min_x, p.max_x = f->max_x, p.min_y = f->min_y, p.max_y = f->max_y;
    p.mbf = f->mbf, p.log_scale = f->log_scale_factor, p.limit = limit;
    p.n_levels = f->n_levels, p.two_cam = rig, p.n = n;
    auto in = [&](size_t o) { return (const float *)(d_in + o); };
    p.px = in(L.px), p.py = in(L.py), p.pz = in(L.pz), p.nx = in(L.nx), p.ny = in(L.ny), p.nz = in(L.nz);
    p.maxd = in(L.maxd), p.mind = in(L.mind), p.prev_depth = in(L.prev_depth);
    p.cand = (const uint8_t *)(d_in + L.cand);
    char *o = d_out - L.in_end;
    for (int c = 0; c < (rig ? 2 : 1); c++) {
        p.status[c] = (uint8_t *)(o + L.status[c]), p.in_view[c] = (uint8_t *)(o + L.in_view[c]);
        p.proj_x[c] = (float *)(o + L.proj_x[c]), p.proj_y[c] = (float *)(o + L.proj_y[c]);
        p.view_cos[c] = (float *)(o + L.view_cos[c]), p.depth[c] = (float *)(o + L.depth[c]);
        p.level[c] = (int32_t *)(o + L.level[c]);
    }
    if (!rig) p.proj_xr = (float *)(o + L.proj_xr);
    return p;
}

// a problem's results from the downloaded output part of its block (host_out + (L.x - L.in_end) is output x)
inline void osg_frustum_unpack(const char *host_out, const FrBlock &L, int n, bool two_cam, osg_frustum_result *r)
{
    const char *o = host_out - L.in_end;
    auto get = [&](void *dst, size_t off, size_t elem) {
        if (dst && n > 0) std::memcpy(dst, o + off, elem * (size_t)n);
    };
    for (int c = 0; c < (two_cam ? 2 : 1); c++) {
        get(r->status[c], L.status[c], 1);
        get(r->proj_x[c], L.proj_x[c], 4), get(r->proj_y[c], L.proj_y[c], 4);
        get(r->view_cos[c], L.view_cos[c], 4), get(r->depth[c], L.depth[c], 4), get(r->level[c], L.level[c], 4);
    }
    if (!two_cam) get(r->proj_xr, L.proj_xr, 4);
}

// argument checks of problem b (ctx may be null: osg_frustum_check)
inline int osg_frustum_check_args(osg_ctx *ctx, const osg_frustum_frame *f, const osg_frustum_points *pts, int b)
{
    OSG_REQUIRE(ctx, f && pts, "problem %d: null frame or points", b);
    OSG_REQUIRE(ctx, pts->n >= 0 && pts->n <= (1 << 24), "problem %d: %d points (limit 2^24)", b, pts->n);
    OSG_REQUIRE(ctx, f->n_levels > 0 && f->n_levels <= 128, "problem %d: n_levels = %d", b, f->n_levels);
    for (int c = 0; c < (f->two_cam ? 2 : 1); c++)
        OSG_REQUIRE(ctx, f->cam[c].cam_type == 0 || f->cam[c].cam_type == 1, "problem %d: camera %d type %d", b, c,
                    f->cam[c].cam_type);
    OSG_REQUIRE(ctx, pts->n == 0 || (pts->pos && pts->normal && pts->max_dist && pts->min_dist && pts->candidate),
                "problem %d: null point arrays", b);
    return OSG_OK;
}

// frustum.hip
// runs k_frustum over d_probs[B] on ctx->stream; n_to_match of problem b is added to d_counts[b], which is zeroed
// on the stream first when zero_counts (else the caller uploaded zeros).  max_lanes: the largest n (2 n in a rig)
// of the problems, > 0
int osg_frustum_enqueue(osg_ctx *ctx, const FrProb *d_probs, int32_t *d_counts, int B, int max_lanes, bool zero_counts);
