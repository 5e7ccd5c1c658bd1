// Whole-chip rate of the headline top-2 step on the two FP4 block-scaled MFMA shapes, at the same output tile per
// wave (32 rows x 64 queries of 256-bit keys per step):
//   32 x 32 x 64:  two query tiles, per tile a chain of 4 MFMAs (32 cycles each) beside the other tile's 21 key
//                  updates on the row tile before, A from LDS by four ds_read_b128 per row tile at the 144-B row
//                  stride (k_top2_fp4q2's loop; mfma_fp4_rate.hip mode 8 with the shared A fragments);
//   16 x 16 x 128: the same tile as 2 row sub-tiles x 4 query sub-tiles, two K = 128 MFMAs (16 cycles) each; per
//                  query tile (two sub-tiles) a chain of 8 MFMAs into four sub-accumulators beside the other
//                  tile's 22 updates, spread behind MFMAs 2-8; A by four ds_read_b128 per row tile, row
//                  (l & 15) + 16 rs, 16 B at 64 kh + 16 (l >> 4), at a 160-B row stride (every lane group of the
//                  read on 64 distinct banks).
// Modes 0 / 1 are the bare chains of either shape (operands in registers, no update), 2 / 3 the patterns above.
// Every loop also runs without block scales (constant zero scale operands select v_mfma_f32_..._f8f6f4; C then
// carries the bias and the row 2^-12 times as large, BIAS_U): what the second instruction word of the scaled
// form costs in vector issue.
// One 1024-thread workgroup per CU at a time (16 waves, 4 per SIMD: the LDS ring's size keeps a second one
// out), 8 workgroups per CU per launch, random-ish operands (the clock the chip holds depends on the data).
// The same four loops then run at one wave per SIMD (256-thread workgroups), which shows a single wave's issue pace.
// Every measurement is most of a second of back-to-back launches, the modes alternate, three repeats; every wave
// stamps s_memtime / s_memrealtime around its loop: the quotient x 100 MHz is the in-kernel clock, and the longest
// loop of a workgroup its cycles.
// Build: hipcc --offload-arch=gfx950 -O3 mfma_fp4_16_rate.hip -o mfma_fp4_16_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int ROWS = 768;                     // three 256-row slots
constexpr int SCALES = 139 | (127 << 8) | (127 << 16);
constexpr float BIAS = 10485760.0f;           // 2^23 + 2^21
constexpr float BIAS_U = 3072.0f;             // the unscaled forms' keys: the same bit patterns 12 binades down

__device__ __forceinline__ void push2f(int &k1, int &k2, int x, int y)
{
    const int m = __float_as_int(__builtin_amdgcn_fmed3f(__int_as_float(k1), __int_as_float(x), __int_as_float(y)));
    k1 = min(min(x, y), k1);
    k2 = min(m, k2);
}

__device__ __forceinline__ uint32_t mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// MODE 0: bare 32 x 32 x 64 chains; 2: the k_top2_fp4q2 step
template <int MODE, int SC>
__global__ __launch_bounds__(1024) void k_32(float *out, unsigned long long *stamp, int iters)
{
    constexpr int RS = 144;
    __shared__ __attribute__((aligned(16))) unsigned char s_buf[ROWS * 160];
    const int t = threadIdx.x, l = t & 63, r = l & 31, h = l >> 5;
    for (int e = t; e < ROWS * 160 / 4; e += blockDim.x) ((uint32_t *)s_buf)[e] = (mix(e * 2654435761u + blockIdx.x) & 0x44444444u) * 3u;
    i32x8 bq[2][4];
    for (int j = 0; j < 2; j++)
        for (int s = 0; s < 4; s++)
            for (int d = 0; d < 8; d++)
                bq[j][s][d] = d < 4 ? (int)(0x22222222u | (mix(t * 977u + j * 131u + s * 17u + d) & 0x88888888u)) : 0;
    f32x16 crow;
    for (int i = 0; i < 16; i++) crow[i] = SC ? BIAS + (float)((i & 3) + 8 * (i >> 2) + 4 * h) : BIAS_U + (float)((i & 3) + 8 * (i >> 2) + 4 * h) / 4096.f;
    const int lbase = r * RS + h * 16;
    __syncthreads();
    auto frag = [&](int off, int s) -> i32x8 {
        const i32x4 v = *(const i32x4 *)(s_buf + lbase + off + 32 * s);
        return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    };
    auto mfma = [&](const i32x8 &a, const i32x8 &b, const f32x16 &c) {
        if (SC) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, SCALES, 1, SCALES);
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, 0, 0, 0);
    };
    int k1[2] = {0x7fffffff, 0x7fffffff}, k2[2] = {0x7fffffff, 0x7fffffff};
    auto pushk = [&](int j, const f32x16 &acc, int s) {
        const int lo = s == 0 ? 0 : 3 * (s - 1), hi = s == 0 ? 0 : (s == 3 ? 8 : 3 * s);
#pragma unroll
        for (int p = lo; p < hi; p++) {
            const int e = (p & 1) * 8 + 2 * (p >> 1);
            push2f(k1[j], k2[j], __float_as_int(acc[e]), __float_as_int(acc[e + 1]));
        }
        if (s == 3) k1[j] -= 32;
    };
    i32x8 a[4];
    for (int s = 0; s < 4; s++) a[s] = frag(0, s);
    f32x16 acc0 = crow, acc1 = crow;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; it++) {
        const int nb = ((it + 1) % (ROWS / 32)) * 32 * RS;
        if (MODE == 0) {
#pragma unroll
            for (int s = 0; s < 4; s++) acc0 = mfma(a[s], bq[0][s], s ? acc0 : crow);
#pragma unroll
            for (int s = 0; s < 4; s++) acc1 = mfma(a[s], bq[1][s], s ? acc1 : crow);
            for (int s = 0; s < 4; s++) asm volatile("" : "+v"(a[s]));
            asm volatile("" : : "v"(acc0), "v"(acc1));   // every iteration's chains stay, at no instruction
        } else {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                acc0 = mfma(a[s], bq[0][s], s ? acc0 : crow);
                __builtin_amdgcn_sched_barrier(0);
                pushk(1, acc1, s);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                acc1 = mfma(a[s], bq[1][s], s ? acc1 : crow);
                a[s] = frag(nb, s);
                __builtin_amdgcn_sched_barrier(0);
                pushk(0, acc0, s);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (l == 0) {
        stamp[2 * (blockIdx.x * 16 + (t >> 6))] = c1 - c0;
        stamp[2 * (blockIdx.x * 16 + (t >> 6)) + 1] = r1 - r0;
    }
    out[blockIdx.x * 1024 + t] = (float)(k1[0] + k2[0] + k1[1] + k2[1]) + acc0[l & 15] + acc1[l & 15];
}

// MODE 1: bare 16 x 16 x 128 chains; 3: the same step on that shape
template <int MODE, int SC>
__global__ __launch_bounds__(1024) void k_16(float *out, unsigned long long *stamp, int iters)
{
    constexpr int RS = 160;
    __shared__ __attribute__((aligned(16))) unsigned char s_buf[ROWS * 160];
    const int t = threadIdx.x, l = t & 63, m = l & 15, g = l >> 4;
    for (int e = t; e < ROWS * 160 / 4; e += blockDim.x) ((uint32_t *)s_buf)[e] = (mix(e * 2654435761u + blockIdx.x) & 0x44444444u) * 3u;
    i32x8 bq[4][2];   // [query sub-tile][K half]
    for (int qs = 0; qs < 4; qs++)
        for (int kh = 0; kh < 2; kh++)
            for (int d = 0; d < 8; d++)
                bq[qs][kh][d] = d < 4 ? (int)(0x22222222u | (mix(t * 977u + qs * 131u + kh * 17u + d) & 0x88888888u)) : 0;
    f32x4 crow[2];
    for (int rs = 0; rs < 2; rs++)
        for (int i = 0; i < 4; i++) crow[rs][i] = SC ? BIAS + (float)(16 * rs + 4 * g + i) : BIAS_U + (float)(16 * rs + 4 * g + i) / 4096.f;
    const int lbase = m * RS + g * 16;
    __syncthreads();
    auto frag = [&](int off, int rs, int kh) -> i32x8 {
        const i32x4 v = *(const i32x4 *)(s_buf + lbase + off + rs * 16 * RS + 64 * kh);
        return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    };
    auto mfma = [&](const i32x8 &a, const i32x8 &b, const f32x4 &c) {
        if (SC) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 4, 0, SCALES, 1, SCALES);
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 4, 0, 0, 0, 0);
    };
    int k1[4], k2[4];
    for (int qs = 0; qs < 4; qs++) k1[qs] = k2[qs] = 0x7fffffff;
    f32x4 acc[2][2][2];   // [query tile][row sub-tile][query sub-tile of the tile]
    for (int j = 0; j < 2; j++)
        for (int rs = 0; rs < 2; rs++)
            for (int q2 = 0; q2 < 2; q2++) acc[j][rs][q2] = crow[rs];
    // MFMA n of query tile j's chain: K half n >> 2, row sub-tile (n >> 1) & 1, query sub-tile n & 1: a
    // sub-accumulator's second MFMA issues four MFMAs behind its first
    auto chain = [&](int j, int n, i32x8 (&a)[2][2]) {
        const int kh = n >> 2, rs = (n >> 1) & 1, q2 = n & 1;
        acc[j][rs][q2] = mfma(a[rs][kh], bq[2 * j + q2][kh], kh ? acc[j][rs][q2] : crow[rs]);
    };
    // update op n of 22 on query tile j's sub-accumulators, in the order their last MFMAs issued: per sub-accumulator
    // two medians, two min3 and one min3 into the second key; then the two rebases
    int ma = 0, mb = 0;
    auto upd = [&](int j, int n) {
        if (n >= 20) {
            k1[2 * j + (n - 20)] -= 32;
            return;
        }
        const int grp = n / 5, o = n % 5, rs = grp >> 1, q2 = grp & 1, qs = 2 * j + q2;
        const f32x4 &v = acc[j][rs][q2];
        const int x0 = __float_as_int(v[0]), x1 = __float_as_int(v[1]), x2 = __float_as_int(v[2]), x3 = __float_as_int(v[3]);
        auto med = [](int a, int b, int c) {
            return __float_as_int(__builtin_amdgcn_fmed3f(__int_as_float(a), __int_as_float(b), __int_as_float(c)));
        };
        switch (o) {
        case 0: ma = med(k1[qs], x0, x1); break;
        case 1: k1[qs] = min(min(x0, x1), k1[qs]); break;
        case 2: mb = med(k1[qs], x2, x3); break;
        case 3: k1[qs] = min(min(x2, x3), k1[qs]); break;
        default: k2[qs] = min(min(ma, mb), k2[qs]); break;
        }
    };
    // the ops behind MFMA n of the other chain: none behind the first, 3 behind MFMAs 2-7, 4 behind the last
    auto upds = [&](int j, int n) {
        if (n == 0) return;
        const int lo = 3 * (n - 1), hi = n == 7 ? 22 : 3 * n;
#pragma unroll
        for (int o = lo; o < hi; o++) upd(j, o);
    };
    i32x8 a[2][2];
    for (int rs = 0; rs < 2; rs++)
        for (int kh = 0; kh < 2; kh++) a[rs][kh] = frag(0, rs, kh);
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; it++) {
        const int nb = ((it + 1) % (ROWS / 32)) * 32 * RS;
        if (MODE == 1) {
#pragma unroll
            for (int n = 0; n < 8; n++) chain(0, n, a);
#pragma unroll
            for (int n = 0; n < 8; n++) chain(1, n, a);
            for (int rs = 0; rs < 2; rs++)
                for (int kh = 0; kh < 2; kh++) asm volatile("" : "+v"(a[rs][kh]));
            for (int j = 0; j < 2; j++)   // every iteration's chains stay, at no instruction
                for (int rs = 0; rs < 2; rs++) asm volatile("" : : "v"(acc[j][rs][0]), "v"(acc[j][rs][1]));
        } else {
#pragma unroll
            for (int n = 0; n < 8; n++) {
                chain(0, n, a);
                __builtin_amdgcn_sched_barrier(0);
                upds(1, n);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int n = 0; n < 8; n++) {
                chain(1, n, a);
                // a[rs][kh] has fed its last MFMA of this row tile when the chain passes its second query sub-tile
                if (n & 1) a[(n >> 1) & 1][n >> 2] = frag(nb, (n >> 1) & 1, n >> 2);
                __builtin_amdgcn_sched_barrier(0);
                upds(0, n);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (l == 0) {
        stamp[2 * (blockIdx.x * 16 + (t >> 6))] = c1 - c0;
        stamp[2 * (blockIdx.x * 16 + (t >> 6)) + 1] = r1 - r0;
    }
    float s = 0;
    for (int j = 0; j < 2; j++)
        for (int rs = 0; rs < 2; rs++)
            for (int q2 = 0; q2 < 2; q2++) s += acc[j][rs][q2][l & 3];
    out[blockIdx.x * 1024 + t] = (float)(k1[0] + k2[0] + k1[1] + k2[1] + k1[2] + k2[2] + k1[3] + k2[3]) + s;
}

struct Result { double ms, ghz, cyc; };

// NW waves per workgroup (16: four per SIMD; 4: one per SIMD).  cyc: the median over the workgroups of the longest
// of a workgroup's wave loops in s_memtime ticks (the oldest wave of a SIMD issues first and leaves its loop early,
// so one wave's stamps alone read low); ghz: the median of the workgroups' summed tick quotients x 100 MHz
template <class K>
Result run(K kern, float *d, unsigned long long *ds, int iters, int G, int NW, int warm, int reps)
{
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int r = 0; r < warm; r++) hipLaunchKernelGGL(kern, dim3(G), dim3(NW * 64), 0, 0, d, ds, iters);
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL(kern, dim3(G), dim3(NW * 64), 0, 0, d, ds, iters);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(2 * 16 * G);
    (void)hipMemcpy(h.data(), ds, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> ghz(G), cyc(G);
    for (int i = 0; i < G; i++) {
        double c = 0, rt = 0, cmax = 0;
        for (int w = 0; w < NW; w++) {
            c += (double)h[2 * (16 * i + w)];
            rt += (double)h[2 * (16 * i + w) + 1];
            cmax = std::max(cmax, (double)h[2 * (16 * i + w)]);
        }
        ghz[i] = rt > 0 ? c / rt * 0.1 : 0.0;
        cyc[i] = cmax;
    }
    std::nth_element(ghz.begin(), ghz.begin() + G / 2, ghz.end());
    std::nth_element(cyc.begin(), cyc.begin() + G / 2, cyc.end());
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return {ms / reps, ghz[G / 2], cyc[G / 2]};
}

int main()
{
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const int G = 8 * ncu, warm = 100, reps = 200;
    float *d;
    unsigned long long *ds;
    (void)hipMalloc(&d, sizeof(float) * G * 1024);
    (void)hipMalloc(&ds, 16 * 16 * G);
    const char *nm[4] = {"32x32x64 bare chains", "16x16x128 bare chains", "32x32x64 step (chain beside updates, A from LDS)",
                         "16x16x128 step (chain beside updates, A from LDS)"};
    for (int rep = 0; rep < 3; rep++)
        for (int m = 0; m < 16; m++) {
            // modes 4-7: modes 0-3 at one wave per SIMD, four times the steps per wave; 8-15: 0-7 without block scales
            const int NW = m % 8 < 4 ? 16 : 4, iters = m % 8 < 4 ? 512 : 2048, sc = m < 8;
            const Result r = m % 4 == 0   ? run(sc ? k_32<0, 1> : k_32<0, 0>, d, ds, iters, G, NW, warm, reps)
                             : m % 4 == 1 ? run(sc ? k_16<1, 1> : k_16<1, 0>, d, ds, iters, G, NW, warm, reps)
                             : m % 4 == 2 ? run(sc ? k_32<2, 1> : k_32<2, 0>, d, ds, iters, G, NW, warm, reps)
                                          : run(sc ? k_16<3, 1> : k_16<3, 0>, d, ds, iters, G, NW, warm, reps);
            // one step = 32 rows x 64 queries x 256 bits = two 32 x 32 tiles of 262144 (query, row, bit) MACs;
            // simd_cycles_per_step: the SIMD's cycles per step of one of its waves (matrix pipe alone: 256)
            const double tiles = (double)G * NW * iters * 2;
            printf("{\"mode\": \"%s\", \"block_scales\": %d, \"waves_per_simd\": %d, \"repeat\": %d, \"ms\": %.4f, \"ns_per_tile_per_simd\": %.3f, "
                   "\"Tmatch_bits_per_s\": %.1f, \"simd_cycles_per_step\": %.1f, \"in_kernel_GHz\": %.3f}\n",
                   nm[m % 4], sc, NW / 4, rep, r.ms, r.ms * 1e6 / (tiles / (4.0 * ncu)), tiles * 262144 / (r.ms * 1e-3) / 1e12,
                   r.cyc / iters / (NW / 4), r.ghz);
            fflush(stdout);
        }
    (void)hipFree(d);
    (void)hipFree(ds);
    return 0;
}
