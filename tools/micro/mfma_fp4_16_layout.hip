// FP4 (e2m1) block-scaled MFMA on gfx950, the 16 x 16 form: operand, scale and C / D maps of
// v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 4), tested with exact data as mfma_fp4_layout.hip does
// for the 32 x 32 x 64 form.
//   Random A (16 x 128) and B (128 x 16) with entries in {-2, -1, 0, 1, 2} are packed on the host by a
//   candidate map (lane l holds row / column l & 15 and 32 nibbles j of K block l >> 4; k = f(l >> 4, j);
//   nibble j in register j >> 3 at bit 4 (j & 7)), C is 1000 m + n, one MFMA runs, and D is compared with
//   the host's A B + C under the candidate C / D map: column l & 15, row 4 (l >> 4) + i.
//   A dot product is unchanged by a K permutation applied to both operands alike, so every consistent K map
//   passes; `mixed` packs A by one map and B by another and must fail (the probe can tell maps apart).
//   `transposed` reads D as row l & 15, column 4 (l >> 4) + i and must fail (A is the row operand).
//   Scales: 127 = 1.0, 139 = 2^12 on A alone; `packed` passes both scales in one register, A's in byte 0
//   (byte select 0) and B's 1.0 in byte 1 (byte select 1), the form k_top2_fp4q2 uses; `unscaled` gives the
//   builtin constant zero scale operands, for which the compiler emits v_mfma_f32_16x16x128_f8f6f4 without
//   block scales, and expects the plain product (both scales 1.0).
// Build: hipcc --offload-arch=gfx950 -O3 mfma_fp4_16_layout.hip -o mfma_fp4_16_layout
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int PACKED>
__global__ void k_one(const int *a, const int *b, const float *c, float *d, int sa, int sb)
{
    const int l = threadIdx.x;
    i32x8 av = {}, bv = {};
    for (int r = 0; r < 4; r++) {
        av[r] = a[l * 4 + r];
        bv[r] = b[l * 4 + r];
    }
    f32x4 cv;
    for (int i = 0; i < 4; i++) cv[i] = c[l * 4 + i];
    if (PACKED == 2) {   // constant zero scale operands: the compiler selects the instruction without block scales
        cv = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, cv, 4, 4, 0, 0, 0, 0);
    } else if (PACKED) {
        const int s = sa | (sb << 8) | (sb << 16);
        cv = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, cv, 4, 4, 0, s, 1, s);
    } else {
        cv = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, cv, 4, 4, 0, sa, 0, sb);
    }
    for (int i = 0; i < 4; i++) d[l * 4 + i] = cv[i];
}

static unsigned code(int v)  // e2m1
{
    switch (v) {
    case 0: return 0x0;
    case 1: return 0x2;
    case -1: return 0xA;
    case 2: return 0x4;
    case -2: return 0xC;
    }
    abort();
}

static int kmap(int hyp, int g, int j)
{
    switch (hyp) {
    case 0: return 32 * g + j;                            // K block g = 32 consecutive k
    case 1: return 16 * g + (j & 15) + 64 * (j >> 4);
    case 2: return 8 * g + (j & 7) + 32 * (j >> 3);
    default: return 4 * g + (j & 3) + 16 * (j >> 2);
    }
}

int main()
{
    srand(7);
    static int A[16][128], B[128][16];
    for (int m = 0; m < 16; m++)
        for (int k = 0; k < 128; k++) A[m][k] = rand() % 5 - 2;
    for (int k = 0; k < 128; k++)
        for (int n = 0; n < 16; n++) B[k][n] = rand() % 5 - 2;
    double ref[16][16];
    for (int m = 0; m < 16; m++)
        for (int n = 0; n < 16; n++) {
            double s = 0;
            for (int k = 0; k < 128; k++) s += A[m][k] * B[k][n];
            ref[m][n] = s;
        }
    int *da, *db;
    float *dc, *dd;
    (void)hipMalloc(&da, 64 * 4 * 4);
    (void)hipMalloc(&db, 64 * 4 * 4);
    (void)hipMalloc(&dc, 64 * 4 * 4);
    (void)hipMalloc(&dd, 64 * 4 * 4);
    std::vector<float> hc(64 * 4);
    for (int l = 0; l < 64; l++)
        for (int i = 0; i < 4; i++) hc[l * 4 + i] = (float)(1000 * (4 * (l >> 4) + i) + (l & 15));
    (void)hipMemcpy(dc, hc.data(), hc.size() * 4, hipMemcpyHostToDevice);
    int unexpected = 0;
    // hb < 0: B packed by the same map as A
    auto trial = [&](const char *name, int ha, int hb, int scaled, int packed, bool transposed, bool must_fail) {
        std::vector<int> pa(64 * 4, 0), pb(64 * 4, 0);
        for (int l = 0; l < 64; l++)
            for (int j = 0; j < 32; j++) {
                const int sh = 4 * (j & 7);
                pa[l * 4 + (j >> 3)] |= (int)(code(A[l & 15][kmap(ha, l >> 4, j)]) << sh);
                pb[l * 4 + (j >> 3)] |= (int)(code(B[kmap(hb < 0 ? ha : hb, l >> 4, j)][l & 15]) << sh);
            }
        (void)hipMemcpy(da, pa.data(), pa.size() * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(db, pb.data(), pb.size() * 4, hipMemcpyHostToDevice);
        if (packed == 2)
            hipLaunchKernelGGL(k_one<2>, dim3(1), dim3(64), 0, 0, da, db, dc, dd, 0, 0);
        else if (packed)
            hipLaunchKernelGGL(k_one<1>, dim3(1), dim3(64), 0, 0, da, db, dc, dd, scaled ? 139 : 127, 127);
        else
            hipLaunchKernelGGL(k_one<0>, dim3(1), dim3(64), 0, 0, da, db, dc, dd, scaled ? 139 : 127, 127);
        std::vector<float> h(64 * 4);
        (void)hipMemcpy(h.data(), dd, h.size() * 4, hipMemcpyDeviceToHost);
        int bad = 0;
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 4; i++) {
                const int n = l & 15, m = 4 * (l >> 4) + i;
                const double want = (transposed ? ref[n][m] : ref[m][n]) * (scaled ? 4096.0 : 1.0) + hc[l * 4 + i];
                if ((double)h[l * 4 + i] != want) bad++;
            }
        const bool ok = must_fail ? bad > 0 : bad == 0;
        if (!ok) unexpected++;
        printf("%s: A map %d, B map %d, scale_a %d, %s scales: %d of 256 outputs differ (%s)\n", name, ha,
               hb < 0 ? ha : hb, scaled ? 139 : 127, packed == 2 ? "no" : packed ? "packed" : "separate", bad,
               ok ? (must_fail ? "differs, as it must" : "exact") : "UNEXPECTED");
    };
    for (int hyp = 0; hyp < 4; hyp++)
        for (int scaled = 0; scaled < 2; scaled++)
            for (int packed = 0; packed < 2; packed++) trial("consistent", hyp, -1, scaled, packed, false, false);
    trial("unscaled", 0, -1, 0, 2, false, false);
    trial("mixed", 0, 1, 1, 1, false, true);
    trial("mixed", 0, 3, 1, 1, false, true);
    trial("transposed", 0, -1, 1, 1, true, true);
    printf("%s\n", unexpected ? "FAILED" : "all as expected");
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dc);
    (void)hipFree(dd);
    return unexpected ? 1 : 0;
}
