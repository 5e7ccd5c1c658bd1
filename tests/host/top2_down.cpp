// Host check of MX_DOWN / MX_DOWN_BITS (csrc/top2_key.h): k_top2_fp4q2 computes every key 2^-12 times as large as
// the block-scaled form did.  For every value the accumulator can hold (the bias and row from C, every partial sum
// of the 256 products, the pad of rows past nt, the start key) the float 2^-12 times as large must have the bit
// pattern of the original minus MX_DOWN_BITS, and the sums must stay exact.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstring>

#include "top2_key.h"

static int fails = 0;
#define CHECK(c, ...)                                 \
    do {                                              \
        if (!(c)) {                                   \
            if (fails++ < 20) {                       \
                printf("FAIL %s: ", #c);              \
                printf(__VA_ARGS__);                  \
                printf("\n");                         \
            }                                         \
        }                                             \
    } while (0)

static int bits(float f)
{
    int b;
    memcpy(&b, &f, 4);
    return b;
}
static float from_bits(int b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static_assert(MX_DOWN_BITS == 0x06000000, "12 in the exponent field");

int main()
{
    const float bias = from_bits(MX_KEY0);    // MX_BIAS, 2^23 + 2^21
    const float pad = 1073741824.0f;          // MX_PAD, 2^30
    CHECK(bias == 10485760.0f, "MX_KEY0 is the bit pattern of the bias");
    CHECK(MX_DOWN * 4096.0f == 1.0f, "MX_DOWN");
    volatile float down = MX_DOWN;            // the products below are rounded to float, not folded in double
    for (int row = 0; row < TOP2_TILE_ROWS; row++) {
        // C of a full row tile and of a cut one (the pad swamps the row: both forms round alike)
        const float c = bias + (float)row, cd = c * down;
        CHECK(bits(cd) == bits(c) - MX_DOWN_BITS, "C row %d", row);
        const float cp = c + pad, cpd = cd + pad * down;
        CHECK(bits(cpd) == bits(cp) - MX_DOWN_BITS, "padded C row %d: %#x %#x", row, bits(cpd), bits(cp));
        CHECK(bits(cpd) > bits((bias + 31.0f + 8192.0f * 256.0f) * down), "pad above every key, row %d", row);
        // every partial sum: the scaled form adds multiples of 8192 (2 x 4096 per differing bit pair), this one
        // multiples of 2, in any order; the running value stays C + the sum so far, exactly
        for (int m = -256; m <= 256; m++) {
            const float k = c + 8192.0f * (float)m, kd = cd + 2.0f * (float)m;
            CHECK(bits(kd) == bits(k) - MX_DOWN_BITS, "key row %d m %d", row, m);
            CHECK(bits(k) == m * MF_MAX_ROWS + row + MX_KEY0, "the scaled form's key, row %d m %d", row, m);
            CHECK(kd >= 2048.0f && kd < 4096.0f, "binade, row %d m %d", row, m);
        }
    }
    // the pad accumulator the pipeline opens on
    CHECK(bits(pad * down) == bits(pad) - MX_DOWN_BITS, "pad alone");
    // the start key and the rebases by 32 are integer steps on the bits in both forms; what is held stays the bit
    // pattern of a positive normal float (v_med3_f32 orders it as the integer ops do) down to the lowest value a
    // first key can take: D = -256 rebased 256 times
    const int lowest = -256 * MF_MAX_ROWS - MF_MAX_ROWS + MX_KEY0 - MX_DOWN_BITS;
    CHECK(lowest > 0x00800000 && from_bits(lowest) > 0.0f, "lowest held key %#x", lowest);
    for (int pc = 0; pc <= 256; pc++) {
        const int held = ((256 - pc) << MF_SHIFT) + MX_KEY0 - MX_DOWN_BITS;
        CHECK(top2_k2_dist(held + MX_DOWN_BITS) + pc == 256, "start key, |q| %d", pc);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
