// Host check of csrc/top2_key.h: the decode of a never-rebased second key and of a rebased first key, over
// every D = H - |q| in [-256, 256] and every rho the kernel can hold.  Exit status 0 and "ok" when all hold.
#include <cstdio>

#include "top2_key.h"

static_assert(MF_SHIFT == 13 && MF_MAX_ROWS == 8192, "key layout");
static_assert(TOP2_K2_OFFSET == 8160 && TOP2_K2_LAST_REBASE == 32, "second-key constants");
static_assert(top2_k2_dist(MX_KEY0) == 0 && top2_k2_dist(MX_KEY0 - TOP2_K2_OFFSET) == 0, "constexpr decode");

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

static int bits_of(int D, int rho) { return D * MF_MAX_ROWS + rho + MX_KEY0; }

int main()
{
    const int RHO_MIN = -TOP2_K2_OFFSET, RHO_MAX = TOP2_TILE_ROWS - 1;
    // every (D, rho) decodes to D; the bit pattern stays that of a positive normal float in [2^22, 2^24), whose
    // float order is its integer order (key_push2f takes the median as v_med3_f32; D = -256 with rho < 0 dips
    // below 2^23, where the integer arithmetic on the bits still holds)
    for (int D = -256; D <= 256; D++)
        for (int rho = RHO_MIN; rho <= RHO_MAX; rho++) {
            const int b = bits_of(D, rho);
            CHECK(top2_k2_dist(b) == D, "D %d rho %d -> %d", D, rho, top2_k2_dist(b));
            CHECK(b >= 0x4A800000 && b < 0x4B800000, "D %d rho %d bits %#x", D, rho, b);
        }
    // one step outside the range on either side decodes wrongly: the range is tight, and the + 32 of the final
    // merge is needed for a first key rebased 256 times
    CHECK(top2_k2_dist(bits_of(7, RHO_MIN - 1)) == 6, "below the range");
    CHECK(top2_k2_dist(bits_of(7, RHO_MAX + 1)) == 8, "above the range");
    for (int D = -256; D <= 256; D++)
        for (int row = 0; row < TOP2_TILE_ROWS; row++) {
            const int k1 = bits_of(D, row - MF_MAX_ROWS);   // row of tile 0 after 256 rebases
            CHECK(top2_k2_dist(k1) == D - 1, "unfixed D %d row %d", D, row);
            CHECK(top2_k2_dist(k1 + TOP2_K2_LAST_REBASE) == D, "fixed D %d row %d", D, row);
        }
    // keys of different D order by D for every rho pair at the extremes (adjacent D is the tight case)
    const int ext[4] = {RHO_MIN, RHO_MIN + 1, RHO_MAX - 1, RHO_MAX};
    for (int D = -256; D < 256; D++)
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                CHECK(bits_of(D, ext[i]) < bits_of(D + 1, ext[j]), "order D %d rho %d %d", D, ext[i], ext[j]);
                CHECK(bits_of(-256, ext[i]) < bits_of(D + 1, ext[j]), "order -256 / %d", D + 1);
            }
    // the first key: every row of every tile count, rebased by 32 per tile, decodes to (D, row)
    for (int ntile = 1; ntile <= MF_MAX_ROWS / TOP2_TILE_ROWS; ntile += (ntile < 4 || ntile > 250) ? 1 : 41) {
        const int base = TOP2_TILE_ROWS * ntile;
        for (int D = -256; D <= 256; D += 64)
            for (int row = 0; row < base; row++) {
                const int b = bits_of(D, row - base);
                CHECK(top2_k1_dist(b, base) == D && top2_k1_row(b, base) == row, "k1 D %d row %d base %d", D, row, base);
            }
    }
    // the pad key (rows past nt: the bits of a float near 2^30) and the start sentinel ((256 - |q|) << 13, as a
    // second key and as a first key of any tile count) decode to >= 256 once |q| is added
    const int pad_lo = 0x4E800000 - 1, pad_hi = 0x4E800000 + 1;   // 2^30 -+ one ulp of its neighbourhood
    for (int pc = 0; pc <= 256; pc++) {
        CHECK(top2_k2_dist(pad_lo) + pc >= 256 && top2_k2_dist(pad_hi) + pc >= 256, "pad as k2, |q| %d", pc);
        CHECK(top2_k1_dist(pad_lo - MF_MAX_ROWS, MF_MAX_ROWS) + pc >= 256, "pad as k1, |q| %d", pc);
        const int s = bits_of(256 - pc, 0);
        CHECK(top2_k2_dist(s) + pc == 256, "sentinel as k2, |q| %d", pc);
        for (int base = TOP2_TILE_ROWS; base <= MF_MAX_ROWS; base += TOP2_TILE_ROWS) {
            CHECK(top2_k1_dist(s - base, base) + pc == 256, "sentinel as k1, |q| %d base %d", pc, base);
            // demoted into a second key at any tile but the last rebase, or after it with the + 32
            CHECK(top2_k2_dist(s - base + TOP2_K2_LAST_REBASE) + pc == 256, "sentinel demoted, |q| %d base %d", pc, base);
        }
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
