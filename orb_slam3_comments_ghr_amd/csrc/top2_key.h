// Key layout and decode of the MFMA top-2 kernels (hamming_mfma.hip); plain C++, also compiled on the host
// (tests/host/top2_key.cpp).
//
// A key is D * 2^13 + rho with D = H - |q| in [-256, 256] (H the Hamming distance, |q| the query's popcount)
// and rho a row index relative to some 32-row tile base.  The FP4 kernels hold it as the bit pattern of a
// float in [2^23, 2^24): bits = key + MX_KEY0.
//
// First key (k1): rebased by -32 after every row tile, so at the end rho = row - base with
// base = 32 * ceil(nt / 32), and key + base = D * 2^13 + row.
//
// Second key (k2) of k_top2_fp4q2: never rebased.  It only ever holds a fresh key (rho in [0, 31]) or a
// former k1 demoted by the median, whose rho is row - 32 * tile >= -32 * 255 (nt <= 8192: tile <= 255), so
// rho is in [-TOP2_K2_OFFSET, 31].  Two such keys of different D keep the order of D, since their rho differ
// by at most 8191 < 2^13; two of equal D decode alike; and (key + TOP2_K2_OFFSET) >> 13 = D exactly,
// however often the value was rebased while it was a k1.  After the last tile k1 has been rebased once more
// (rho >= -8192): a k1 that enters a k2 there takes TOP2_K2_LAST_REBASE back first.
#pragma once

constexpr int MF_SHIFT = 13;                       // key = (H - |q|) << 13 | row
constexpr int MF_MAX_ROWS = 1 << MF_SHIFT;         // rows per problem on this path
constexpr int MX_KEY0 = 0x4B000000 + (1 << 21);    // bit pattern of MX_BIAS (2^23 + 2^21): bits = key + MX_KEY0
constexpr int TOP2_TILE_ROWS = 32;                 // rows per tile = the rebase step of k1
constexpr int TOP2_K2_OFFSET = TOP2_TILE_ROWS * (MF_MAX_ROWS / TOP2_TILE_ROWS - 1);   // 8160
constexpr int TOP2_K2_LAST_REBASE = TOP2_TILE_ROWS;
// k_top2_fp4q2 computes every key 2^-12 times as large (MFMA without block scales, C scaled down to match): a
// float in [2^11, 2^12), whose bit pattern is the one above minus 12 in the exponent field.  The kernel holds
// bits - MX_DOWN_BITS through the row tiles and adds MX_DOWN_BITS back before the merge and the decode below.
constexpr float MX_DOWN = 1.0f / 4096.0f;
constexpr int MX_DOWN_BITS = 12 << 23;

// D * 2^13 + row of a rebased first key (FP4 bit pattern) after the last tile; base = 32 * ceil(nt / 32)
constexpr int top2_k1_value(int bits, int base) { return bits - MX_KEY0 + base; }
constexpr int top2_k1_dist(int bits, int base) { return top2_k1_value(bits, base) >> MF_SHIFT; }
constexpr int top2_k1_row(int bits, int base) { return top2_k1_value(bits, base) & (MF_MAX_ROWS - 1); }
// D of a never-rebased second key (FP4 bit pattern)
constexpr int top2_k2_dist(int bits) { return (bits - MX_KEY0 + TOP2_K2_OFFSET) >> MF_SHIFT; }
