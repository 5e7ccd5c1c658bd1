// Host check of csrc/top2_ring.h: the three-slot chunk ring of k_top2_fp4q2, walked by barrier epoch for every
// nt in 1..8192 at the kernel's chunk size.  The walk below transcribes the kernel's control flow for a wave
// with two query tiles, with one, and with none; the header's epoch functions must agree with it, and
//   1. every write to a slot lies in an epoch strictly after the last read of the slot's previous chunk by any wave,
//   2. every read lies in an epoch strictly after the write it needs (an unused prefetch only must not share its
//      epoch with a write to the slot it reads),
//   3. the three kinds of wave pass the same number of barriers, top2_ring_barriers(nt).
// Negative control: the same schedule on a two-slot ring must fail check 1.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <vector>

#include "top2_ring.h"

static_assert(TOP2_RING_SLOTS == 3 && TOP2_RING_AHEAD == 2 && TOP2_RING_PROLOGUE_BARRIERS == 2, "ring constants");
static_assert(top2_ring_slot(4) == 1 && top2_ring_next(2) == 0 && top2_ring_next(0) == 1, "slot arithmetic");
static_assert(top2_ring_chunks(2000, 256) == 8 && top2_ring_full_chunks(2000, 256) == 7, "chunk counts");
static_assert(top2_ring_barriers(2000, 256) == 10, "barriers of the headline shape");
static_assert(top2_ring_write_epoch(0) == 1 && top2_ring_write_epoch(1) == 1 && top2_ring_write_epoch(2) == 3, "writes");
static_assert(top2_ring_first_read_epoch(0) == 2 && top2_ring_first_read_epoch(1) == 3, "first reads");

constexpr int CR = 256, MAX_NT = 8192;
enum Kind { TWO = 0, ONE = 1, IDLE = 2 };

struct Access {
    int epoch, chunk, slot;
    bool write, needed;   // a write of chunk >= nch is the branch-free seam's store of zero rows
};

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

// one wave's LDS accesses to the ring and its barrier count, in program order
static int walk(Kind kind, int nt, int slots, std::vector<Access> &out)
{
    const int nch = top2_ring_chunks(nt, CR), nfc = top2_ring_full_chunks(nt, CR);
    int epoch = 0;
    epoch++;   // barrier: the byte table
    out.push_back({epoch, 0, top2_ring_slot(0, slots), true, true});
    out.push_back({epoch, 1, top2_ring_slot(1, slots), true, 1 < nch});
    epoch++;   // barrier: chunks 0 and 1
    auto seam = [&](int c) {
        epoch++;   // barrier at the top of block c
        out.push_back({epoch, c + TOP2_RING_AHEAD, top2_ring_slot(c + TOP2_RING_AHEAD, slots), true, c + TOP2_RING_AHEAD < nch});
    };
    if (kind == TWO) {
        if (nfc > 0) {
            out.push_back({epoch, 0, top2_ring_slot(0, slots), false, true});   // the first row tile's fragments
            for (int c = 0; c < nfc; c++) {
                seam(c);
                out.push_back({epoch, c, top2_ring_slot(c, slots), false, true});
                // the last row tile's prefetch from the next slot, used only when chunk c + 1 is full too
                out.push_back({epoch, c + 1, top2_ring_slot(c + 1, slots), false, c + 1 < nfc});
            }
        }
    } else {
        for (int c = 0; c < nfc; c++) {
            seam(c);
            if (kind == ONE) out.push_back({epoch, c, top2_ring_slot(c, slots), false, true});
        }
    }
    if (nfc < nch) {
        seam(nfc);
        if (kind != IDLE) out.push_back({epoch, nfc, top2_ring_slot(nfc, slots), false, true});
    }
    return epoch;
}

// -> number of violations of check 1 (a write not strictly after the reads of the slot's earlier chunks)
static int check_ring(int nt, int slots, bool report)
{
    const int nch = top2_ring_chunks(nt, CR);
    std::vector<Access> acc[3];
    int nbar[3];
    for (int k = 0; k < 3; k++) nbar[k] = walk((Kind)k, nt, slots, acc[k]);
    if (report) {
        CHECK(nbar[TWO] == nbar[ONE] && nbar[ONE] == nbar[IDLE], "nt %d barriers %d %d %d", nt, nbar[TWO], nbar[ONE], nbar[IDLE]);
        CHECK(nbar[TWO] == top2_ring_barriers(nt, CR), "nt %d barriers %d header %d", nt, nbar[TWO], top2_ring_barriers(nt, CR));
    }
    int late_writes = 0;
    for (int wk = 0; wk < 3; wk++)
        for (const Access &w : acc[wk]) {
            if (!w.write) continue;
            if (report && w.chunk < nch)
                CHECK(w.epoch == top2_ring_write_epoch(w.chunk), "nt %d chunk %d written in %d, header %d", nt, w.chunk, w.epoch,
                      top2_ring_write_epoch(w.chunk));
            for (int rk = 0; rk < 3; rk++)
                for (const Access &r : acc[rk]) {
                    if (r.write || r.slot != w.slot) continue;
                    if (r.chunk < w.chunk && r.chunk < nch && r.epoch >= w.epoch) {   // check 1
                        late_writes++;
                        if (report) CHECK(false, "nt %d: chunk %d written in epoch %d over chunk %d read in %d", nt, w.chunk, w.epoch, r.chunk, r.epoch);
                    }
                    if (!report) continue;
                    if (r.chunk == w.chunk && r.needed)   // check 2
                        CHECK(w.epoch < r.epoch, "nt %d: chunk %d read in epoch %d, written in %d", nt, r.chunk, r.epoch, w.epoch);
                    if (!r.needed) CHECK(w.epoch != r.epoch, "nt %d: unused prefetch and a write share epoch %d", nt, r.epoch);
                }
        }
    if (report)
        for (const Access &r : acc[TWO]) {
            if (r.write || !r.needed) continue;
            CHECK(r.epoch >= top2_ring_first_read_epoch(r.chunk) && r.epoch <= top2_ring_last_read_epoch(r.chunk),
                  "nt %d chunk %d read in %d outside the header's %d..%d", nt, r.chunk, r.epoch, top2_ring_first_read_epoch(r.chunk),
                  top2_ring_last_read_epoch(r.chunk));
        }
    return late_writes;
}

int main()
{
    // the kernel steps the slots without a division: the same sequence as top2_ring_slot
    for (int c = 0, slot = top2_ring_slot(0), freed = top2_ring_slot(TOP2_RING_SLOTS - 1); c < MAX_NT / CR + 2; c++) {
        CHECK(slot == top2_ring_slot(c), "slot of chunk %d", c);
        CHECK(freed == top2_ring_slot(c + TOP2_RING_AHEAD), "block %d writes slot %d", c, freed);
        freed = slot;
        slot = top2_ring_next(slot);
    }
    for (int nt = 1; nt <= MAX_NT; nt++) CHECK(check_ring(nt, TOP2_RING_SLOTS, true) == 0, "nt %d", nt);
    // negative control: two slots under the same schedule: block c stores chunk c + 2 (or, past the last chunk, zero
    // rows) into the slot that chunk c is being read from, at every nt
    for (int nt = 1; nt <= MAX_NT; nt++) CHECK(check_ring(nt, 2, false) > 0, "two slots pass check 1 at nt %d", nt);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
