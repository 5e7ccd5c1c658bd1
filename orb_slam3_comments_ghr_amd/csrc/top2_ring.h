// The LDS chunk ring of k_top2_fp4q2 (hamming_mfma.hip): which slot a chunk lives in, which block writes it, and
// in which barrier epoch each write and read falls; plain C++, also compiled on the host
// (tests/host/top2_ring.cpp).
//
// A workgroup walks nch = ceil(nt / CR) chunks of CR train rows.  Chunk c is expanded into slot c % 3.  The
// prologue stores chunks 0 and 1 behind the table's barrier and closes with a second barrier.  Block c (the
// compute of chunk c) opens with one barrier; behind it every thread expands its part of chunk c + 2, which goes
// into the slot that held chunk c - 1 (the last two blocks, whose chunk c + 2 does not exist, write nothing: their
// write epochs stay free).  An epoch is the number of barriers a wave has passed, so block c runs in
// epoch 3 + c.  All waves, whether they own two query tiles, one or none, pass the same 2 + nch barriers.
//
// Reads: a wave with two query tiles runs the row tiles of full chunks as one pipeline that does not stop at a
// chunk's end, so the last row tile of block c prefetches the first fragments of chunk c + 1 from the next slot
// (whether or not that chunk exists or is full: an unused prefetch reads a slot nobody writes in that epoch).
// Chunk 0's first fragments are read behind the prologue's second barrier.  Every other read of chunk c falls in
// block c.
#pragma once

constexpr int TOP2_RING_SLOTS = 3;
constexpr int TOP2_RING_AHEAD = 2;               // block c expands chunk c + 2; the prologue chunks 0 and 1
constexpr int TOP2_RING_PROLOGUE_BARRIERS = 2;   // the byte table; chunks 0 and 1

constexpr int top2_ring_slot(int chunk, int slots = TOP2_RING_SLOTS) { return chunk % slots; }
// the slot after `slot`, without a division (the kernel keeps the slot and steps it once per chunk)
constexpr int top2_ring_next(int slot, int slots = TOP2_RING_SLOTS) { return slot + 1 == slots ? 0 : slot + 1; }

constexpr int top2_ring_chunks(int nt, int cr) { return (nt + cr - 1) / cr; }
constexpr int top2_ring_full_chunks(int nt, int cr) { return nt / cr; }
// barriers every wave of the workgroup executes; depends on nt alone
constexpr int top2_ring_barriers(int nt, int cr) { return TOP2_RING_PROLOGUE_BARRIERS + top2_ring_chunks(nt, cr); }

constexpr int top2_ring_prologue_store_epoch() { return 1; }
constexpr int top2_ring_block_epoch(int c) { return TOP2_RING_PROLOGUE_BARRIERS + 1 + c; }
// the epoch in which chunk `chunk` is written into its slot
constexpr int top2_ring_write_epoch(int chunk)
{
    return chunk < TOP2_RING_AHEAD ? top2_ring_prologue_store_epoch() : top2_ring_block_epoch(chunk - TOP2_RING_AHEAD);
}
// first and last epoch in which a wave with two query tiles reads chunk `chunk` (the first read is the fragment
// prefetch one block earlier; chunk 0's comes behind the prologue's last barrier)
constexpr int top2_ring_first_read_epoch(int chunk)
{
    return chunk == 0 ? TOP2_RING_PROLOGUE_BARRIERS : top2_ring_block_epoch(chunk - 1);
}
constexpr int top2_ring_last_read_epoch(int chunk) { return top2_ring_block_epoch(chunk); }
