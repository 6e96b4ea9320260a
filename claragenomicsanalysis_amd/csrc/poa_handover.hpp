// Block hand-over of row carries between neighbouring waves of the 16-bit LDS
// forward pass (fwd2_rows, poa_fwd2.hpp): slot, threshold and flush arithmetic.
// Plain constexpr functions of ints, so the same text runs in the kernel and in
// the host model that steps a producer against a consumer
// (tests/handover_model.cpp).
//
// Rows are 1 .. V.  Row r lives in slot r & 63 of a channel of kHandSlots
// words, and in lane r & 63 of the register either side keeps.  A block is the
// B rows that share r / B (B divides 64; the first block is rows 1 .. B-1).
//
//   producer, row r:  [r opens a block and r >= 64: wait tail >= hand_free_tail]
//                     reg[r & 63] = carry of row r
//                     [r closes a block or r == V: store the block's lanes to
//                      their slots, then head = r]
//   consumer, row r:  [r opens a block: wait head >= hand_need_head, load the
//                      slots, merge the block's lanes, then tail = that row]
//                     carry of row r = reg[r & 63]
//
// head: rows posted so far.  tail: rows taken so far.  Both start at 0, only
// grow, and each has one writer.
//
// Why no wait is for ever (V >= 1, producer and consumer run the same V; a
// wave whose span is empty, or V < 1, enters neither role, and its neighbour
// is then no producer or consumer of it either: `feed` of wave q and the
// activity of wave q+1 are the same predicate cb + span < L):
//  * the consumer waits at block [s, e] for head >= min(e, V).  The producer
//    posts head = min(e, V) when it finishes that row: the block's last row, or
//    row V, where a partial last block (V not a multiple of B, V < B) is
//    flushed.  Before that row it can only wait for tail >= s' - 64 + B - 1
//    with s' <= s, the end of a block at least 64 - B rows older;
//  * the producer waits at block start s >= 64 for tail >= s - 64 + B - 1
//    = e - 64.  That row is a block end below s <= V, head >= s - 1 >= e - 64
//    was posted with the previous block, so the consumer's wait for it has
//    ended or will, and it publishes tail = e - 64 right after;
//  * so each wait is for a block strictly older than the waiter's own, and
//    the oldest block is waited for by nobody: by induction every wait ends;
//  * a restart (next read, next sweep) zeroes head, tail and the slots between
//    two barriers, after every wave has left the row loop.
//
// The row loop is written block by block: an outer loop whose step is one
// block [s, min(e, V)] (hand_block_last), with the consumer's wait, load and
// tail store and the producer's flow-control wait before the block's first
// row, and the producer's slot and head stores after its last; the rows inside
// test for none of these.  This is the same sequence of waits and stores, at
// the same rows, as the per-row tests hand_opens / hand_closes gave (the loop
// starts at row 1, every later block at a multiple of B, and a block ends at
// its last row or at V), so the argument above holds unchanged: no wait was
// added, moved before a store it used to follow, or given a larger threshold.
//
// The wave that ends a sweep keeps its carries for the next sweep in HBM.  It
// fills the same register as a producer and stores the block's lanes to
// carry[row] after the block's last row, rows 1 .. V only.  Nobody waits for
// these stores in the row loop: the next sweep starts behind two barriers, and
// its wave 0 then loads them block by block (hand_lane_row).
#pragma once

namespace gwamd
{
namespace poa
{

constexpr int kHandSlots = 64; // channel depth in rows (kChanRows); lanes of the register

constexpr bool hand_block_ok(int B) { return B >= 1 && B <= kHandSlots && kHandSlots % B == 0; }

// slot of row r in the channel, lane of row r in the register
constexpr int hand_slot(int r) { return r & (kHandSlots - 1); }
// first slot / lane of row r's block; the block is slots [first, first + B)
constexpr int hand_block_slot(int r, int B) { return hand_slot(r) & ~(B - 1); }
constexpr bool hand_lane_in_block(int lane, int r, int B) { return (lane & ~(B - 1)) == hand_block_slot(r, B); }
// row whose carry lane `lane` holds once the block of row r is in the register
constexpr int hand_lane_row(int lane, int r) { return (r & ~(kHandSlots - 1)) + lane; }

// row r opens a block (the first block opens at row 1)
constexpr bool hand_opens(int r, int B) { return (r & (B - 1)) == 0 || r == 1; }
// row r closes a block: the block's last row, or row V (flush of a partial block)
constexpr bool hand_closes(int r, int V, int B) { return (r & (B - 1)) == B - 1 || r == V; }
// last row of row r's block that exists
constexpr int hand_block_last(int r, int V, int B) { return (r | (B - 1)) < V ? (r | (B - 1)) : V; }

// consumer, at a row that opens a block: head it needs before it loads the slots
constexpr int hand_need_head(int r, int V, int B) { return hand_block_last(r, V, B); }
// ... and the tail it publishes after the load
constexpr int hand_new_tail(int r, int V, int B) { return hand_block_last(r, V, B); }
// producer, at a row that opens a block: does it overwrite slots of older rows,
// and the tail that shows they have been taken
constexpr bool hand_must_wait(int r) { return r >= kHandSlots; }
constexpr int hand_free_tail(int r, int B) { return (r | (B - 1)) - kHandSlots; }

} // namespace poa
} // namespace gwamd
