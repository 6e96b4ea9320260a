// The aligner host's plan (aligner_plan.hpp): arithmetic only, no device.
#include "aligner_plan.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace gwamd
{
namespace aln
{
namespace
{
int64_t a16(int64_t v) { return (v + 15) & ~int64_t(15); }
} // namespace

AlignerLimits aligner_limits(int algo)
{
    switch (algo)
    {
    case kAlgoHm:
        // long mode (hm_kernel<true>): query patterns in HBM, striped sweeps;
        // the target's 2-bit letter codes stay in LDS up to kHmLdsTarget
        return {kHmMaxQuery, kHmMaxTarget};
    case kAlgoMyers:
        // stripes of 8,192 rows; the (word, column) state of the largest pair
        // must fit one workspace slot (kMyersMaxSlot)
        return {kHmMaxQuery, kHmMaxTarget};
    case kAlgoBanded:
        // patterns (Q / 2 bytes) and target codes (T / 4 bytes) in LDS
        return {65536, 65536};
    default:
        // Ukkonen: both sequences in LDS (ukkonen_wide_kernel: up to 2 x 64 KiB
        // of its 160 KiB), (1 + int(0.1f * T) + 2p + 1) / 2 = 3,377 band rows
        // at 65,536, within kUkWideChunks x 1,024; the reference benchmark's
        // largest size (cudaaligner/benchmarks/main.cpp:140-143)
        return {65536, 65536};
    }
}

// Workspace slot of the full Myers aligner (always long mode): the padded
// (word, column) matrix of pv / mv / score (128-B rows), the stripes'
// per-column deltas, the query patterns and, past kHmLdsTarget, the target
// letter codes; slots start on 256-B lines.
int64_t myers_slot_layout(int32_t max_q, int32_t max_t, int64_t* hbuf_off, int64_t* pat_off, int64_t* tcod_off)
{
    const int64_t pw    = (int64_t(max_q) + kWordBits - 1) / kWordBits;
    const int64_t nwp   = (pw + 31) & ~int64_t(31);
    const bool tcod_hbm = max_t > kHmLdsTarget;
    const int64_t hb    = a16(nwp * (int64_t(max_t) + 1) * 12 + 64);
    const int64_t po    = a16(hb + int64_t(max_t) + 1 + kWave + 64);
    const int64_t to    = a16(po + pw * 32 + 64);
    const int64_t slot  = a16(to + (tcod_hbm ? (int64_t(max_t) + 15) / 16 * 4 + 64 : 0));
    if (hbuf_off)
        *hbuf_off = hb, *pat_off = po, *tcod_off = to;
    return (slot + 255) & ~int64_t(255);
}

// Limits of this implementation (the reference has none): the Myers state of a
// query segment is register-resident (4 blocks of 64x32 bits), the banded
// aligners keep both sequences in LDS, the Ukkonen band has at most
// kUkWideChunks x 1,024 rows, a full Myers pair fits one workspace slot.
std::string aligner_limit_error(int algo, int32_t max_q, int32_t max_t)
{
    const AlignerLimits lim = aligner_limits(algo);
    if (max_q > lim.max_query)
        return "max_query_length above " + std::to_string(lim.max_query) + " is not supported by this aligner.";
    if (algo == kAlgoUkkonen && ukkonen_band_rows(ukkonen_max_difference(max_t)) > kUkWideChunks * 1024)
        return "max_target_length too large for the Ukkonen aligner's band.";
    if (max_t > lim.max_target)
        return "max_target_length above " + std::to_string(lim.max_target) + " is not supported by this aligner.";
    if (algo == kAlgoMyers)
    {
        const int64_t slot = myers_slot_layout(max_q, max_t, nullptr, nullptr, nullptr);
        if (slot > kMyersMaxSlot)
            return "max_query_length x max_target_length too large for the full Myers aligner's score matrix (" +
                   std::to_string(slot) + " bytes)";
    }
    return std::string();
}

namespace
{

// Banded Myers: target as 2-bit letter codes, letter-major query patterns, and
// a chunk-state / backtrace tile.
void layout_banded(AlignerPlan& p, int32_t max_q, int32_t max_t, const AlignerTuning& tuning)
{
    Args& a           = p.args;
    a.lds_target_off  = 0;
    a.lds_pat_off     = int32_t(a16((max_t + 15) / 16 * 4 + 16));
    a.lds_tile_off    = int32_t(a.lds_pat_off + a16(int64_t(a.pat_words) * 16 + 16));
    // at least 128 16-byte band entries (two columns of 64 words, or 128 chunk
    // words: a smaller LDS image keeps more short pairs resident, D_banded
    // 372.8k -> 451.7k alignments/s with 2 KiB against 4 KiB); up to the whole
    // band's chunk state while the workgroup's LDS stays within the CU's
    // 160 KiB (a 65,536 bp query: 16 KiB target + 32 KiB patterns + 32 KiB
    // state; wider bands keep the state in HBM and wait on it every column)
    a.tile_bytes      = 2048;
    int64_t want      = a16(int64_t(a.pat_words) * 16);
    want              = std::min<int64_t>(want, (kLdsPerCu - 512 - a.lds_tile_off) & ~int64_t(511)); // static LDS
    if (tuning.band_tile_bytes.set) // parity tests: HBM chunk state
    {
        // 2048 (128 words) up to 48 KiB, in whole 512-byte steps; anything
        // else is a typo that would silently keep the default plan
        long v = 0;
        if (!tuning.band_tile_bytes.number_in(2048, 48 << 10, v) || v % 512 != 0)
            throw std::invalid_argument("GWAMD_BAND_TILE_BYTES must be 2048..49152 in steps of 512");
        a.tile_bytes = int32_t(v);
        want         = v;
    }
    if (want > a.tile_bytes)
        a.tile_bytes = int32_t(want);
    // long queries (bands of many 32-word chunks) run 8 waves per pair, 16
    // target columns in flight; short ones keep one wave per pair and their
    // occupancy
    a.band_waves = max_q > kLongBandQuery ? 8 : 1;
    if (tuning.band_waves.set)
    {
        long v = 0;
        if (!tuning.band_waves.number_in(1, 16, v) || (v != 1 && v != 4 && v != 8 && v != 16))
            throw std::invalid_argument("GWAMD_BAND_WAVES must be 1, 4, 8 or 16");
        a.band_waves        = int32_t(v);
        p.band_waves_forced = true;
    }
    if (tuning.band_spec.set)
    {
        long v = 0;
        if (!tuning.band_spec.number_in(0, kMaxSpecSweeps, v))
            throw std::invalid_argument("GWAMD_BAND_SPEC must be 0..8 sweeps");
        p.spec_forced = int32_t(v);
    }
    a.lds_bytes  = a.lds_tile_off + a.tile_bytes;
    // band entries (pv, mv, score, pad) of the widest band (the whole query)
    p.slot_bytes = a16(int64_t(a.pat_words) * (max_t + 1) * 16 + 64);
}

// Ukkonen.  The band of a pair is (1 + |n - m| + 2p + 1) / 2 rows; the
// workspace is sized for the largest allowed difference, but each launch runs
// the single-wave kernel (ukkonen_kernel, up to kUkChunks * 64 rows) when every
// pair of the batch fits it, and the workgroup kernel (ukkonen_wide_kernel, up
// to 1,024 threads of kUkWideChunks rows, as calc_good_blockdim,
// ukkonen_gpu.cu:268-273) otherwise.  Both keep the sequences in LDS; the wide
// kernel's backtrace tile reuses them.
void layout_ukkonen(AlignerPlan& p, int32_t max_q, int32_t max_t, const AlignerTuning& tuning)
{
    Args& a            = p.args;
    const int rows     = ukkonen_band_rows(ukkonen_max_difference(max_t));
    a.lds_target_off   = 0;
    a.lds_seq2_off     = int32_t(a16(a.stride + 16));
    const int64_t seqs = a.lds_seq2_off + a16(a.stride + 16);
    // ukkonen_kernel's backtrace tile (the narrow kernel's only use of it; any
    // size is correct, reads outside it go to HBM).  Pairs up to 8 kb: 5 KiB,
    // 10 workgroups per CU at 5 kb (8 KiB: 8; measured 653-658k against 611k
    // alignments/s on D_ukkonen); up to 32 kb: 8 KiB, which keeps the window
    // walk for bands up to 255 rows; pairs of 32 kb and more (few per batch,
    // one workgroup per CU already) take what the CU's LDS has left, up to
    // 48 KiB, so the walk refills every ~100 columns instead of every ~22 (one
    // HBM latency each)
    int32_t uk_tile    = a.stride <= 8192 ? 5120 : 8192;
    if (a.stride >= 32768)
        uk_tile = int32_t(std::max<int64_t>(8192, std::min<int64_t>(49152, (kLdsPerCu - 64 - seqs) & ~int64_t(511))));
    if (tuning.uk_tile_bytes.set)
    {
        long v = 0;
        if (!tuning.uk_tile_bytes.number_in(1024, 65536, v) || v % 512 != 0)
            throw std::invalid_argument("GWAMD_UK_TILE_BYTES must be 1024..65536 in steps of 512");
        uk_tile = int32_t(v);
    }
    a.lds_tile_off = int32_t(seqs);
    a.tile_bytes   = uk_tile;
    a.lds_bytes    = int32_t(seqs + uk_tile);
    a.lds_edge_off = int32_t(std::max<int64_t>(seqs, kUkTileRows * kUkTileCols * 2));
    p.uk_wide_lds  = a.lds_edge_off + 4 * kUkWideChunks * 16 * 4;
    p.uk_wide      = rows > kUkChunks * kWave; // batches with wide bands run one workgroup per pair
    p.slot_bytes   = a16(int64_t(rows) * (int64_t(max_q) + max_t + 2) * 2 + 64);
}

// Hirschberg-Myers and full Myers.  Long mode: patterns in HBM, target codes
// through a generic pointer.  Full Myers always: its patterns are read only
// when a stripe starts, and with them in HBM a wave needs ~4 KiB of LDS instead
// of ~10 KiB, so the occupancy query allows twice the waves (config D_myers:
// 353 -> 241 ms per 100k pairs).
void layout_full(AlignerPlan& p, int32_t max_q, int32_t max_t, const AlignerTuning& tuning)
{
    Args& a       = p.args;
    const bool hm = p.algo == kAlgoHm;
    bool long_mode = hm ? (max_q > kHmShortQuery || max_t > kHmShortTarget) : true;
    // GWAMD_HM_STRIPE_BLOCKS=1..4 (parity tests): long mode at any size, with
    // stripes of that many blocks, so short pairs take the striped sweeps
    long sb = 0;
    if (hm && tuning.hm_stripe_blocks.number_in(1, kMaxChunks, sb))
    {
        a.stripe_blocks = int32_t(sb);
        long_mode       = true;
    }
    a.long_mode        = long_mode ? 1 : 0;
    const int sc_bytes = long_mode ? 4 : 2; // split scores
    a.lds_target_off   = 0;
    // target as 2-bit letter codes (long mode: in HBM past kHmLdsTarget)
    const bool tcod_hbm = long_mode && max_t > kHmLdsTarget;
    a.lds_pat_off       = int32_t(tcod_hbm ? 0 : a16((max_t + 15) / 16 * 4 + 16));
    // long mode: the patterns live in the HBM slot
    a.lds_scratch_off   = int32_t(a.lds_pat_off + (long_mode ? 0 : a16(int64_t(a.pat_words) * 32 + 16)));
    if (hm) // LDS split scores of segments up to kSplitLds columns
        a.scratch_bytes = int32_t(a16(int64_t(2) * kSplitLds * sc_bytes));
    else // full Myers: the backtrace tile (kTbW words x 64 columns of pv, mv, score)
        a.scratch_bytes = 4 * 64 * 12;
    a.lds_stack_off = a.lds_scratch_off + a.scratch_bytes;
    a.lds_bytes     = a.lds_stack_off + (hm ? kStackSize * 16 : 0);
    int64_t tcod_off = 0;
    if (hm)
    {
        // slot: split scores of wide segments (forward, reverse), the
        // breadth-first frontier (two buffers of (qb, qe, tb, te) + one split
        // column per entry; at most 2 * (query + 1) segments: every leaf has a
        // query row or is one of the target-only halves of a split), per-lane
        // base cases (columns of every segment: target + one per segment;
        // (offset, length) per segment; paths), and in long mode the query
        // patterns and the striped sweeps' deltas
        a.ws_split_off    = 0;
        a.front_cap       = 2 * (max_q + 2);
        a.ws_front_off    = a16(int64_t(2) * (a.stride + 1 + kWave) * sc_bytes + 64);
        a.leaf_cols       = max_t + a.front_cap + 2;
        a.ws_leaf_off     = a16(a.ws_front_off + int64_t(a.front_cap) * (2 * 16 + 4) + 64);
        const int64_t end = a16(a.ws_leaf_off + int64_t(a.leaf_cols) * kLeafColBytes + 16 +
                                int64_t(a.front_cap) * 8 + max_q + max_t + 64);
        a.ws_pat_off  = end;
        a.ws_hbuf_off = a16(a.ws_pat_off + (long_mode ? int64_t(a.pat_words) * 32 + 64 : 0));
        tcod_off      = a16(a.ws_hbuf_off + (long_mode ? int64_t(max_t) + 1 + kWave + 64 : 0));
        p.slot_bytes  = a16(tcod_off + (tcod_hbm ? int64_t(max_t + 15) / 16 * 4 + 64 : 0));
    }
    else
        // full matrix: pv, mv, score per (word, column), then the stripes'
        // per-column deltas, the patterns and the target codes
        p.slot_bytes = myers_slot_layout(max_q, max_t, &a.ws_hbuf_off, &a.ws_pat_off, &tcod_off);
    a.ws_tcod_off = tcod_hbm ? tcod_off : -1;
}

} // namespace

AlignerPlan plan_layout(int algo, int32_t max_q, int32_t max_t, int32_t max_n, const AlignerTuning& tuning)
{
    const std::string refused = aligner_limit_error(algo, max_q, max_t);
    if (!refused.empty())
        throw std::invalid_argument(refused);
    AlignerPlan p;
    p.algo             = algo;
    Args& a            = p.args;
    a.stride           = std::max(max_q, max_t);
    a.max_path_length  = (max_q + max_t + 3) / 4 * 4; // calc_max_result_length (aligner_global.cpp:26-31)
    a.max_query_length = max_q;
    a.max_matrix_elems = int64_t((max_q + 3) / 4) * (kFullMyers + 1);
    a.pat_words        = (max_q + kWordBits - 1) / kWordBits;
    a.stripe_blocks    = kMaxChunks;
    a.ws_tcod_off      = -1;
    a.ukkonen_p        = kUkkonenP;
    a.band_waves       = 1;
    const bool banded  = algo == kAlgoBanded || algo == kAlgoUkkonen;
    if (algo == kAlgoBanded)
        layout_banded(p, max_q, max_t, tuning);
    else if (algo == kAlgoUkkonen)
        layout_ukkonen(p, max_q, max_t, tuning);
    else
        layout_full(p, max_q, max_t, tuning);
    if (a.lds_bytes > (banded ? kLdsPerCu : 65536) || p.uk_wide_lds > kLdsPerCu)
        throw std::invalid_argument("aligner problem size does not fit in LDS");
    a.ws_slot_bytes = p.slot_bytes;
    p.fixed_bytes   = int64_t(2) * a.stride * max_n + 16 + int64_t(2) * max_n * 4 +
                    int64_t(a.max_path_length) * max_n + 16 + int64_t(max_n) * 4 + 32 +
                    (algo == kAlgoBanded ? int64_t(max_n) * kMaxSpecSweeps * 4 : 0);
    p.occupancy_key = {algo, a.long_mode, a.band_waves, 0};
    return p;
}

SlotPlan plan_slots(const AlignerPlan& plan, const DeviceFacts& facts, int32_t max_n, const AlignerTuning& tuning)
{
    SlotPlan sp;
    const int per_cu = plan.uk_wide ? std::max(facts.per_cu, facts.wide_per_cu) : facts.per_cu;
    int64_t slots    = std::max(1, per_cu * facts.cus);
    int64_t ws_cap   = plan.algo == kAlgoHm ? kHmWorkspace : kMyersWorkspace;
    if (plan.algo == kAlgoBanded || plan.algo == kAlgoUkkonen)
    {
        sp.resident = int32_t(slots);
        sp.cus      = facts.cus;
        // resident workspace slots within 64 GiB of the 288 GB HBM; only a
        // batch whose slots need more (32 pairs of 65,536 bp: 32 band-matrix
        // slots of 2.15 GB, and one slot fewer than pairs doubles the kernel)
        // may take up to 96 GiB, and at most 3/4 of the free memory, so short-
        // pair aligners keep a plan that does not depend on what else the
        // process has allocated
        const int64_t want_ws = std::min<int64_t>(slots, max_n) * plan.slot_bytes;
        if (want_ws > ws_cap)
            ws_cap = std::max<int64_t>(ws_cap, std::min<int64_t>({int64_t(96) << 30, want_ws,
                                                                  int64_t(uint64_t(facts.free_bytes) / 4 * 3)}));
    }
    slots = std::max<int64_t>(1, std::min<int64_t>(slots, ws_cap / plan.slot_bytes));
    // GWAMD_ALIGNER_GRID (diagnostic): slots per CU instead of what is resident
    if (tuning.grid.set && !tuning.grid.text.empty())
    {
        long per = 0;
        if (!tuning.grid.number_in(1, 32, per))
            throw std::invalid_argument("GWAMD_ALIGNER_GRID must be 1..32 workgroups per CU");
        slots = per * facts.cus;
    }
    sp.slots = int32_t(std::min<int64_t>(slots, max_n));
    return sp;
}

LaunchPlan plan_launch(const AlignerPlan& plan, const SlotPlan& sp, int32_t count, int32_t nslots,
                       int32_t max_query_in_range, int32_t max_diff)
{
    const Args& a = plan.args;
    LaunchPlan l;
    l.uk_threads   = 0;
    l.lds_bytes    = a.lds_bytes;
    l.lds_tile_off = a.lds_tile_off;
    l.tile_bytes   = a.tile_bytes;
    l.band_waves   = a.band_waves;
    if (plan.algo == kAlgoUkkonen)
    {
        // the widest band of this batch decides the Ukkonen kernel
        const int rows = ukkonen_band_rows(max_diff);
        if (rows > kUkChunks * kWave)
        {
            l.uk_threads   = std::min(1024, (rows + kWave - 1) / kWave * kWave);
            l.lds_bytes    = plan.uk_wide_lds;
            l.lds_tile_off = 0;
            l.tile_bytes   = kUkTileRows * kUkTileCols * 2;
        }
    }
    // an aligner planned for long queries (8 waves per pair) runs a launch
    // whose queries are all short with one wave per pair: the one-wave kernel
    // is the default plan for such queries (short bands leave most of 8 waves
    // idle, and one wave per pair keeps more pairs resident)
    if (launch_needs_max_query(plan) && max_query_in_range <= kLongBandQuery)
        l.band_waves = 1;
    // banded Myers: sweeps of the band doubling run ahead on their own
    // workgroups when a launch's pairs leave most of the GPU idle (few long
    // pairs: every pair on its own slot, all (pair, sweep) items resident) and
    // every band's chunk state fits LDS; GWAMD_BAND_SPEC forces their number
    if (plan.algo == kAlgoBanded && count > 0)
    {
        const int k     = plan.spec_forced >= 0 ? plan.spec_forced : l.band_waves > 1 ? kDefaultSpecSweeps : 0;
        const bool fits = count <= nslots && int64_t(count) * k <= sp.resident && 2 * count <= sp.cus &&
                          a.pat_words <= a.tile_bytes / 16;
        l.spec_sweeps = fits ? k : 0;
    }
    l.key = {plan.algo, a.long_mode, l.band_waves, l.uk_threads};
    if (l.spec_sweeps > 0)
    {
        // every (pair, sweep) on its own workgroup, then one workgroup per pair on its own slot
        l.grid[0] = std::min(count * l.spec_sweeps, sp.resident);
        l.grid[1] = count;
    }
    else
        l.grid[0] = std::min(count, nslots);
    return l;
}

int pipeline_stages(int32_t slots, int32_t n, const AlignerTuning& tuning)
{
    if (tuning.pipeline.set) // forces k stages (diagnostic)
    {
        long k = 0;
        if (!tuning.pipeline.number_in(0, kMaxStages, k))
            throw std::invalid_argument("GWAMD_ALIGNER_PIPELINE must be 0..8 stages");
        return slots < 2 ? 1 : std::max(1, std::min(int(k), n));
    }
    if (slots < 2)
        return 1;
    const int64_t per = int64_t(4) * (slots / 2); // pairs per stage
    // (config D, 100k pairs on 3,328 slots: 1 / 2 / 4 / 8 stages measured
    // 365 / 348 / 320 / 309 ms per step)
    return int(std::max<int64_t>(1, std::min<int64_t>(kMaxStages, n / per)));
}

} // namespace aln
} // namespace gwamd
