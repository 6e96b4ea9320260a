// cudapolish: aligned overlaps cut into target windows from their CIGAR runs
// (the records of polish_windows.hip on the expanded state path; semantics in
// include/gwamd_polish.h).  The ops are in this project's convention and in
// path order (the host normalises a SAM CIGAR in one pass over its ops): M, =
// and X advance both sequences, I only the target, D only the query.
//
// One wave owns one overlap from its first op to its last: no workgroup
// barrier, no LDS.  The ops are walked in tiles of 64, a lane one op (a 4-byte
// load, so an overlap's ops may begin at any word of the packed array).  Per tile
//   - an inclusive wave scan of the lanes' (target, query) advances, each sum
//     saturating at 2^31, plus the saturating carry of the earlier tiles gives
//     the lane the offsets before its op.  Spans are below 2^31, so a
//     saturated sum never passes for an offset inside the overlap and a path
//     whose advances pass 2^32 cannot wrap into a fit;
//   - a match run (M, =, X of length > 0) is checked against the two spans
//     before anything is formed from it.  One that fits has its first state
//     (q, t, k = t / w) and its last; an overlap with one that does not is a
//     misfit and the run stores nothing, so ops of any value never yield a
//     record or a position outside the overlap's own range;
//   - every window boundary inside the run closes window k with the last
//     state before the boundary and opens the next window with the state
//     after it, q from the run's diagonal.  A run with at most
//     kCigarOwnCrossings boundaries is walked by its lane; a longer one is
//     named by a ballot, broadcast, and its boundaries lane, lane + 64, ...
//     are taken by the whole wave;
//   - the first state of a lane's run meets the last state of the nearest
//     match run before it (a ballot names the lane, three shuffles fetch k, q,
//     t; or the carry of the earlier tiles) as the states of
//     polish_windows.hip meet: where the windows differ, the earlier one is
//     closed and the later one opened.  Lane 0 closes the last run of the
//     overlap at the end.
// Every word of a record has one writer, plain vector stores, the result does
// not depend on timing.
#include "polish_cut.hpp"

namespace gwamd
{
namespace polish
{
namespace
{

constexpr uint32_t kThreads = kCutWaves * 64;
constexpr uint32_t kSumCap  = uint32_t(1) << 31; // above every span
static_assert(kCigarTileOps == 64, "one op per lane");

struct CigarArgs
{
    const uint32_t* ops;
    int64_t num_ops;
    const int64_t* offsets;
    const uint32_t* overlaps;
    const uint32_t* record_base;
    uint32_t* records;
    uint32_t* status;
    uint32_t n;
    uint32_t window_length;
    WindowDivisor w;
};

// min(a + b, 2^31) for a, b <= 2^31
__device__ inline uint32_t add_capped(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return (s < a || s > kSumCap) ? kSumCap : s;
}

// Boundary j of a match run whose first state is `first`: the state before
// it closes window first.k +- j, the one after it opens the next.  The caller
// has checked that the run crosses more than j boundaries inside the overlap.
__device__ inline void store_crossing(uint32_t* record0, uint32_t k0, const Mark& first, uint32_t j, uint32_t w,
                                      bool reverse)
{
    Mark close, open;
    if (reverse)
    {
        close.k = first.k - j;
        close.t = close.k * w;
        close.q = first.q + (first.t - close.t);
        open.k  = close.k - 1;
        open.t  = close.t - 1;
    }
    else
    {
        close.k = first.k + j;
        close.t = (close.k + 1) * w - 1;
        close.q = first.q + (close.t - first.t);
        open.k  = close.k + 1;
        open.t  = close.t + 1;
    }
    open.q = close.q + 1;
    store_mark(record0, k0, close, false, reverse);
    store_mark(record0, k0, open, true, reverse);
}

__global__ __launch_bounds__(kThreads) void window_segments_cigar_kernel(const CigarArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t o    = blockIdx.x * kCutWaves + (threadIdx.x >> 6);
    if (o >= a.n)
        return;
    const uint32_t* overlap = a.overlaps + size_t(o) * kOverlapWords;
    const uint32_t qs       = uniform(overlap[2]);
    const uint32_t ts       = uniform(overlap[3]);
    const uint32_t qe       = uniform(overlap[4]);
    const uint32_t te       = uniform(overlap[5]);
    const bool reverse      = (uniform(overlap[6]) & 0xff) == '-';
    const uint32_t span_t = te - ts, span_q = qe - qs; // the host has checked start <= end < 2^31
    const uint32_t k0     = window_of(ts, a.w);
    uint32_t* record0     = a.records + size_t(uniform(a.record_base[o])) * kRecordWords;

    // the overlap's ops: [begin, end) of the array, cut to the array
    int64_t begin = uniform(a.offsets[o]);
    int64_t end   = uniform(a.offsets[o + 1]);
    bool bad      = false;
    if (begin < 0 || begin > a.num_ops || end < begin)
    {
        bad   = true;
        begin = end = 0;
    }
    else if (end > a.num_ops)
    {
        bad = true;
        end = a.num_ops;
    }

    uint32_t done_t = 0, done_q = 0; // capped target and query advances of the tiles walked
    bool have_last  = false;         // the last match state of the tiles walked (the same on every lane)
    Mark last{0, 0, 0};

    uint32_t next = begin + lane < end ? a.ops[begin + lane] : 0;
    for (int64_t tile = begin; tile < end; tile += kCigarTileOps)
    {
        const bool have_op = tile + lane < end;
        const uint32_t op  = next;
        next               = tile + kCigarTileOps + lane < end ? a.ops[tile + kCigarTileOps + lane] : 0;
        const uint32_t code = op & 15, length = op >> 4;
        const bool match    = code == 0 || code == 7 || code == 8;
        if (have_op && !match && code != 1 && code != 2)
            bad = true;
        const uint32_t adv_t = have_op && (match || code == 1) ? length : 0;
        const uint32_t adv_q = have_op && (match || code == 2) ? length : 0;
        uint32_t scan_t = adv_t, scan_q = adv_q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t below_t = uint32_t(__shfl_up(int(scan_t), d, 64));
            const uint32_t below_q = uint32_t(__shfl_up(int(scan_q), d, 64));
            if (lane >= uint32_t(d))
            {
                scan_t = add_capped(scan_t, below_t);
                scan_q = add_capped(scan_q, below_q);
            }
        }
        const uint32_t tile_t = uniform(uint32_t(__shfl(int(scan_t), 63, 64)));
        const uint32_t tile_q = uniform(uint32_t(__shfl(int(scan_q), 63, 64)));
        uint32_t before_t     = uint32_t(__shfl_up(int(scan_t), 1, 64));
        uint32_t before_q     = uint32_t(__shfl_up(int(scan_q), 1, 64));
        if (lane == 0)
            before_t = before_q = 0;
        const uint32_t at_t = add_capped(done_t, before_t);
        const uint32_t at_q = add_capped(done_q, before_q);

        // the lane's match run: its first and last state, and the boundaries between them
        bool have_mine = false;
        Mark mine_first{0, 0, 0}, mine{0, 0, 0};
        uint32_t crossings = 0;
        if (have_op && match && length > 0)
        {
            if (at_t <= span_t && length <= span_t - at_t && at_q <= span_q && length <= span_q - at_q)
            {
                mine_first.t = reverse ? te - 1 - at_t : ts + at_t;
                mine_first.q = qs + at_q;
                mine_first.k = window_of(mine_first.t, a.w);
                mine.t       = reverse ? mine_first.t - (length - 1) : mine_first.t + (length - 1);
                mine.q       = mine_first.q + (length - 1);
                mine.k       = window_of(mine.t, a.w);
                crossings    = reverse ? mine_first.k - mine.k : mine.k - mine_first.k;
                have_mine    = true;
            }
            else
                bad = true;
        }
        if (have_mine && crossings <= kCigarOwnCrossings)
            for (uint32_t j = 0; j < crossings; j++)
                store_crossing(record0, k0, mine_first, j, a.window_length, reverse);
        uint64_t wide = __ballot(have_mine && crossings > kCigarOwnCrossings);
        while (wide)
        {
            const int from = __ffsll((long long)wide) - 1;
            wide &= wide - 1;
            Mark first;
            first.k              = uniform(uint32_t(__shfl(int(mine_first.k), from, 64)));
            first.q              = uniform(uint32_t(__shfl(int(mine_first.q), from, 64)));
            first.t              = uniform(uint32_t(__shfl(int(mine_first.t), from, 64)));
            const uint32_t count = uniform(uint32_t(__shfl(int(crossings), from, 64)));
            for (uint32_t j = lane; j < count; j += 64)
                store_crossing(record0, k0, first, j, a.window_length, reverse);
        }

        // the first state of the lane's run against the last match state before it
        const uint64_t with_marks = __ballot(have_mine);
        const uint64_t before     = with_marks & ((uint64_t(1) << lane) - 1);
        const int from            = before ? 63 - __clzll((long long)before) : 0;
        Mark prev;
        prev.k = uint32_t(__shfl(int(mine.k), from, 64));
        prev.q = uint32_t(__shfl(int(mine.q), from, 64));
        prev.t = uint32_t(__shfl(int(mine.t), from, 64));
        bool have_prev = before != 0;
        if (!have_prev && have_last)
        {
            prev      = last;
            have_prev = true;
        }
        if (have_mine)
        {
            if (!have_prev)
                store_mark(record0, k0, mine_first, true, reverse);
            else if (prev.k != mine_first.k)
            {
                store_mark(record0, k0, prev, false, reverse);
                store_mark(record0, k0, mine_first, true, reverse);
            }
        }
        if (with_marks)
        {
            const int top = 63 - __clzll((long long)with_marks);
            last.k        = uniform(uint32_t(__shfl(int(mine.k), top, 64)));
            last.q        = uniform(uint32_t(__shfl(int(mine.q), top, 64)));
            last.t        = uniform(uint32_t(__shfl(int(mine.t), top, 64)));
            have_last     = true;
        }
        done_t = add_capped(done_t, tile_t);
        done_q = add_capped(done_q, tile_q);
    }

    if (have_last && lane == 0)
        store_mark(record0, k0, last, false, reverse);
    const bool misfit = __ballot(bad) != 0 || done_t != span_t || done_q != span_q;
    if (lane == 0)
        a.status[o] = misfit;
}

} // namespace

void launch_window_cut_cigar(const CigarSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                             gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                             hipStream_t stream)
{
    if (n == 0)
        return;
    if (n < 0 || n >= (int64_t(1) << 31) || window_length <= 0)
        throw std::invalid_argument("window cut: bad overlap count or window length");
    if (source.num_ops < 0 || !source.ops || !source.offsets)
        throw std::invalid_argument("window cut: no ops or op offsets");
    CigarArgs a;
    a.ops           = source.ops;
    a.num_ops       = source.num_ops;
    a.offsets       = source.offsets;
    a.overlaps      = reinterpret_cast<const uint32_t*>(d_overlaps);
    a.record_base   = d_record_base;
    a.records       = reinterpret_cast<uint32_t*>(d_records);
    a.status        = d_status;
    a.n             = uint32_t(n);
    a.window_length = uint32_t(window_length);
    a.w             = window_divisor(uint32_t(window_length));
    const unsigned blocks = unsigned((n + kCutWaves - 1) / kCutWaves);
    window_segments_cigar_kernel<<<blocks, kThreads, 0, stream>>>(a);
    GWAMD_HIP_CHECK(hipGetLastError());
}

} // namespace polish
} // namespace gwamd
