// cudapolish: aligned overlaps cut into target windows (racon's
// find_breaking_points on AlignmentState paths; semantics in
// include/gwamd_polish.h).
//
// One wave owns one overlap from the first byte of its path to the last: no
// workgroup barrier, no LDS.  The path is walked in memory order in tiles of
// 64 aligned 16-byte chunks, a lane one chunk; bytes of a chunk outside
// [A, A + len) are masked and never interpreted.  Per tile
//   - a lane sums the (target, query) advances of its 16 states, packed in
//     one register (at most 16 each);
//   - an exclusive wave scan of the packed sums plus the carry of the earlier
//     tiles gives the lane the offsets before its first state;
//   - the lane walks its 16 states.  For a match or mismatch state it forms
//     (q, t, k = t / w), only after checking that the offsets lie inside the
//     overlap, so a path of any bytes never yields a record or a position
//     outside its overlap's own range.  Where k differs from the k of the
//     match state before it in the lane, that state closes its window's run
//     and this one opens its own;
//   - the first match state of a lane meets the last one of the nearest lane
//     before it that has one (a ballot names the lane, three shuffles fetch k,
//     q, t), or the carry of the earlier tiles, in the same way.
// A state that opens a run stores the two words it defines into its window's
// record, one that closes it the other two: every word has one writer, plain
// vector stores, the result does not depend on timing.  Walked end -> start
// (the aligner's order) the offsets count down from the overlap's lengths and
// "opens" and "closes" swap their words.
//
// k = t / w is a multiplication by a reciprocal the host prepares (w is the
// same for every state of a launch).
#include "polish_cut.hpp"

namespace gwamd
{
namespace polish
{
namespace
{

constexpr uint32_t kThreads = kCutWaves * 64;
static_assert(kCutTileStates == 64 * 16, "16 states per lane");

struct CutArgs
{
    const uint8_t* paths;
    int64_t paths_bytes;
    const int64_t* offsets;
    int64_t stride;
    int64_t first;
    const int32_t* lengths;
    int32_t max_length;
    uint32_t end_to_start;
    const uint32_t* overlaps;
    const uint32_t* record_base;
    uint32_t* records;
    uint32_t* status;
    uint32_t n;
    WindowDivisor w;
};

__global__ __launch_bounds__(kThreads) void window_segments_kernel(const CutArgs a)
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
    const uint32_t span_t = te - ts, span_q = qe - qs; // the host has checked start <= end
    const uint32_t k0     = window_of(ts, a.w);
    uint32_t* record0     = a.records + size_t(uniform(a.record_base[o])) * kRecordWords;
    const bool backwards  = a.end_to_start != 0;

    // the path's bytes: [begin, begin + len) of the buffer, cut to the buffer
    const int64_t begin  = a.offsets ? uniform(a.offsets[o]) : (a.first + int64_t(o)) * a.stride;
    const int32_t stated = int32_t(uniform(uint32_t(a.lengths[o])));
    int64_t len          = stated < 0 ? 0 : stated > a.max_length ? a.max_length : stated;
    if (begin < 0 || begin > a.paths_bytes)
        len = 0;
    else if (len > a.paths_bytes - begin)
        len = a.paths_bytes - begin;
    bool bad = len != int64_t(stated);

    uint32_t done_t = 0, done_q = 0; // target and query advances of the tiles walked
    bool have_last  = false;         // the last match state of the tiles walked (the same on every lane)
    Mark last{0, 0, 0};

    const int64_t end        = begin + len;
    const int64_t chunk_end  = (end + 15) >> 4;
    for (int64_t chunk0 = begin >> 4; chunk0 < chunk_end; chunk0 += 64)
    {
        const int64_t chunk = chunk0 + lane;
        const int64_t at    = chunk << 4;
        uint32_t word[4]    = {0, 0, 0, 0};
        int32_t lo = 0, hi = 0; // the lane's bytes [lo, hi) belong to the path
        if (chunk < chunk_end)
        {
            lo = int32_t(begin > at ? begin - at : 0);
            hi = int32_t(end - at < 16 ? end - at : 16);
            if (at + 16 <= a.paths_bytes)
            {
                const uint4 v = *reinterpret_cast<const uint4*>(a.paths + at);
                word[0] = v.x, word[1] = v.y, word[2] = v.z, word[3] = v.w;
            }
            else
            {
                for (int d = 0; d < 4; d++)
                    if (4 * d < hi && 4 * d + 4 > lo && at + 4 * d + 4 <= a.paths_bytes)
                        word[d] = *reinterpret_cast<const uint32_t*>(a.paths + at + 4 * d);
            }
        }

        // advances of the lane's states: target in the low half, query in the high half
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < 16; j++)
        {
            const uint32_t s = (word[j >> 2] >> (8 * (j & 3))) & 0xff;
            if (j >= lo && j < hi)
            {
                if (s > 3)
                    bad = true;
                else
                    sum += uint32_t(s != 3) | (uint32_t(s != 2) << 16);
            }
        }
        uint32_t scan = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t below = uint32_t(__shfl_up(int(scan), d, 64));
            if (lane >= uint32_t(d))
                scan += below;
        }
        const uint32_t tile = uniform(uint32_t(__shfl(int(scan), 63, 64)));
        uint32_t at_t = done_t + ((scan - sum) & 0xffff);
        uint32_t at_q = done_q + ((scan - sum) >> 16);

        // the lane's walk: its first and last match state, and every change of window between them
        bool have_mine = false;
        Mark mine_first{0, 0, 0}, mine{0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; j++)
        {
            const uint32_t s = (word[j >> 2] >> (8 * (j & 3))) & 0xff;
            if (j >= lo && j < hi && s <= 3)
            {
                if (s <= 1)
                {
                    if (at_t < span_t && at_q < span_q)
                    {
                        const uint32_t u = backwards ? span_t - 1 - at_t : at_t;
                        const uint32_t v = backwards ? span_q - 1 - at_q : at_q;
                        Mark m;
                        m.t = reverse ? te - 1 - u : ts + u;
                        m.q = qs + v;
                        m.k = window_of(m.t, a.w);
                        if (!have_mine)
                            mine_first = m;
                        else if (m.k != mine.k)
                        {
                            store_mark(record0, k0, mine, backwards, reverse);
                            store_mark(record0, k0, m, !backwards, reverse);
                        }
                        mine      = m;
                        have_mine = true;
                    }
                    else
                        bad = true;
                }
                at_t += s != 3;
                at_q += s != 2;
            }
        }

        // the lane's first match state against the last one before it
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
                store_mark(record0, k0, mine_first, !backwards, reverse);
            else if (prev.k != mine_first.k)
            {
                store_mark(record0, k0, prev, backwards, reverse);
                store_mark(record0, k0, mine_first, !backwards, reverse);
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
        done_t += tile & 0xffff;
        done_q += tile >> 16;
    }

    if (have_last && lane == 0)
        store_mark(record0, k0, last, backwards, reverse);
    const bool misfit = __ballot(bad) != 0 || done_t != span_t || done_q != span_q;
    if (lane == 0)
        a.status[o] = misfit;
}

} // namespace

void launch_window_cut(const PathSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                       gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                       hipStream_t stream)
{
    if (n == 0)
        return;
    if (n < 0 || n >= (int64_t(1) << 31) || window_length <= 0)
        throw std::invalid_argument("window cut: bad overlap count or window length");
    if (reinterpret_cast<uintptr_t>(source.paths) % 16 != 0 || source.paths_bytes < 0)
        throw std::invalid_argument("window cut: the path buffer is not 16-byte aligned");
    CutArgs a;
    a.paths        = reinterpret_cast<const uint8_t*>(source.paths);
    a.paths_bytes  = source.paths_bytes;
    a.offsets      = source.offsets;
    a.stride       = source.stride;
    a.first        = source.first;
    a.lengths      = source.lengths;
    a.max_length   = source.max_length;
    a.end_to_start = source.end_to_start;
    a.overlaps     = reinterpret_cast<const uint32_t*>(d_overlaps);
    a.record_base  = d_record_base;
    a.records      = reinterpret_cast<uint32_t*>(d_records);
    a.status       = d_status;
    a.n            = uint32_t(n);
    a.w            = window_divisor(uint32_t(window_length));
    const unsigned blocks = unsigned((n + kCutWaves - 1) / kCutWaves);
    window_segments_kernel<<<blocks, kThreads, 0, stream>>>(a);
    GWAMD_HIP_CHECK(hipGetLastError());
}

} // namespace polish
} // namespace gwamd
