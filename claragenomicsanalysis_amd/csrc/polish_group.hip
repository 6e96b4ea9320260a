// Window grouping on the device (polish_group.hpp): cut records -> the arrays of
// gwamd_window_slices_view, element for element what group_slices
// (polish_windows_host.cpp) builds on one host thread.
//
// Five passes over S records and W windows, none of which lets an atomic or the
// order of the waves decide a position:
//
//   classify  a thread per record: which overlap and window the record belongs
//             to (read from a completed record; for a raw one found in
//             record_base, which folds complete_records in), the flags and the
//             2 % rule.  key = the global window id of a record that counts,
//             W + 1 of one that does not; value = overlap << 32 | record index.
//   quality   a wave per record that counts, with qualities only: the sum of
//             its quality characters, read as aligned 32-bit words with the
//             bytes outside [q_begin, q_end) masked, reduced across the wave
//             in registers.  A record below the threshold gets key W.
//   sort      hipCUB's stable radix sort of (key, value) by key: the records
//             of a window keep the order of the record array.
//   count     a thread per window: its records are sorted[lower_bound(g),
//             lower_bound(g + 1)), the first cap - 1 of them are kept.  The
//             exclusive sum of 1 + kept gives every window's first sequence.
//   emit      a thread per window writes its backbone, a thread per sorted
//             record with rank < cap - 1 its slice.
//
// dropped_by_quality is the number of keys W and dropped_by_cap the number
// of keys below W less the slices written, both read off the sorted keys.
#include "mapper_gather.hpp"
#include "mapper_prims.hpp"
#include "polish_group.hpp"

namespace gwamd
{
namespace polish
{
namespace
{

using namespace gwamd::mapper;

constexpr uint32_t kWaves = kThreads / 64;

// the last i in [0, n) with a[i] <= v; a[0] <= v (a ascends)
__device__ inline uint32_t last_not_above(const uint32_t* __restrict__ a, uint32_t n, uint32_t v)
{
    uint32_t lo = 0, hi = n; // a[lo] <= v < a[hi] (a[n] counts as infinite)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the first p in [0, n] with keys[p] >= v
__device__ inline uint32_t lower_bound(const uint64_t* __restrict__ keys, uint32_t n, uint64_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

struct Located
{
    uint32_t overlap;
    uint32_t window; // k within the target
    bool counts;     // before the 2 % rule
};

__device__ inline Located locate(const GroupInput& in, uint32_t s, const gwamd_window_segment& r)
{
    Located at;
    if (!in.record_base)
    {
        at.overlap = r.overlap;
        at.window  = r.window;
        at.counts  = (r.flags & (GWAMD_SEGMENT_EMPTY | GWAMD_SEGMENT_BAD_PATH | GWAMD_SEGMENT_NOT_ALIGNED)) == 0;
        return at;
    }
    // (an overlap without records has base[i] == base[i + 1]: the last i with base[i] <= s owns s)
    at.overlap          = last_not_above(in.record_base, uint32_t(in.num_overlaps), s);
    const uint32_t slot = in.status_slot[at.overlap];
    at.window = in.overlaps[at.overlap].target_start / uint32_t(in.window_length) + (s - in.record_base[at.overlap]);
    at.counts = slot != kNotAligned && in.status[slot] == 0 && r.q_end != 0;
    return at;
}

__global__ __launch_bounds__(kThreads) void classify_records_kernel(GroupInput in, uint64_t* __restrict__ keys,
                                                                    uint64_t* __restrict__ vals)
{
    const uint64_t s = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (s >= uint64_t(in.num_records))
        return;
    const gwamd_window_segment r = in.records[s];
    const Located at             = locate(in, uint32_t(s), r);
    uint64_t key                 = uint64_t(in.num_windows) + 1;
    if (at.counts && (int64_t(r.q_end) - int64_t(r.q_begin)) * 50 >= int64_t(in.window_length))
        key = uint64_t(in.window_first[in.overlaps[at.overlap].target_read_id]) + at.window;
    keys[s] = key;
    vals[s] = uint64_t(at.overlap) << 32 | s;
}

// the sum of v over the wave, in every lane's return value (v below 2^25)
__device__ inline uint32_t wave_sum(uint32_t v)
{
    int x = int(v);
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true); // row_shr 1, 2, 4, 8
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false); // row_bcast 15, 31
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return uint32_t(__builtin_amdgcn_readlane(x, 63));
}

// One wave per record.  The record's facts are wave-uniform and held in SGPRs;
// a lane adds the bytes of every 64th word into a 64-bit sum, so nothing wraps
// for a segment as long as a read (below 2^31 bases of at most 255 each).
__global__ __launch_bounds__(kThreads) void quality_filter_kernel(GroupInput in, uint64_t* __restrict__ keys,
                                                                  const uint64_t* __restrict__ vals)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (wave >= uint64_t(in.num_records))
        return;
    const uint32_t s = uniform(uint32_t(wave));
    if (uniform(uint32_t(keys[s])) >= uint32_t(in.num_windows)) // the keys are below 2^32
        return;
    const uint32_t overlap = uniform(uint32_t(vals[s] >> 32));
    const uint32_t q_begin = uniform(in.records[s].q_begin);
    const uint32_t length  = uniform(in.records[s].q_end) - q_begin; // at least 1: the 2 % rule held
    const uint32_t query   = uniform(in.overlaps[overlap].query_read_id);
    const uintptr_t first =
        reinterpret_cast<uintptr_t>(in.query_qualities) + uintptr_t(in.query_offsets[query]) + q_begin;
    // bytes [lead, lead + length) of the aligned words from `words` on
    const uint32_t* words    = reinterpret_cast<const uint32_t*>(first & ~uintptr_t(3));
    const uint32_t lead      = uint32_t(first & 3);
    const uint32_t num_words = (lead + length + 3) / 4; // below 2^29
    const uint32_t tail      = (lead + length) & 3;     // bytes of the last word that count; 0: all four
    uint64_t sum             = 0;
    for (uint32_t i = lane; i < num_words; i += 64)
    {
        uint32_t w = words[i];
        if (i == 0)
            w &= 0xffffffffu << (8 * lead);
        if (i == num_words - 1 && tail != 0)
            w &= 0xffffffffu >> (8 * (4 - tail));
        const uint32_t pairs = (w & 0x00ff00ffu) + ((w >> 8) & 0x00ff00ffu);
        sum += (pairs & 0xffffu) + (pairs >> 16);
    }
    // a lane's sum is below 2^25 * 255 < 2^33: its low 24 bits and the rest add up without a wrap
    const uint64_t high = wave_sum(uint32_t(sum >> 24));
    const uint64_t low  = wave_sum(uint32_t(sum) & 0xffffffu);
    const int64_t phred = int64_t((high << 24) + low) - int64_t(33) * int64_t(length);
    if (lane == 0 && phred * 10 < int64_t(in.quality_threshold_tenths) * int64_t(length))
        keys[s] = uint64_t(in.num_windows);
}

// Window g < W: start[g] and its number of sequences; thread W writes the two
// totals start[W] (records that count) and start[W + 1] (those and the ones the
// quality filter dropped) and a count of 0 for the exclusive sum's last entry.
__global__ __launch_bounds__(kThreads) void count_windows_kernel(const uint64_t* __restrict__ sorted_keys,
                                                                 uint32_t num_records, uint32_t num_windows,
                                                                 uint32_t cap, uint32_t* __restrict__ start,
                                                                 int32_t* __restrict__ counts)
{
    const uint64_t g = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (g > num_windows)
        return;
    const uint32_t lo = lower_bound(sorted_keys, num_records, g);
    const uint32_t hi = lower_bound(sorted_keys, num_records, g + 1);
    start[g]          = lo;
    if (g == num_windows)
    {
        start[g + 1] = hi;
        counts[g]    = 0;
    }
    else
        counts[g] = int32_t(1 + min(hi - lo, cap - 1));
}

struct GroupArrays
{
    gwamd_read_slice* slices;
    uint32_t* window_target;
    uint32_t* window_index;
    int32_t* sequence_overlap;
    int32_t* sequence_t_begin;
    int32_t* sequence_t_end;
};

__global__ __launch_bounds__(kThreads) void emit_backbones_kernel(GroupInput in, const int32_t* __restrict__ first_seq,
                                                                  GroupArrays out)
{
    const uint64_t g = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (g >= uint64_t(in.num_windows))
        return;
    // (a target of length 0 has first[r] == first[r + 1]: the last r with first[r] <= g owns g)
    const uint32_t r   = last_not_above(in.window_first, uint32_t(in.num_targets), uint32_t(g));
    const uint32_t k   = uint32_t(g) - in.window_first[r];
    const int64_t size = in.target_offsets[r + 1] - in.target_offsets[r];
    const int64_t from = int64_t(k) * in.window_length;
    const int64_t to   = min(from + in.window_length, size);
    const int32_t at   = first_seq[g];
    out.slices[at]           = gwamd_read_slice{0, r, uint32_t(from), uint32_t(to), 0u};
    out.sequence_overlap[at] = -1;
    out.sequence_t_begin[at] = 0;
    out.sequence_t_end[at]   = int32_t(to - from);
    out.window_target[g]     = r;
    out.window_index[g]      = k;
}

__global__ __launch_bounds__(kThreads) void emit_slices_kernel(GroupInput in, const uint64_t* __restrict__ sorted_keys,
                                                               const uint64_t* __restrict__ sorted_vals,
                                                               const uint32_t* __restrict__ start,
                                                               const int32_t* __restrict__ first_seq, GroupArrays out)
{
    const uint64_t p = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p >= uint64_t(in.num_records) || p >= start[in.num_windows])
        return;
    const uint32_t g    = uint32_t(sorted_keys[p]);
    const uint32_t rank = uint32_t(p) - start[g];
    if (rank >= uint32_t(in.max_sequences_per_window) - 1)
        return;
    const uint64_t v             = sorted_vals[p];
    const uint32_t overlap       = uint32_t(v >> 32);
    const gwamd_window_segment r = in.records[uint32_t(v)];
    const OverlapRecord& o       = in.overlaps[overlap];
    const uint32_t k             = g - in.window_first[o.target_read_id];
    const int64_t from           = int64_t(k) * in.window_length;
    const int32_t at             = first_seq[g] + 1 + int32_t(rank);
    // (a completed record carries the strand in its flags, and that is what group_slices reads)
    const bool reverse = in.record_base ? o.relative_strand == '-' : (r.flags & GWAMD_SEGMENT_REVERSE) != 0;
    out.slices[at]     = gwamd_read_slice{1, o.query_read_id, r.q_begin, r.q_end, reverse ? GWAMD_SLICE_REVERSE : 0u};
    out.sequence_overlap[at] = int32_t(overlap);
    out.sequence_t_begin[at] = int32_t(int64_t(r.t_begin) - from);
    out.sequence_t_end[at]   = int32_t(int64_t(r.t_end) - from);
}

template <typename T>
void download(std::vector<T>& out, const DevBuf<T>& d, size_t count, hipStream_t stream)
{
    out.resize(count);
    if (count > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(out.data(), d.data(), count * sizeof(T), hipMemcpyDeviceToHost, stream));
}

} // namespace

void group_on_device(const GroupInput& in, GroupOutput& out, const Budget& budget, hipStream_t stream)
{
    out = GroupOutput{};
    const size_t S = size_t(in.num_records), W = size_t(in.num_windows);
    if (W == 0)
        return;
    if (in.num_records >= (int64_t(1) << 31) || in.num_windows >= (int64_t(1) << 31) ||
        in.num_overlaps >= (int64_t(1) << 31) || in.max_sequences_per_window < 1 || in.window_length < 1)
        throw std::invalid_argument("group_on_device: a count of 2^31 or more, or a cap or window length below 1");
    DevBuf<uint64_t> keys(std::max<size_t>(S, 1), budget), vals(std::max<size_t>(S, 1), budget);
    DevBuf<uint64_t> sorted_keys(std::max<size_t>(S, 1), budget), sorted_vals(std::max<size_t>(S, 1), budget);
    DevBuf<uint32_t> start(W + 2, budget);
    DevBuf<int32_t> counts(W + 1, budget), first_seq(W + 1, budget);
    if (S > 0)
    {
        classify_records_kernel<<<blocks_for(S, uint64_t(1) << 31), kThreads, 0, stream>>>(in, keys.data(),
                                                                                             vals.data());
        check_launch();
        if (in.query_qualities)
        {
            quality_filter_kernel<<<unsigned((S + kWaves - 1) / kWaves), kThreads, 0, stream>>>(in, keys.data(),
                                                                                                vals.data());
            check_launch();
        }
        sort_pairs(keys.data(), sorted_keys.data(), vals.data(), sorted_vals.data(), S, bit_length(uint64_t(W) + 1),
                   budget, stream);
    }
    count_windows_kernel<<<blocks_for(W + 1, uint64_t(1) << 31), kThreads, 0, stream>>>(
        sorted_keys.data(), uint32_t(S), uint32_t(W), uint32_t(in.max_sequences_per_window), start.data(),
        counts.data());
    check_launch();
    exclusive_sum(counts.data(), first_seq.data(), W + 1, budget, stream);
    uint32_t totals[2] = {0, 0}; // records that count; those and the quality filter's
    int32_t num_seqs   = 0;
    GWAMD_HIP_CHECK(hipMemcpyAsync(totals, start.data() + W, sizeof(totals), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipMemcpyAsync(&num_seqs, first_seq.data() + W, sizeof(num_seqs), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    // (every window has its backbone: num_seqs >= W >= 1)
    const size_t N = size_t(num_seqs);
    DevBuf<gwamd_read_slice> slices(N, budget);
    DevBuf<uint32_t> window_target(W, budget), window_index(W, budget);
    DevBuf<int32_t> sequence_overlap(N, budget), sequence_t_begin(N, budget), sequence_t_end(N, budget);
    const GroupArrays arrays{slices.data(),           window_target.data(),    window_index.data(),
                             sequence_overlap.data(), sequence_t_begin.data(), sequence_t_end.data()};
    emit_backbones_kernel<<<blocks_for(W, uint64_t(1) << 31), kThreads, 0, stream>>>(in, first_seq.data(), arrays);
    check_launch();
    if (S > 0)
    {
        emit_slices_kernel<<<blocks_for(S, uint64_t(1) << 31), kThreads, 0, stream>>>(
            in, sorted_keys.data(), sorted_vals.data(), start.data(), first_seq.data(), arrays);
        check_launch();
    }
    download(out.slices, slices, N, stream);
    download(out.window_counts, counts, W, stream);
    download(out.window_target, window_target, W, stream);
    download(out.window_index, window_index, W, stream);
    download(out.sequence_overlap, sequence_overlap, N, stream);
    download(out.sequence_t_begin, sequence_t_begin, N, stream);
    download(out.sequence_t_end, sequence_t_end, N, stream);
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    out.dropped_by_quality = int64_t(totals[1]) - int64_t(totals[0]);
    out.dropped_by_cap     = int64_t(totals[0]) - (int64_t(N) - int64_t(W));
}

} // namespace polish
} // namespace gwamd
