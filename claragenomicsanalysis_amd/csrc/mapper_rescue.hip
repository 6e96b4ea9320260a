// Overlap-end rescue on the GPU (reference Overlapper::rescue_overlap_ends and
// details::overlapper::extend_overlap_by_sequence_similarity,
// cudamapper/src/overlapper.cpp:254-365; sequence_jaccard_similarity,
// cudamapper/src/cudamapper_utils.cpp:114-170).
//
// One wave owns one overlap from its record to its record: no workgroup
// barrier.  A round stages the (at most) four windows of the two ends, each at
// most kMaxRescueExtension bytes, in the wave's slice of LDS; the target's
// windows of a Reverse overlap are read through the mirrored address and
// complemented on load, so no reversed copy of a read exists anywhere.
//
// Similarity of two windows of L bytes.  L < 15: each side is one string.
// Otherwise side s has n = L - 14 substrings, substring i = s[i, min(L, 2i + 15))
// (the reference's substr(i, i + 15) takes a count, not an end), of length
// min(i + 15, L - i).  That length rises strictly, then falls strictly, so only
// substrings i and n - 1 - i have it: substring i of one window can equal only
// those two of the other window, or of its own.  Lane i counts its substring
// into the multiset intersection when its rank among its own window's copies
// (0 or 1) is below its number of copies in the other window (0, 1 or 2); a
// ballot sums the lanes.  Every compare is of whole substrings, four bytes at
// a step; nothing is hashed.
//
// An end that a round refused, or accepted with nothing to add, meets the
// same windows in the next round; it is left out of the later rounds.
#include "mapper_prims.hpp"
#include "mapper_reads.hpp"

namespace gwamd
{
namespace mapper
{
namespace
{

constexpr uint32_t kWaves       = kThreads / 64;
constexpr uint32_t kWindowWords = kMaxRescueExtension / 4 + 4; // a four-byte step may read one word past the window
constexpr uint32_t kOverlapWords = sizeof(OverlapRecord) / sizeof(uint32_t);
static_assert(kMaxRescueExtension % 4 == 0 && kMaxRescueExtension <= 128, "two bytes and two substrings per lane");

__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a value every lane of the wave holds, in a scalar register
__device__ inline uint32_t uniform(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ inline int64_t uniform(int64_t v)
{
    return int64_t((uint64_t(uniform(uint32_t(uint64_t(v) >> 32))) << 32) | uniform(uint32_t(v)));
}

// bytes p .. p + 3 of a window
__device__ inline uint32_t four_bytes(const uint32_t* w, uint32_t p)
{
    const uint64_t pair = (uint64_t(w[(p >> 2) + 1]) << 32) | w[p >> 2];
    return uint32_t(pair >> (8 * (p & 3)));
}

// a[pa, pa + len) == b[pb, pb + len)
__device__ inline bool same_bytes(const uint32_t* a, uint32_t pa, const uint32_t* b, uint32_t pb, uint32_t len)
{
    for (uint32_t k = 0; k < len; k += 4)
    {
        uint32_t diff = four_bytes(a, pa + k) ^ four_bytes(b, pb + k);
        if (len - k < 4)
            diff &= (1u << (8 * (len - k))) - 1;
        if (diff)
            return false;
    }
    return true;
}

// sequence_jaccard_similarity(a, b, 15, 1) >= required_similarity for two
// windows of len bytes; the same on every lane
__device__ inline bool accepted(const uint32_t* a, const uint32_t* b, uint32_t len, float required_similarity,
                                uint32_t lane)
{
    uint32_t n = 1, shared = 0;
    if (len < uint32_t(kRescueKmer))
        shared = same_bytes(a, 0, b, 0, len);
    else
    {
        n = len - kRescueKmer + 1;
        for (uint32_t first = 0; first < n; first += 64)
        {
            const uint32_t i = first + lane;
            bool counts      = false;
            if (i < n)
            {
                const uint32_t j   = n - 1 - i; // the other substring of this length
                const uint32_t sub = min(i + kRescueKmer, len - i);
                uint32_t in_b      = same_bytes(a, i, b, i, sub);
                uint32_t rank      = 0;
                if (j != i)
                {
                    in_b += same_bytes(a, i, b, j, sub);
                    rank = j < i && same_bytes(a, i, a, j, sub);
                }
                counts = rank < in_b;
            }
            shared += uint32_t(__popcll(__ballot(counts)));
        }
    }
    // IEEE float32 quotient against a float32 threshold
    return float(shared) / float(2 * n - shared) >= required_similarity;
}

// Base j of the target as the rounds see it: of the read, or for a Reverse
// overlap of what the reference's reverse_complement leaves (overlapper.cpp:94-109):
// A<->T and C<->G, every other byte as it is, and the middle base of a read of
// odd length not complemented.
__device__ inline uint8_t target_base(const uint8_t* t, uint32_t len, bool reverse, uint32_t j)
{
    if (!reverse)
        return t[j];
    const uint8_t c = t[len - 1 - j];
    if ((len & 1) && j == len / 2)
        return c;
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

__global__ __launch_bounds__(kThreads) void rescue_kernel(const uint8_t* __restrict__ query_bases,
                                                          const int64_t* __restrict__ query_offsets,
                                                          const uint8_t* __restrict__ target_bases,
                                                          const int64_t* __restrict__ target_offsets,
                                                          uint32_t* __restrict__ overlaps, uint32_t n,
                                                          uint32_t extension, float required_similarity)
{
    // query head, target head, query tail, target tail of each wave
    __shared__ uint32_t windows[kWaves][4][kWindowWords];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t o    = blockIdx.x * kWaves + wave;
    if (o >= n)
        return;
    uint32_t* record = overlaps + size_t(o) * kOverlapWords;

    const uint32_t query_id  = uniform(record[0]);
    const uint32_t target_id = uniform(record[1]);
    uint32_t qs              = uniform(record[2]);
    uint32_t ts              = uniform(record[3]);
    uint32_t qe              = uniform(record[4]);
    uint32_t te              = uniform(record[5]);
    const bool reverse       = (uniform(record[6]) & 0xff) == '-';
    const int64_t q_first    = uniform(query_offsets[query_id]);
    const int64_t t_first    = uniform(target_offsets[target_id]);
    const uint32_t q_len     = uint32_t(uniform(query_offsets[query_id + 1]) - q_first);
    const uint32_t t_len     = uint32_t(uniform(target_offsets[target_id + 1]) - t_first);
    const uint8_t* q         = query_bases + q_first;
    const uint8_t* t         = target_bases + t_first;
    if (reverse)
    {
        const uint32_t start = ts;
        ts                   = t_len - te;
        te                   = t_len - start;
    }

    uint32_t* q_head = windows[wave][0];
    uint32_t* t_head = windows[wave][1];
    uint32_t* q_tail = windows[wave][2];
    uint32_t* t_tail = windows[wave][3];
    bool head_open = true, tail_open = true;
    for (int round = 0; round < kRescueRounds && (head_open || tail_open); round++)
    {
        const uint32_t head = head_open ? min(min(qs, ts), extension) : 0;
        const uint32_t tail = tail_open ? min(extension, min(q_len - qe, t_len - te)) : 0;
        for (uint32_t p = lane; p < head; p += 64)
        {
            reinterpret_cast<uint8_t*>(q_head)[p] = q[qs - head + p];
            reinterpret_cast<uint8_t*>(t_head)[p] = target_base(t, t_len, reverse, ts - head + p);
        }
        for (uint32_t p = lane; p < tail; p += 64)
        {
            reinterpret_cast<uint8_t*>(q_tail)[p] = q[qe + p];
            reinterpret_cast<uint8_t*>(t_tail)[p] = target_base(t, t_len, reverse, te + p);
        }
        wave_sync();
        if (head_open)
        {
            const bool ok = accepted(q_head, t_head, head, required_similarity, lane);
            head_open     = ok && head > 0;
            if (ok)
            {
                qs -= head;
                ts -= head;
            }
        }
        if (tail_open)
        {
            const bool ok = accepted(q_tail, t_tail, tail, required_similarity, lane);
            tail_open     = ok && tail > 0;
            if (ok)
            {
                qe += tail;
                te += tail;
            }
        }
        wave_sync(); // the next round writes the windows
    }

    if (reverse)
    {
        const uint32_t start = ts;
        ts                   = t_len - te;
        te                   = t_len - start;
    }
    // words 2..5: query_start, target_start, query_end, target_end
    if (lane < 4)
        record[2 + lane] = lane == 0 ? qs : lane == 1 ? ts : lane == 2 ? qe : te;
}

template <typename T>
void upload(DevBuf<T>& d, const void* src, size_t count, const Budget& budget, hipStream_t stream)
{
    d.alloc(count, budget);
    if (count > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(d.data(), src, count * sizeof(T), hipMemcpyHostToDevice, stream));
}

} // namespace

void rescue_overlap_ends(OverlapRecord* overlaps, int64_t n, const ReadSet& query, const ReadSet& target,
                         int extension, float required_similarity, const Budget& budget, hipStream_t stream)
{
    const bool one_side = query.bases == target.bases && query.offsets == target.offsets &&
                          query.num_reads == target.num_reads;
    DevBuf<uint8_t> query_bases, target_bases;
    DevBuf<int64_t> query_offsets, target_offsets;
    DevBuf<OverlapRecord> records;
    upload(query_bases, query.bases, size_t(query.offsets[query.num_reads]), budget, stream);
    upload(query_offsets, query.offsets, size_t(query.num_reads) + 1, budget, stream);
    if (!one_side)
    {
        upload(target_bases, target.bases, size_t(target.offsets[target.num_reads]), budget, stream);
        upload(target_offsets, target.offsets, size_t(target.num_reads) + 1, budget, stream);
    }
    upload(records, overlaps, size_t(n), budget, stream);
    const unsigned blocks = unsigned((n + kWaves - 1) / kWaves);
    rescue_kernel<<<blocks, kThreads, 0, stream>>>(
        query_bases.data(), query_offsets.data(), one_side ? query_bases.data() : target_bases.data(),
        one_side ? query_offsets.data() : target_offsets.data(), reinterpret_cast<uint32_t*>(records.data()),
        uint32_t(n), uint32_t(extension), required_similarity);
    check_launch();
    GWAMD_HIP_CHECK(
        hipMemcpyAsync(overlaps, records.data(), size_t(n) * sizeof(OverlapRecord), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
}

// The same kernel on reads that are already on the device: the records go up and come back.
void rescue_overlap_ends(OverlapRecord* overlaps, int64_t n, const DeviceReads& query, const DeviceReads& target,
                         int extension, float required_similarity, const Budget& budget, hipStream_t stream)
{
    DevBuf<OverlapRecord> records;
    upload(records, overlaps, size_t(n), budget, stream);
    const unsigned blocks = unsigned((n + kWaves - 1) / kWaves);
    rescue_kernel<<<blocks, kThreads, 0, stream>>>(query.bases(), query.d_offsets.data(), target.bases(),
                                                   target.d_offsets.data(),
                                                   reinterpret_cast<uint32_t*>(records.data()), uint32_t(n),
                                                   uint32_t(extension), required_similarity);
    check_launch();
    GWAMD_HIP_CHECK(
        hipMemcpyAsync(overlaps, records.data(), size_t(n) * sizeof(OverlapRecord), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
}

} // namespace mapper
} // namespace gwamd
