// (k,w)-minimizer index on the GPU (reference cudamapper/src/minimizer.cu,
// index_gpu.cuh; interface include/.../cudamapper/index.hpp).
//
// Sketch: one kernel over (read, tile) pairs instead of the reference's three
// kernels sized by read length.  A tile owns kTile consecutive windows of one
// read, where window j (0 <= j < K + w - 1, K = n - k + 1 k-mers) covers
// k-mers [max(0, j - w + 1), min(K - 1, j)]: that one formula yields the
// reference's front-end, central and back-end windows.  A window's minimizer
// is its rightmost k-mer of minimal representation, and a window emits a
// sketch element when its minimizer's position differs from the previous
// window's (positions never decrease from one window to the next).  A tile
// stages its k-mers plus a halo of w k-mers on the left, enough to recompute
// the window before its first, so tiles are independent.  The kernel runs
// twice, counting then writing, with an exclusive scan of the tile counts in
// between; the output is exactly sized and in (read, position) order without
// atomics.
//
// Index: a stable radix sort by representation of the (read, position)-ordered
// elements gives the (representation, read_id, position) order; head flags and
// a scan give the unique representations and their first occurrences;
// filtering drops representations with count >= threshold and compacts.
//
// A read shorter than w + k - 1 contributes nothing but keeps its id.  This
// differs from the reference on purpose: there a skipped read shifts the ids
// of the reads after it (index_gpu.cuh:720-734 carries a TODO about it).
#include "mapper_prims.hpp"

#include <vector>

namespace gwamd
{
namespace mapper
{
namespace
{

constexpr int kTile     = 2048;                          // windows per tile
constexpr int kMaxKmers = kTile + kMaxWindowSize;        // tile + halo
constexpr int kMaxBases = kMaxKmers + kMaxKmerSize - 1;  // and k - 1 further bases

// minimizer.cu:55-66: Thomas Wang's 64-bit hash masked to 32 bits
__device__ __forceinline__ uint64_t wang_hash(uint64_t key)
{
    const uint64_t mask = 0xFFFFFFFFull;
    key                 = (~key + (key << 21)) & mask;
    key                 = key ^ (key >> 24);
    key                 = ((key + (key << 3)) + (key << 8)) & mask;
    key                 = key ^ (key >> 14);
    key                 = ((key + (key << 2)) + (key << 4)) & mask;
    key                 = key ^ (key >> 28);
    key                 = (key + (key << 31)) & mask;
    return key;
}

// Forward code in bits 0-1: 3 & ((b >> 2) ^ (b >> 1)), A/a=0 C/c=1 G/g=2 T/t=3.
// Complement code in bits 2-3, by the reference's 8-entry table on b & 7
// (minimizer.cu:147-154, 186): 1 (A) -> 3, 3 (C) -> 2, 4 (T) -> 0, 7 (G) -> 1,
// and 0 for 0, 2, 5, 6, so e.g. N (0x4E) reads as A on both strands.
__device__ __forceinline__ uint8_t base_codes(uint8_t b)
{
    const uint32_t fwd  = 3u & ((b >> 2) ^ (b >> 1));
    const uint32_t comp = (0x10002030u >> (4 * (b & 7))) & 3u;
    return uint8_t(fwd | (comp << 2));
}

__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void sketch_kernel(const char* __restrict__ bases,
                                                          const uint64_t* __restrict__ read_start,
                                                          const uint32_t* __restrict__ read_length,
                                                          const uint32_t* __restrict__ tile_read,
                                                          const uint32_t* __restrict__ tile_first_window, int k, int w,
                                                          int hash_representations, uint32_t first_read_id,
                                                          uint64_t* __restrict__ tile_count,
                                                          const uint64_t* __restrict__ tile_offset,
                                                          uint64_t* __restrict__ keys, uint64_t* __restrict__ values)
{
    __shared__ uint64_t s_rep[kMaxKmers];
    __shared__ uint32_t s_wpos[kTile + 1];
    __shared__ uint8_t s_code[kMaxBases + 1];
    __shared__ uint8_t s_dir[kMaxKmers];
    __shared__ uint32_t s_wave[kThreads / 64];

    const int tid       = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const uint32_t r    = tile_read[tile];
    const int64_t j0    = tile_first_window[tile];
    const int64_t K     = int64_t(read_length[r]) - k + 1;
    const int64_t j1    = imin(j0 + kTile, K + w - 1); // past the tile's last window
    // the window before the tile's first is recomputed from the halo
    const int64_t jfirst = j0 > 0 ? j0 - 1 : 0;
    const int64_t p0     = imax(0, jfirst - w + 1); // first k-mer staged
    const int64_t p1     = imin(K - 1, j1 - 1);     // last k-mer staged
    const int nk         = int(p1 - p0 + 1); // <= kTile + w <= kMaxKmers
    const int nb         = nk + k - 1;       // <= kMaxBases, and p1 + k <= the read's length
    const int nwin       = int(j1 - jfirst); // <= kTile + 1

    const char* src = bases + read_start[r] + p0;
    for (int i = tid; i < nb; i += kThreads)
        s_code[i] = base_codes(uint8_t(src[i]));
    __syncthreads();

    for (int i = tid; i < nk; i += kThreads)
    {
        uint64_t fwd = 0, rev = 0;
        for (int b = 0; b < k; b++)
        {
            const uint32_t c = s_code[i + b];
            fwd              = (fwd << 2) | (c & 3u);
            rev |= uint64_t(c >> 2) << (2 * b);
        }
        if (hash_representations)
        {
            fwd = wang_hash(fwd);
            rev = wang_hash(rev);
        }
        const bool forward = fwd <= rev; // forward wins a tie
        s_rep[i]           = forward ? fwd : rev;
        s_dir[i]           = forward ? 0 : 1;
    }
    __syncthreads();

    // rightmost minimum of every window (<= while scanning left to right)
    for (int t = tid; t < nwin; t += kThreads)
    {
        const int64_t j = jfirst + t;
        const int lo    = int(imax(0, j - w + 1) - p0);
        const int hi    = int(imin(K - 1, j) - p0);
        int best        = lo;
        uint64_t bv     = s_rep[lo];
        for (int p = lo + 1; p <= hi; p++)
        {
            const uint64_t v = s_rep[p];
            if (v <= bv)
            {
                bv   = v;
                best = p;
            }
        }
        s_wpos[t] = uint32_t(best);
    }
    __syncthreads();

    // compaction: ballot and popcount within a wave, wave totals through LDS
    const int lane     = tid & 63;
    const int wave     = tid >> 6;
    uint64_t running   = 0;
    const uint64_t out = WRITE ? tile_offset[tile] : 0;
    for (int c = (j0 > 0 ? 1 : 0); c < nwin; c += kThreads)
    {
        const int t                   = c + tid;
        const bool emit               = t < nwin && (t == 0 || s_wpos[t] != s_wpos[t - 1]);
        const unsigned long long mask = __ballot(emit);
        if (lane == 0)
            s_wave[wave] = uint32_t(__popcll(mask));
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int v = 0; v < kThreads / 64; v++)
        {
            const uint32_t n = s_wave[v];
            before += v < wave ? n : 0;
            total += n;
        }
        if (WRITE && emit)
        {
            const uint64_t dst = out + running + before + uint32_t(__popcll(mask & ((1ull << lane) - 1)));
            const uint32_t p   = s_wpos[t];
            keys[dst]          = s_rep[p];
            values[dst]        = (uint64_t(first_read_id + r) << 32) | (uint64_t(p0 + p) << 1) | s_dir[p];
        }
        running += total;
        __syncthreads();
    }
    if (!WRITE && tid == 0)
        tile_count[tile] = running;
}

__global__ void unpack_kernel(const uint64_t* __restrict__ values, uint64_t n, uint32_t* __restrict__ read_ids,
                              uint32_t* __restrict__ positions, uint8_t* __restrict__ directions)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kThreads)
    {
        const uint64_t v = values[i];
        read_ids[i]      = uint32_t(v >> 32);
        positions[i]     = uint32_t(v & 0xFFFFFFFFull) >> 1;
        directions[i]    = uint8_t(v & 1);
    }
}

// flags[i] = 1 where a new representation starts; flags[n] = 0
__global__ void head_flag_kernel(const uint64_t* __restrict__ rep, uint64_t n, uint32_t* __restrict__ flags)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= n; i += uint64_t(gridDim.x) * kThreads)
        flags[i] = i < n && (i == 0 || rep[i] != rep[i - 1]) ? 1u : 0u;
}

__global__ void first_occurrence_kernel(const uint64_t* __restrict__ rep, uint64_t n,
                                        const uint32_t* __restrict__ flags, const uint32_t* __restrict__ index,
                                        uint32_t num_unique, uint64_t* __restrict__ unique,
                                        uint32_t* __restrict__ first)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kThreads)
    {
        if (flags[i])
        {
            unique[index[i]] = rep[i];
            first[index[i]]  = uint32_t(i);
        }
        if (i == 0)
            first[num_unique] = uint32_t(n);
    }
}

// keep[i] = 1 when element i's representation has fewer than threshold
// elements; index[i] + flags[i] - 1 is that representation's rank; keep[n] = 0
__global__ void keep_flag_kernel(uint64_t n, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ index,
                                 const uint32_t* __restrict__ first, uint64_t threshold, uint32_t* __restrict__ keep)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= n; i += uint64_t(gridDim.x) * kThreads)
    {
        uint32_t kept = 0;
        if (i < n)
        {
            const uint32_t u = index[i] + flags[i] - 1;
            kept             = uint64_t(first[u + 1] - first[u]) < threshold ? 1u : 0u;
        }
        keep[i] = kept;
    }
}

__global__ void compact_kernel(uint64_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ dst,
                               const uint64_t* __restrict__ rep_in, const uint32_t* __restrict__ read_in,
                               const uint32_t* __restrict__ pos_in, const uint8_t* __restrict__ dir_in,
                               uint64_t* __restrict__ rep_out, uint32_t* __restrict__ read_out,
                               uint32_t* __restrict__ pos_out, uint8_t* __restrict__ dir_out)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kThreads)
    {
        if (!keep[i])
            continue;
        const uint32_t d = dst[i];
        rep_out[d]       = rep_in[i];
        read_out[d]      = read_in[i];
        pos_out[d]       = pos_in[i];
        dir_out[d]       = dir_in[i];
    }
}

template <typename T>
void upload(DevBuf<T>& d, const std::vector<T>& h, const Budget& budget, hipStream_t stream)
{
    d.alloc(h.size(), budget);
    if (!h.empty())
        GWAMD_HIP_CHECK(hipMemcpyAsync(d.data(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
}

// unique representations and first occurrences of n > 0 sorted elements;
// flags and index (n + 1 entries each) are left for the filter
void find_first_occurrences(IndexData& out, uint64_t n, DevBuf<uint32_t>& flags, DevBuf<uint32_t>& index,
                            const Budget& budget, hipStream_t stream)
{
    flags.alloc(n + 1, budget);
    index.alloc(n + 1, budget);
    head_flag_kernel<<<blocks_for(n + 1), kThreads, 0, stream>>>(out.representations.data(), n, flags.data());
    check_launch();
    exclusive_sum(flags.data(), index.data(), n + 1, budget, stream);
    const uint32_t num_unique = read_back(index.data() + n, stream);
    out.unique_representations.alloc(num_unique, budget);
    out.first_occurrence_of_representations.alloc(size_t(num_unique) + 1, budget);
    first_occurrence_kernel<<<blocks_for(n), kThreads, 0, stream>>>(
        out.representations.data(), n, flags.data(), index.data(), num_unique, out.unique_representations.data(),
        out.first_occurrence_of_representations.data());
    check_launch();
}

void clear_arrays(IndexData& out)
{
    out.representations.free();
    out.read_ids.free();
    out.positions_in_reads.free();
    out.directions_of_reads.free();
    out.unique_representations.free();
    out.first_occurrence_of_representations.free();
}

} // namespace

void build_index(IndexData& out, const char* bases, const int64_t* offsets, uint32_t first_read_id, uint32_t num_reads,
                 int k, int w, bool hash_representations, double filtering_parameter, const Budget& budget,
                 hipStream_t stream)
{
    clear_arrays(out);
    out.number_of_reads = out.smallest_read_id = out.largest_read_id = out.number_of_basepairs_in_longest_read = 0;

    // tiles of the reads that hold at least one full window
    std::vector<uint64_t> read_start(num_reads);
    std::vector<uint32_t> read_length(num_reads);
    std::vector<uint32_t> tile_read, tile_first_window;
    uint32_t longest = 0;
    for (uint32_t r = 0; r < num_reads; r++)
    {
        const int64_t len = offsets[r + 1] - offsets[r];
        read_start[r]     = uint64_t(offsets[r] - offsets[0]);
        read_length[r]    = uint32_t(len);
        if (len < int64_t(w) + k - 1)
            continue;
        longest               = std::max(longest, uint32_t(len));
        const int64_t windows = len - k + w; // K + w - 1
        for (int64_t j = 0; j < windows; j += kTile)
        {
            tile_read.push_back(r);
            tile_first_window.push_back(uint32_t(j));
        }
    }
    if (tile_read.empty())
        return; // no read long enough: the empty index
    if (tile_read.size() > size_t(INT32_MAX))
        throw std::runtime_error("too many bases for one index");

    const uint32_t num_tiles = uint32_t(tile_read.size());
    uint64_t n               = 0;
    DevBuf<uint64_t> values_sorted;
    {
        const size_t total_bases = size_t(offsets[num_reads] - offsets[0]);
        DevBuf<char> d_bases(total_bases, budget);
        GWAMD_HIP_CHECK(
            hipMemcpyAsync(d_bases.data(), bases + offsets[0], total_bases, hipMemcpyHostToDevice, stream));
        DevBuf<uint64_t> d_start;
        DevBuf<uint32_t> d_length, d_tile_read, d_tile_first;
        upload(d_start, read_start, budget, stream);
        upload(d_length, read_length, budget, stream);
        upload(d_tile_read, tile_read, budget, stream);
        upload(d_tile_first, tile_first_window, budget, stream);

        DevBuf<uint64_t> counts(size_t(num_tiles) + 1, budget), tile_offset(size_t(num_tiles) + 1, budget);
        GWAMD_HIP_CHECK(hipMemsetAsync(counts.data() + num_tiles, 0, sizeof(uint64_t), stream));
        sketch_kernel<false><<<num_tiles, kThreads, 0, stream>>>(
            d_bases.data(), d_start.data(), d_length.data(), d_tile_read.data(), d_tile_first.data(), k, w,
            hash_representations ? 1 : 0, first_read_id, counts.data(), nullptr, nullptr, nullptr);
        check_launch();
        exclusive_sum(counts.data(), tile_offset.data(), size_t(num_tiles) + 1, budget, stream);
        n = read_back(tile_offset.data() + num_tiles, stream);
        // first_occurrence_of_representations is 32 bits wide
        if (n >= (uint64_t(1) << 32))
            throw std::runtime_error("index would hold " + std::to_string(n) +
                                     " sketch elements; fewer than 2^32 fit one index");

        DevBuf<uint64_t> keys(n, budget), values(n, budget);
        sketch_kernel<true><<<num_tiles, kThreads, 0, stream>>>(
            d_bases.data(), d_start.data(), d_length.data(), d_tile_read.data(), d_tile_first.data(), k, w,
            hash_representations ? 1 : 0, first_read_id, nullptr, tile_offset.data(), keys.data(), values.data());
        check_launch();
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream)); // the host vectors were read asynchronously
        d_bases.free();

        out.representations.alloc(n, budget);
        values_sorted.alloc(n, budget);
        // hashed representations are 32 bits wide, plain ones 2k bits
        const int key_bits = hash_representations ? 32 : 2 * k;
        sort_pairs(keys.data(), out.representations.data(), values.data(), values_sorted.data(), n, key_bits, budget,
                   stream);
    }

    out.read_ids.alloc(n, budget);
    out.positions_in_reads.alloc(n, budget);
    out.directions_of_reads.alloc(n, budget);
    unpack_kernel<<<blocks_for(n), kThreads, 0, stream>>>(values_sorted.data(), n, out.read_ids.data(),
                                                          out.positions_in_reads.data(),
                                                          out.directions_of_reads.data());
    check_launch();
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    values_sorted.free();

    DevBuf<uint32_t> flags, index;
    find_first_occurrences(out, n, flags, index, budget, stream);

    if (filtering_parameter < 1.0)
    {
        // index_gpu.cuh:420-422
        const uint64_t threshold = uint64_t(double(n) * filtering_parameter + 0.001);
        DevBuf<uint32_t> keep(n + 1, budget), dst(n + 1, budget);
        keep_flag_kernel<<<blocks_for(n + 1), kThreads, 0, stream>>>(
            n, flags.data(), index.data(), out.first_occurrence_of_representations.data(), threshold, keep.data());
        check_launch();
        exclusive_sum(keep.data(), dst.data(), n + 1, budget, stream);
        const uint32_t kept = read_back(dst.data() + n, stream);
        if (kept != n)
        {
            IndexData f;
            f.representations.alloc(kept, budget);
            f.read_ids.alloc(kept, budget);
            f.positions_in_reads.alloc(kept, budget);
            f.directions_of_reads.alloc(kept, budget);
            if (kept > 0)
            {
                compact_kernel<<<blocks_for(n), kThreads, 0, stream>>>(
                    n, keep.data(), dst.data(), out.representations.data(), out.read_ids.data(),
                    out.positions_in_reads.data(), out.directions_of_reads.data(), f.representations.data(),
                    f.read_ids.data(), f.positions_in_reads.data(), f.directions_of_reads.data());
                check_launch();
                find_first_occurrences(f, kept, flags, index, budget, stream);
            }
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
            out.representations                     = std::move(f.representations);
            out.read_ids                            = std::move(f.read_ids);
            out.positions_in_reads                  = std::move(f.positions_in_reads);
            out.directions_of_reads                 = std::move(f.directions_of_reads);
            out.unique_representations              = std::move(f.unique_representations);
            out.first_occurrence_of_representations = std::move(f.first_occurrence_of_representations);
        }
    }
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));

    out.number_of_reads                     = num_reads;
    out.smallest_read_id                    = first_read_id;
    out.largest_read_id                     = first_read_id + num_reads - 1;
    out.number_of_basepairs_in_longest_read = longest;
}

} // namespace mapper
} // namespace gwamd
