// Host side of cudapolish (include/gwamd_polish.h,
// claraparabricks/genomeworks/cudapolish/windows.hpp): the argument checks, the
// layout of the records, the walk of one path on the host, the completion of
// the records the kernel leaves (polish_windows.hip), the one launch of the
// cut (cut_launch) for paths from the host, for the aligner's device paths
// (window_segments_resident, on the engines of overlap_engines.hpp) and for
// CIGAR ops (cut_cigars, polish_cigar.hip; walk_cigar_on_host), the grouping
// into cudapoa groups on the host (group_slices) and on the device
// (group_segments_on_device, slices_resident; polish_group.hip) and the C ABI.  Every argument is checked here, before any
// device call, so that the kernel is never given an overlap with start > end or
// a record range it does not own.
//
// Who completes a record: the kernel stores q_begin, q_end, t_begin, t_end of
// the windows that hold a match or mismatch state into records the host has
// zeroed, and one status word per overlap; complete_records, on the host after
// the copy back, writes overlap, window, flags and the reserved word of every
// record.
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include "allocator_handle.hpp"
#include "mapper_capi.hpp"
#include "mapper_reads.hpp"
#include "overlap_engines.hpp"
#include "polish_group.hpp"
#include "polish_windows.hpp"

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gm = gwamd::mapper;
namespace gp = gwamd::polish;
namespace gw = claraparabricks::genomeworks;

static_assert(sizeof(gw::cudapolish::WindowSegment) == sizeof(gwamd_window_segment) &&
                  sizeof(gwamd_window_segment) == 32,
              "a record is eight 32-bit words");
static_assert(sizeof(gw::cudaaligner::AlignmentState) == 1, "states are bytes");

// (gwamd_window_slices, the handle of all three grouping routes: polish_group.hpp)

// the slices with their bases copied out of the host's reads
struct gwamd_windows
{
    std::vector<char> bases;
    std::vector<int64_t> sequence_offsets{0};
    gwamd_window_slices grouped;
};

namespace gwamd
{
namespace polish
{

namespace
{

uint32_t records_of(const OverlapRecord& o, uint32_t w)
{
    return o.target_end == o.target_start ? 0 : (o.target_end - 1) / w - o.target_start / w + 1;
}

} // namespace

RecordLayout plan_records(const OverlapRecord* overlaps, int64_t n, int32_t window_length)
{
    if (window_length <= 0)
        throw std::invalid_argument("window_length must be positive, got " + std::to_string(window_length));
    RecordLayout layout;
    layout.base.assign(size_t(n) + 1, 0);
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++)
    {
        total += records_of(overlaps[i], uint32_t(window_length));
        if (total >= (int64_t(1) << 31))
            throw std::invalid_argument("more than 2^31 window records in one call");
        layout.base[size_t(i) + 1] = uint32_t(total);
    }
    return layout;
}

void complete_records(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                      int32_t window_length, uint32_t flag)
{
    const uint32_t k0      = overlap.target_start / uint32_t(window_length);
    const uint32_t reverse = overlap.relative_strand == '-' ? GWAMD_SEGMENT_REVERSE : 0;
    for (uint32_t j = 0; j < count; j++)
    {
        gwamd_window_segment& r = records[j];
        r.overlap               = index;
        r.window                = k0 + j;
        r.reserved              = 0;
        r.flags                 = reverse;
        // (a window with a match or mismatch state has q_end >= 1)
        if (flag != 0 || r.q_end == 0)
        {
            r.q_begin = r.q_end = r.t_begin = r.t_end = 0;
            r.flags |= GWAMD_SEGMENT_EMPTY | flag;
        }
    }
}

void walk_on_host(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                  const int8_t* states, int64_t num_states, int32_t window_length)
{
    const uint32_t w = uint32_t(window_length);
    const uint32_t span_t = overlap.target_end - overlap.target_start;
    const uint32_t span_q = overlap.query_end - overlap.query_start;
    const bool reverse    = overlap.relative_strand == '-';
    const uint32_t k0     = overlap.target_start / w;
    std::memset(static_cast<void*>(records), 0, size_t(count) * sizeof(gwamd_window_segment));
    uint32_t u = 0, v = 0;
    bool fits = true;
    uint32_t open = UINT32_MAX; // the window of the last match state
    for (int64_t p = 0; p < num_states && fits; p++)
    {
        const int8_t s = states[p];
        if (s < 0 || s > 3)
            fits = false;
        else if (s <= 1)
        {
            if (u >= span_t || v >= span_q)
                fits = false;
            else
            {
                const uint32_t t = reverse ? overlap.target_end - 1 - u : overlap.target_start + u;
                const uint32_t q = overlap.query_start + v;
                gwamd_window_segment& r = records[t / w - k0];
                if (t / w != open)
                {
                    open      = t / w;
                    r.q_begin = q;
                    (reverse ? r.t_end : r.t_begin) = reverse ? t + 1 : t;
                }
                r.q_end = q + 1;
                (reverse ? r.t_begin : r.t_end) = reverse ? t : t + 1;
            }
        }
        if (fits)
        {
            u += s != 3;
            v += s != 2;
        }
    }
    fits = fits && u == span_t && v == span_q;
    complete_records(records, count, index, overlap, window_length, fits ? 0 : GWAMD_SEGMENT_BAD_PATH);
}

void walk_cigar_on_host(gwamd_window_segment* records, uint32_t count, uint32_t index, const OverlapRecord& overlap,
                        const uint32_t* ops, int64_t num_ops, bool sam, int32_t window_length)
{
    const int64_t w      = window_length;
    const int64_t span_t = int64_t(overlap.target_end) - int64_t(overlap.target_start);
    const int64_t span_q = int64_t(overlap.query_end) - int64_t(overlap.query_start);
    const bool reverse   = overlap.relative_strand == '-';
    const int64_t k0     = overlap.target_start / w;
    std::memset(static_cast<void*>(records), 0, size_t(count) * sizeof(gwamd_window_segment));
    int64_t u = 0, v = 0; // at most num_ops * 2^28: no wrap
    bool fits = true;
    int64_t open = -1; // the window of the last match state
    for (int64_t j = 0; j < num_ops && fits; j++)
    {
        const uint32_t op    = normalised_op(ops, num_ops, j, sam, reverse);
        const uint32_t code  = op & 15;
        const int64_t length = op >> 4;
        const bool match     = code == 0 || code == 7 || code == 8;
        if (!match && code != 1 && code != 2)
            fits = false;
        else if (match && length > 0)
        {
            if (u + length > span_t || v + length > span_q)
                fits = false;
            else
            {
                // the run's first and last target position, and the windows between them in path order
                const int64_t t0 = reverse ? int64_t(overlap.target_end) - 1 - u : int64_t(overlap.target_start) + u;
                const int64_t t1 = reverse ? t0 - (length - 1) : t0 + (length - 1);
                const int64_t q0 = int64_t(overlap.query_start) + v;
                const int64_t step = reverse ? -1 : 1;
                for (int64_t k = t0 / w; k != t1 / w + step; k += step)
                {
                    const int64_t lo = std::max(std::min(t0, t1), k * w);
                    const int64_t hi = std::min(std::max(t0, t1), (k + 1) * w - 1);
                    gwamd_window_segment& r = records[k - k0];
                    if (k != open)
                    {
                        open      = k;
                        r.q_begin = uint32_t(q0 + (reverse ? t0 - hi : lo - t0));
                        (reverse ? r.t_end : r.t_begin) = uint32_t(reverse ? hi + 1 : lo);
                    }
                    r.q_end = uint32_t(q0 + (reverse ? t0 - lo : hi - t0) + 1);
                    (reverse ? r.t_begin : r.t_end) = uint32_t(reverse ? lo : hi + 1);
                }
            }
        }
        if (fits)
        {
            u += code != 2 ? length : 0;
            v += code != 1 ? length : 0;
        }
    }
    fits = fits && u == span_t && v == span_q;
    complete_records(records, count, index, overlap, window_length, fits ? 0 : GWAMD_SEGMENT_BAD_PATH);
}

namespace
{

// what every entry point asks of its overlaps before anything else
// (there are no reads to check them against; positions of 2^31 or more are refused here only)
template <typename T>
void check_cut_overlaps(const T* overlaps, int64_t n, std::vector<OverlapRecord>& records)
{
    gm::check_overlap_count(overlaps, n);
    records = gm::to_records(overlaps, n);
    for (int64_t i = 0; i < n; i++)
    {
        const OverlapRecord& o = records[size_t(i)];
        if (o.query_start > o.query_end || o.target_start > o.target_end)
            throw std::invalid_argument("overlap " + std::to_string(i) + ": positions are not start <= end");
        if (o.query_end >= (1u << 31) || o.target_end >= (1u << 31))
            throw std::invalid_argument("overlap " + std::to_string(i) + ": a position of 2^31 or more");
        if (o.relative_strand != '+' && o.relative_strand != '-')
            throw std::invalid_argument("overlap " + std::to_string(i) + ": relative_strand is neither '+' nor '-'");
    }
}

void check_path_length(const OverlapRecord& o, int64_t i, int64_t length)
{
    if (length < 0)
        throw std::invalid_argument("path " + std::to_string(i) + ": negative length");
    if (length > int64_t(o.query_end - o.query_start) + int64_t(o.target_end - o.target_start))
        throw std::invalid_argument("path " + std::to_string(i) + " is longer than its overlap's two spans together");
}

void clear_outputs(gwamd_window_segment** out, int64_t* num_out)
{
    if (out)
        *out = nullptr;
    if (num_out)
        *num_out = 0;
}

template <typename T>
void upload(gm::DevBuf<T>& d, const T* src, size_t count, const Budget& budget, hipStream_t stream)
{
    d.alloc(count, budget);
    if (count > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(d.data(), src, count * sizeof(T), hipMemcpyHostToDevice, stream));
}

// The records of one launch, completed, where `layout` puts them, and what
// the kernel said of each overlap's path (0 or 1, it does not fit)
struct CutRecords
{
    RecordLayout layout;
    std::vector<gwamd_window_segment> records;
    std::vector<uint32_t> status;
};

// the kernel of a source: on state paths or on CIGAR ops
inline void launch_cut(const PathSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                       gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                       hipStream_t stream)
{
    launch_window_cut(source, d_overlaps, d_record_base, d_records, d_status, n, window_length, stream);
}

inline void launch_cut(const CigarSource& source, const OverlapRecord* d_overlaps, const uint32_t* d_record_base,
                       gwamd_window_segment* d_records, uint32_t* d_status, int64_t n, int32_t window_length,
                       hipStream_t stream)
{
    launch_window_cut_cigar(source, d_overlaps, d_record_base, d_records, d_status, n, window_length, stream);
}

// what the cut's kernel reads besides its source: held until the stream has been synchronized
struct CutInputs
{
    gm::DevBuf<OverlapRecord> overlaps;
    gm::DevBuf<uint32_t> base;
};

// The one launch of the cut: n > 0 checked overlaps in host memory whose paths
// or CIGAR ops `source` names on the device.  The overlaps and base[0, n), the
// index of each one's first record in d_records, go up and the kernel runs on
// stream: it writes the records, which the caller has zeroed, and d_status[0, n).
// Asynchronous; records and status stay on the device.
template <typename Source>
void cut_to_device(const Source& source, const OverlapRecord* overlaps, int64_t n, const uint32_t* base,
                   gwamd_window_segment* d_records, uint32_t* d_status, int32_t window_length, const Budget& budget,
                   hipStream_t stream, CutInputs& held)
{
    upload(held.overlaps, overlaps, size_t(n), budget, stream);
    upload(held.base, base, size_t(n), budget, stream);
    launch_cut(source, held.overlaps.data(), held.base.data(), d_records, d_status, n, window_length, stream);
}

// cut_to_device for a caller that wants the records on the host: they are
// zeroed on the device, cut, and come back with the status, and
// complete_records writes the rest; the records of overlap i carry index[i]
// (null: i).  Returns after the stream has been synchronized.
template <typename Source>
CutRecords cut_launch(const Source& source, const OverlapRecord* overlaps, int64_t n, const int32_t* index,
                      int32_t window_length, const Budget& budget, hipStream_t stream)
{
    CutRecords out;
    out.layout = plan_records(overlaps, n, window_length);
    out.records.assign(size_t(out.layout.total()), gwamd_window_segment{});
    out.status.assign(size_t(n), 0);
    const std::vector<uint32_t>& base = out.layout.base;
    CutInputs held;
    gm::DevBuf<uint32_t> d_status(size_t(n), budget);
    gm::DevBuf<gwamd_window_segment> d_records(std::max<size_t>(out.records.size(), 1), budget);
    GWAMD_HIP_CHECK(hipMemsetAsync(d_records.data(), 0, d_records.size() * sizeof(gwamd_window_segment), stream));
    cut_to_device(source, overlaps, n, base.data(), d_records.data(), d_status.data(), window_length, budget, stream,
                  held);
    if (!out.records.empty())
        GWAMD_HIP_CHECK(hipMemcpyAsync(out.records.data(), d_records.data(),
                                       out.records.size() * sizeof(gwamd_window_segment), hipMemcpyDeviceToHost,
                                       stream));
    GWAMD_HIP_CHECK(hipMemcpyAsync(out.status.data(), d_status.data(), size_t(n) * sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    for (int64_t i = 0; i < n; i++)
        complete_records(out.records.data() + base[size_t(i)], base[size_t(i) + 1] - base[size_t(i)],
                         index ? uint32_t(index[i]) : uint32_t(i), overlaps[i], window_length,
                         out.status[size_t(i)] ? GWAMD_SEGMENT_BAD_PATH : 0);
    return out;
}

// One launch over checked overlaps whose paths are in host memory: `bytes`
// bytes of path buffer (a multiple of 4), path i at offsets[i] or i * stride.
void cut_on_device(const std::vector<OverlapRecord>& overlaps, const int8_t* paths, int64_t bytes,
                   const std::vector<int64_t>* offsets, int64_t stride, const std::vector<int32_t>& lengths,
                   int32_t max_length, bool end_to_start, int32_t window_length, const Budget& budget,
                   std::vector<gwamd_window_segment>& out)
{
    const size_t n = overlaps.size();
    gm::DevBuf<int8_t> d_paths(size_t(std::max<int64_t>(bytes, 16)), budget);
    gm::DevBuf<int64_t> d_offsets;
    gm::DevBuf<int32_t> d_lengths;
    if (bytes > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_paths.data(), paths, size_t(bytes), hipMemcpyHostToDevice, nullptr));
    if (offsets)
        upload(d_offsets, offsets->data(), n, budget, nullptr);
    upload(d_lengths, lengths.data(), n, budget, nullptr);
    PathSource source;
    source.paths        = d_paths.data();
    source.paths_bytes  = bytes;
    source.offsets      = offsets ? d_offsets.data() : nullptr;
    source.stride       = stride;
    source.lengths      = d_lengths.data();
    source.max_length   = max_length;
    source.end_to_start = end_to_start;
    out = cut_launch(source, overlaps.data(), int64_t(n), nullptr, window_length, budget, nullptr).records;
}

// The cut of host paths (start -> end): each path is packed on a 16-byte
// boundary of a buffer padded to a multiple of 16.
void cut_host_paths(const std::vector<OverlapRecord>& overlaps, const int8_t* states, const int64_t* state_offsets,
                    int32_t window_length, const Budget& budget, std::vector<gwamd_window_segment>& out)
{
    const size_t n = overlaps.size();
    std::vector<int64_t> offsets(n);
    std::vector<int32_t> lengths(n);
    int64_t bytes = 0;
    for (size_t i = 0; i < n; i++)
    {
        offsets[i] = bytes;
        lengths[i] = int32_t(state_offsets[i + 1] - state_offsets[i]);
        bytes += (int64_t(lengths[i]) + 15) / 16 * 16;
    }
    std::vector<int8_t> packed(static_cast<size_t>(bytes), 0);
    for (size_t i = 0; i < n; i++)
        if (lengths[i] > 0)
            std::memcpy(packed.data() + offsets[i], states + state_offsets[i], size_t(lengths[i]));
    cut_on_device(overlaps, packed.data(), bytes, &offsets, 0, lengths, INT32_MAX, false, window_length, budget, out);
}

void check_states(const std::vector<OverlapRecord>& overlaps, const int8_t* states, const int64_t* state_offsets)
{
    const int64_t n = int64_t(overlaps.size());
    if (n > 0 && !state_offsets)
        throw std::invalid_argument("state_offsets is NULL");
    for (int64_t i = 0; i < n; i++)
    {
        if (state_offsets[i] < 0 || state_offsets[i] > state_offsets[i + 1])
            throw std::invalid_argument("state_offsets must be non-decreasing");
        check_path_length(overlaps[size_t(i)], i, state_offsets[i + 1] - state_offsets[i]);
    }
    if (n > 0 && state_offsets[n] > 0 && !states)
        throw std::invalid_argument("states is NULL");
}

bool is_sam(int32_t convention)
{
    if (convention != GWAMD_CIGAR_GENOMEWORKS && convention != GWAMD_CIGAR_SAM)
        throw std::invalid_argument("convention must be GWAMD_CIGAR_GENOMEWORKS or GWAMD_CIGAR_SAM, got " +
                                    std::to_string(convention));
    return convention == GWAMD_CIGAR_SAM;
}

void check_cigars(int64_t n, const uint32_t* ops, const int64_t* op_offsets)
{
    if (n > 0 && !op_offsets)
        throw std::invalid_argument("op_offsets is NULL");
    for (int64_t i = 0; i < n; i++)
        if (op_offsets[i] < 0 || op_offsets[i] > op_offsets[i + 1])
            throw std::invalid_argument("op_offsets must be non-decreasing");
    if (n > 0 && op_offsets[n] > op_offsets[0] && !ops)
        throw std::invalid_argument("ops is NULL");
}

// The CIGAR ops of checked overlaps on the device, and the source that names them
struct DeviceCigars
{
    gm::DevBuf<uint32_t> ops;
    gm::DevBuf<int64_t> offsets;
    CigarSource source;
};

// The ops [op_offsets[0], op_offsets[n]) go up as they are, or normalised in
// one pass when they are SAM's; no run is expanded.
void upload_cigars(const std::vector<OverlapRecord>& overlaps, const uint32_t* ops, const int64_t* op_offsets, bool sam,
                   const Budget& budget, DeviceCigars& up)
{
    const size_t n      = overlaps.size();
    const int64_t first = op_offsets[0], total = op_offsets[n] - first;
    std::vector<int64_t> offsets(n + 1);
    for (size_t i = 0; i <= n; i++)
        offsets[i] = op_offsets[i] - first;
    std::vector<uint32_t> normalised;
    if (sam)
    {
        normalised.resize(size_t(total));
        for (size_t i = 0; i < n; i++)
        {
            const int64_t count = offsets[i + 1] - offsets[i];
            for (int64_t j = 0; j < count; j++)
                normalised[size_t(offsets[i] + j)] = normalised_op(ops + first + offsets[i], count, j, true,
                                                                   overlaps[i].relative_strand == '-');
        }
    }
    up.ops.alloc(size_t(std::max<int64_t>(total, 1)), budget);
    if (total > 0)
        GWAMD_HIP_CHECK(hipMemcpyAsync(up.ops.data(), sam ? normalised.data() : ops + first,
                                       size_t(total) * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    upload(up.offsets, offsets.data(), n + 1, budget, nullptr);
    GWAMD_HIP_CHECK(hipStreamSynchronize(nullptr)); // the copies have read this function's arrays
    up.source.ops     = up.ops.data();
    up.source.num_ops = total;
    up.source.offsets = up.offsets.data();
}

// The cut of checked overlaps from their CIGAR ops in host memory
void cut_cigars(const std::vector<OverlapRecord>& overlaps, const uint32_t* ops, const int64_t* op_offsets, bool sam,
                int32_t window_length, const Budget& budget, std::vector<gwamd_window_segment>& out)
{
    DeviceCigars up;
    upload_cigars(overlaps, ops, op_offsets, sam, budget, up);
    out = cut_launch(up.source, overlaps.data(), int64_t(overlaps.size()), nullptr, window_length, budget, nullptr)
              .records;
}

} // namespace

void window_segments_resident(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target,
                              const OverlapRecord* overlaps, int32_t n, int32_t window_length,
                              int32_t num_alignment_engines, std::vector<gwamd_window_segment>& out)
{
    namespace ga              = gwamd::aln;
    const RecordLayout layout = plan_records(overlaps, n, window_length);
    out.assign(size_t(layout.total()), gwamd_window_segment{});
    const ga::ResidentOverlaps pairs(overlaps, n);
    // After the align_all() of the kept overlaps [start, end): the cut runs on
    // the aligner's stream over its device paths, and the records of the range
    // go to the places the layout of the whole call gives them.
    const ga::RangeFn cut = [&](claraparabricks::genomeworks::cudaaligner::Aligner& aligner, int32_t start,
                                int32_t end) {
        const ga::DevicePaths p = ga::device_paths(aligner);
        PathSource source;
        source.paths        = p.paths;
        source.paths_bytes  = p.bytes;
        source.stride       = p.max_path_length;
        source.lengths      = p.lengths;
        source.max_length   = p.max_path_length;
        source.end_to_start = true;
        const CutRecords batch = cut_launch(source, pairs.kept_records.data() + start, end - start,
                                            pairs.kept.data() + start, window_length, nullptr, p.stream);
        for (int32_t k = 0; k < end - start; k++)
        {
            const uint32_t from = batch.layout.base[size_t(k)], count = batch.layout.base[size_t(k) + 1] - from;
            if (count > 0)
                std::memcpy(static_cast<void*>(out.data() + layout.base[size_t(pairs.kept[size_t(start + k)])]),
                            batch.records.data() + from, size_t(count) * sizeof(gwamd_window_segment));
        }
    };
    ga::run_engines(pairs.lengths, pairs.kept, num_alignment_engines, {pairs.add(query, target), cut, true});
    // the overlaps the aligner's limits left out
    std::vector<bool> aligned(static_cast<size_t>(n), false);
    for (int32_t i : pairs.kept)
        aligned[size_t(i)] = true;
    for (int32_t i = 0; i < n; i++)
        if (!aligned[size_t(i)])
            complete_records(out.data() + layout.base[size_t(i)], layout.base[size_t(i) + 1] - layout.base[size_t(i)],
                             uint32_t(i), overlaps[i], window_length, GWAMD_SEGMENT_NOT_ALIGNED);
}

} // namespace polish
} // namespace gwamd

// ---- grouping ---------------------------------------------------------------

namespace
{

char complement(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

// What the host and the device grouping ask of their scalar arguments
void check_grouping(const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
                    int32_t max_sequences_per_window)
{
    if (window_length <= 0)
        throw std::invalid_argument("window_length must be positive, got " + std::to_string(window_length));
    if (max_sequences_per_window < 1)
        throw std::invalid_argument("max_sequences_per_window must be at least 1");
    if (num_segments < 0 || (num_segments > 0 && !segments))
        throw std::invalid_argument("segments: bad count or NULL");
}

// first[r]: the global index of target r's first window; first[num_reads]: the number of windows
std::vector<int64_t> first_windows(const gm::ReadSet& targets, int64_t w)
{
    std::vector<int64_t> first(size_t(targets.num_reads) + 1, 0);
    for (int64_t r = 0; r < targets.num_reads; r++)
        first[size_t(r) + 1] = first[size_t(r)] + (targets.offsets[r + 1] - targets.offsets[r] + w - 1) / w;
    return first;
}

// Whether segment s counts, before the quality filter and the cap: it is not
// flagged and passes the 2 % rule.  Throws std::invalid_argument for a segment
// whose overlap index, read ids, window or (unless it is flagged) query range
// are out of bounds.
bool segment_counts(int64_t s, const gwamd_window_segment& seg, const std::vector<gm::OverlapRecord>& overlaps,
                    const gm::ReadSet& targets, const gm::ReadSet& queries, const std::vector<int64_t>& first,
                    int64_t w)
{
    const std::string which = "segment " + std::to_string(s);
    if (seg.overlap >= overlaps.size())
        throw std::invalid_argument(which + ": overlap index beyond the overlaps");
    const gm::OverlapRecord& o = overlaps[seg.overlap];
    if (int64_t(o.query_read_id) >= queries.num_reads || int64_t(o.target_read_id) >= targets.num_reads)
        throw std::invalid_argument(which + ": read id of its overlap beyond the reads");
    if (int64_t(seg.window) >= first[size_t(o.target_read_id) + 1] - first[o.target_read_id])
        throw std::invalid_argument(which + ": window beyond the target's windows");
    if (seg.flags & (GWAMD_SEGMENT_EMPTY | GWAMD_SEGMENT_BAD_PATH | GWAMD_SEGMENT_NOT_ALIGNED))
        return false;
    if (seg.q_begin > seg.q_end ||
        int64_t(seg.q_end) > queries.offsets[o.query_read_id + 1] - queries.offsets[o.query_read_id])
        throw std::invalid_argument(which + ": query range outside its read");
    return (int64_t(seg.q_end) - int64_t(seg.q_begin)) * 50 >= w;
}

// The grouping: which slices of the targets (set 0) and queries (set 1) make
// up which window.  Only offsets are looked at, and the queries' quality
// characters when they are given (racon's mean-quality rule, gwamd_polish.h).
std::unique_ptr<gwamd_window_slices> group_slices(const gm::ReadSet& targets, const gm::ReadSet& queries,
                                                  const char* query_qualities, int32_t quality_threshold_tenths,
                                                  const std::vector<gm::OverlapRecord>& overlaps,
                                                  const gwamd_window_segment* segments, int64_t num_segments,
                                                  int32_t window_length, int32_t max_sequences_per_window)
{
    check_grouping(segments, num_segments, window_length, max_sequences_per_window);
    if (query_qualities && quality_threshold_tenths < 0)
        throw std::invalid_argument("quality_threshold_tenths must not be negative");
    const int64_t w = window_length;
    // the windows of every target, and the kept segments of each in the order given
    const std::vector<int64_t> first = first_windows(targets, w);
    const int64_t num_windows        = first[size_t(targets.num_reads)];
    std::vector<std::vector<int64_t>> kept(static_cast<size_t>(num_windows));
    auto out = std::make_unique<gwamd_window_slices>();
    for (int64_t s = 0; s < num_segments; s++)
    {
        const gwamd_window_segment& seg = segments[s];
        if (!segment_counts(s, seg, overlaps, targets, queries, first, w))
            continue;
        const gm::OverlapRecord& o = overlaps[seg.overlap];
        if (query_qualities)
        {
            const char* q = query_qualities + queries.offsets[o.query_read_id];
            int64_t sum   = 0;
            for (uint32_t j = seg.q_begin; j < seg.q_end; j++)
                sum += int64_t(uint8_t(q[j])) - 33;
            if (sum * 10 < int64_t(quality_threshold_tenths) * (int64_t(seg.q_end) - int64_t(seg.q_begin)))
            {
                out->dropped_by_quality++;
                continue;
            }
        }
        std::vector<int64_t>& list = kept[size_t(first[o.target_read_id] + seg.window)];
        if (int64_t(list.size()) >= int64_t(max_sequences_per_window) - 1)
            out->dropped_by_cap++;
        else
            list.push_back(s);
    }
    auto add = [&](int32_t set, uint32_t read, int64_t begin, int64_t end, bool reverse, int32_t overlap,
                   int32_t t_begin, int32_t t_end) {
        out->slices.push_back(
            gwamd_read_slice{set, read, uint32_t(begin), uint32_t(end), reverse ? GWAMD_SLICE_REVERSE : 0u});
        out->sequence_overlap.push_back(overlap);
        out->sequence_t_begin.push_back(t_begin);
        out->sequence_t_end.push_back(t_end);
    };
    for (int64_t r = 0; r < targets.num_reads; r++)
    {
        const int64_t length = targets.offsets[r + 1] - targets.offsets[r];
        for (int64_t k = 0; k < first[size_t(r) + 1] - first[size_t(r)]; k++)
        {
            const int64_t from = k * w, to = std::min((k + 1) * w, length);
            add(0, uint32_t(r), from, to, false, -1, 0, int32_t(to - from));
            const std::vector<int64_t>& list = kept[size_t(first[size_t(r)] + k)];
            for (int64_t s : list)
            {
                const gwamd_window_segment& seg = segments[s];
                const gm::OverlapRecord& o      = overlaps[seg.overlap];
                add(1, o.query_read_id, seg.q_begin, seg.q_end, (seg.flags & GWAMD_SEGMENT_REVERSE) != 0,
                    int32_t(seg.overlap), int32_t(int64_t(seg.t_begin) - from), int32_t(int64_t(seg.t_end) - from));
            }
            out->window_counts.push_back(int32_t(list.size()) + 1);
            out->window_target.push_back(uint32_t(r));
            out->window_index.push_back(uint32_t(k));
        }
    }
    return out;
}

// group_slices, and every slice's bases copied out of the host's reads
std::unique_ptr<gwamd_windows> group_windows(const gm::ReadSet& targets, const gm::ReadSet& queries,
                                             const std::vector<gm::OverlapRecord>& overlaps,
                                             const gwamd_window_segment* segments, int64_t num_segments,
                                             int32_t window_length, int32_t max_sequences_per_window)
{
    auto out     = std::make_unique<gwamd_windows>();
    out->grouped = std::move(*group_slices(targets, queries, nullptr, 0, overlaps, segments, num_segments,
                                           window_length, max_sequences_per_window));
    for (const gwamd_read_slice& sl : out->grouped.slices)
    {
        const gm::ReadSet& set = sl.set == 0 ? targets : queries;
        const char* src        = set.bases + set.offsets[sl.read] + sl.begin;
        const int64_t len      = int64_t(sl.end) - int64_t(sl.begin);
        const size_t at        = out->bases.size();
        out->bases.resize(at + size_t(len));
        for (int64_t j = 0; j < len; j++)
            out->bases[at + size_t(j)] = (sl.flags & GWAMD_SLICE_REVERSE) ? complement(src[len - 1 - j]) : src[j];
        out->sequence_offsets.push_back(int64_t(out->bases.size()));
    }
    return out;
}

std::vector<gm::OverlapRecord> as_records(const std::vector<gw::cudamapper::Overlap>& overlaps)
{
    std::vector<gm::OverlapRecord> records;
    gp::check_cut_overlaps(overlaps.data(), int64_t(overlaps.size()), records);
    return records;
}

std::vector<gw::cudapolish::WindowSegment> as_segments(const std::vector<gwamd_window_segment>& records)
{
    std::vector<gw::cudapolish::WindowSegment> out(records.size());
    if (!records.empty())
        std::memcpy(static_cast<void*>(out.data()), records.data(), records.size() * sizeof(gwamd_window_segment));
    return out;
}

// the checks of the resident cut, then the cut
void cut_resident(const gm::DeviceReads& query, const gm::DeviceReads& target,
                  const std::vector<gm::OverlapRecord>& records, int32_t window_length, int32_t num_alignment_engines,
                  std::vector<gwamd_window_segment>& out)
{
    gm::check_overlaps(query, target, records.data(), int64_t(records.size()));
    if (num_alignment_engines < 1)
        throw std::invalid_argument("num_alignment_engines must be at least 1");
    (void)gp::plan_records(records.data(), int64_t(records.size()), window_length);
    out.clear();
    if (records.empty())
        return;
    gm::check_on_current_device(query, target);
    gp::window_segments_resident(query, target, records.data(), int32_t(records.size()), window_length,
                                 num_alignment_engines, out);
}

// ---- grouping on the device (polish_group.hip) ----------------------------------

// first_windows as the kernels read it.  Throws std::invalid_argument for 2^31
// windows or more, and when the windows and `records` records, each of which may
// become a sequence, come to 2^31 or more.
std::vector<uint32_t> device_first_windows(const gm::ReadSet& targets, int64_t w, int64_t records)
{
    const std::vector<int64_t> first = first_windows(targets, w);
    if (first.back() >= (int64_t(1) << 31) || first.back() + records >= (int64_t(1) << 31))
        throw std::invalid_argument("2^31 or more windows or sequences in one call");
    return std::vector<uint32_t>(first.begin(), first.end());
}

// gwamd_build_window_slices_device after the checks of its pointers and read
// sets: the rest of the checks, all of them before the first device call, then
// the given segments go up and are grouped.
std::unique_ptr<gwamd_window_slices> group_segments_on_device(
    const gm::ReadSet& targets, const gm::ReadSet& queries, const gm::DeviceReads* query_reads,
    int32_t quality_threshold_tenths, const std::vector<gm::OverlapRecord>& overlaps,
    const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
    int32_t max_sequences_per_window, int32_t device_id, const gp::Budget& budget, int32_t repeats = 1,
    double* seconds = nullptr)
{
    check_grouping(segments, num_segments, window_length, max_sequences_per_window);
    if (quality_threshold_tenths < 0)
        throw std::invalid_argument("quality_threshold_tenths must not be negative");
    if (query_reads)
    {
        if (device_id >= 0 && query_reads->device_id != device_id)
            throw std::invalid_argument("query_reads is on device " + std::to_string(query_reads->device_id) +
                                        ", the call is for device " + std::to_string(device_id));
        if (query_reads->num_reads() != queries.num_reads ||
            !std::equal(query_reads->offsets.begin(), query_reads->offsets.end(), queries.offsets,
                        [&](int64_t a, int64_t b) { return a == b - queries.offsets[0]; }))
            throw std::invalid_argument("query_reads does not hold the reads of query_offsets");
    }
    const std::vector<uint32_t> first = device_first_windows(targets, window_length, num_segments);
    {
        const std::vector<int64_t> first64(first.begin(), first.end());
        for (int64_t s = 0; s < num_segments; s++)
            (void)segment_counts(s, segments[s], overlaps, targets, queries, first64, window_length);
    }
    auto out = std::make_unique<gwamd_window_slices>();
    if (first.back() == 0)
        return out;
    if (device_id < 0) // the C++ entry: the current device
    {
        GWAMD_HIP_CHECK(hipGetDevice(&device_id));
        if (query_reads && query_reads->device_id != device_id)
            throw std::invalid_argument("query_reads is not on the current device");
    }
    gwamd::host::ScopedDevice dev(device_id);
    const bool filter = query_reads && query_reads->has_qualities;
    gm::DevBuf<gwamd_window_segment> d_records;
    gm::DevBuf<gm::OverlapRecord> d_overlaps;
    gm::DevBuf<int64_t> d_target_offsets;
    gm::DevBuf<uint32_t> d_first;
    gp::upload(d_records, segments, size_t(num_segments), budget, nullptr);
    gp::upload(d_overlaps, overlaps.data(), overlaps.size(), budget, nullptr);
    gp::upload(d_target_offsets, targets.offsets, size_t(targets.num_reads) + 1, budget, nullptr);
    gp::upload(d_first, first.data(), first.size(), budget, nullptr);
    gp::GroupInput in;
    in.records                  = d_records.data();
    in.num_records              = num_segments;
    in.overlaps                 = d_overlaps.data();
    in.num_overlaps             = int64_t(overlaps.size());
    in.target_offsets           = d_target_offsets.data();
    in.window_first             = d_first.data();
    in.num_targets              = targets.num_reads;
    in.num_windows              = int64_t(first.back());
    in.query_offsets            = filter ? query_reads->d_offsets.data() : nullptr;
    in.query_qualities          = filter ? query_reads->qualities() : nullptr;
    in.quality_threshold_tenths = quality_threshold_tenths;
    in.window_length            = window_length;
    in.max_sequences_per_window = max_sequences_per_window;
    // (repeats > 1, seconds: the measurement hook times each grouping of the records that are now resident)
    GWAMD_HIP_CHECK(hipStreamSynchronize(nullptr));
    for (int32_t r = 0; r < repeats; r++)
    {
        const auto begin = std::chrono::steady_clock::now();
        gp::group_on_device(in, *out, budget, nullptr);
        if (seconds)
            seconds[r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    }
    return out;
}

// gwamd_window_slices_resident after the checks of its pointers: the rest of
// the checks, then the cut (of the aligner's device paths, engine range by
// engine range, or of the CIGAR ops) into one device array of records, laid out
// by plan_records over all overlaps, and the grouping of that array.  No record
// comes to the host.
std::unique_ptr<gwamd_window_slices> slices_resident(const gm::DeviceReads& query, const gm::DeviceReads& target,
                                                     const std::vector<gm::OverlapRecord>& overlaps,
                                                     const uint32_t* ops, const int64_t* op_offsets,
                                                     int32_t convention, int32_t window_length,
                                                     int32_t max_sequences_per_window,
                                                     int32_t quality_threshold_tenths, int32_t num_alignment_engines)
{
    namespace ga      = gwamd::aln;
    const int32_t n   = int32_t(overlaps.size());
    const bool cigars = op_offsets != nullptr;
    const bool sam    = cigars && gp::is_sam(convention);
    gm::check_overlaps(query, target, overlaps.data(), n);
    if (cigars)
        gp::check_cigars(n, ops, op_offsets);
    else if (num_alignment_engines < 1)
        throw std::invalid_argument("num_alignment_engines must be at least 1");
    const gp::RecordLayout layout = gp::plan_records(overlaps.data(), n, window_length);
    if (max_sequences_per_window < 1)
        throw std::invalid_argument("max_sequences_per_window must be at least 1");
    if (quality_threshold_tenths < 0)
        throw std::invalid_argument("quality_threshold_tenths must not be negative");
    const gm::ReadSet targets{nullptr, target.offsets.data(), target.num_reads()};
    const std::vector<uint32_t> first = device_first_windows(targets, window_length, layout.total());
    auto out                          = std::make_unique<gwamd_window_slices>();
    if (first.back() == 0)
        return out;
    gm::check_on_current_device(query, target);

    const gp::Budget budget; // the fused entry has no pool to count against
    gm::DevBuf<gwamd_window_segment> d_records(std::max<size_t>(size_t(layout.total()), 1), budget);
    gm::DevBuf<uint32_t> d_status(std::max<size_t>(size_t(n), 1), budget);
    std::vector<uint32_t> slot(size_t(n), gp::kNotAligned); // overlap -> its word of d_status
    GWAMD_HIP_CHECK(hipMemsetAsync(d_records.data(), 0, d_records.size() * sizeof(gwamd_window_segment), nullptr));
    GWAMD_HIP_CHECK(hipStreamSynchronize(nullptr)); // the engines' streams do not wait for the null stream
    if (n > 0 && cigars)
    {
        gp::DeviceCigars up;
        gp::CutInputs held;
        gp::upload_cigars(overlaps, ops, op_offsets, sam, budget, up);
        gp::cut_to_device(up.source, overlaps.data(), n, layout.base.data(), d_records.data(), d_status.data(),
                          window_length, budget, nullptr, held);
        GWAMD_HIP_CHECK(hipStreamSynchronize(nullptr));
        for (int32_t i = 0; i < n; i++)
            slot[size_t(i)] = uint32_t(i);
    }
    else if (n > 0)
    {
        const ga::ResidentOverlaps pairs(overlaps.data(), n);
        for (size_t k = 0; k < pairs.kept.size(); k++)
            slot[size_t(pairs.kept[k])] = uint32_t(k);
        // as window_segments_resident, but the records of the range stay on the
        // device, at the places the layout of the whole call gives them
        const ga::RangeFn cut = [&](claraparabricks::genomeworks::cudaaligner::Aligner& aligner, int32_t start,
                                    int32_t end) {
            const ga::DevicePaths p = ga::device_paths(aligner);
            gp::PathSource source;
            source.paths        = p.paths;
            source.paths_bytes  = p.bytes;
            source.stride       = p.max_path_length;
            source.lengths      = p.lengths;
            source.max_length   = p.max_path_length;
            source.end_to_start = true;
            std::vector<uint32_t> base(size_t(end - start));
            for (int32_t k = 0; k < end - start; k++)
                base[size_t(k)] = layout.base[size_t(pairs.kept[size_t(start + k)])];
            gp::CutInputs held;
            gp::cut_to_device(source, pairs.kept_records.data() + start, end - start, base.data(), d_records.data(),
                              d_status.data() + start, window_length, budget, p.stream, held);
            GWAMD_HIP_CHECK(hipStreamSynchronize(p.stream));
        };
        ga::run_engines(pairs.lengths, pairs.kept, num_alignment_engines, {pairs.add(query, target), cut, true});
    }
    gm::DevBuf<gm::OverlapRecord> d_overlaps;
    gm::DevBuf<uint32_t> d_base, d_slot, d_first;
    gp::upload(d_overlaps, overlaps.data(), size_t(n), budget, nullptr);
    gp::upload(d_base, layout.base.data(), size_t(n) + 1, budget, nullptr);
    gp::upload(d_slot, slot.data(), size_t(n), budget, nullptr);
    gp::upload(d_first, first.data(), first.size(), budget, nullptr);
    gp::GroupInput in;
    in.records                  = d_records.data();
    in.num_records              = layout.total();
    in.overlaps                 = d_overlaps.data();
    in.num_overlaps             = n;
    in.record_base              = d_base.data();
    in.status                   = d_status.data();
    in.status_slot              = d_slot.data();
    in.target_offsets           = target.d_offsets.data();
    in.window_first             = d_first.data();
    in.num_targets              = target.num_reads();
    in.num_windows              = int64_t(first.back());
    in.query_offsets            = query.has_qualities ? query.d_offsets.data() : nullptr;
    in.query_qualities          = query.qualities();
    in.quality_threshold_tenths = quality_threshold_tenths;
    in.window_length            = window_length;
    in.max_sequences_per_window = max_sequences_per_window;
    gp::group_on_device(in, *out, budget, nullptr);
    return out;
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapolish
{

std::vector<WindowSegment> window_segments(DefaultDeviceAllocator allocator,
                                           const std::vector<cudamapper::Overlap>& overlaps,
                                           const std::vector<std::vector<cudaaligner::AlignmentState>>& paths,
                                           int32_t window_length)
{
    if (paths.size() != overlaps.size())
        throw std::invalid_argument("window_segments: one path per overlap expected");
    const std::vector<gm::OverlapRecord> records = as_records(overlaps);
    std::vector<int64_t> offsets(paths.size() + 1, 0);
    for (size_t i = 0; i < paths.size(); i++)
        offsets[i + 1] = offsets[i] + int64_t(paths[i].size());
    std::vector<int8_t> states(static_cast<size_t>(offsets.back()));
    for (size_t i = 0; i < paths.size(); i++)
        if (!paths[i].empty())
            std::memcpy(states.data() + offsets[i], paths[i].data(), paths[i].size());
    gp::check_states(records, states.data(), offsets.data());
    (void)gp::plan_records(records.data(), int64_t(records.size()), window_length);
    std::vector<gwamd_window_segment> out;
    if (!records.empty())
        gp::cut_host_paths(records, states.data(), offsets.data(), window_length, allocator.budget(), out);
    return as_segments(out);
}

std::vector<WindowSegment> window_segments(DefaultDeviceAllocator /*allocator*/,
                                           const std::vector<cudamapper::Overlap>& overlaps,
                                           const cudamapper::DeviceReads& query_reads,
                                           const cudamapper::DeviceReads& target_reads, int32_t window_length,
                                           int32_t num_alignment_engines)
{
    if (overlaps.size() > size_t(INT32_MAX))
        throw std::invalid_argument("too many overlaps for one call");
    std::vector<gwamd_window_segment> out;
    cut_resident(*query_reads.impl().reads, *target_reads.impl().reads, as_records(overlaps), window_length,
                 num_alignment_engines, out);
    return as_segments(out);
}

std::vector<WindowSegment> window_segments_cigar(DefaultDeviceAllocator allocator,
                                                 const std::vector<cudamapper::Overlap>& overlaps,
                                                 const std::vector<std::vector<uint32_t>>& cigars,
                                                 int32_t window_length, CigarConvention convention)
{
    if (cigars.size() != overlaps.size())
        throw std::invalid_argument("window_segments_cigar: one CIGAR per overlap expected");
    const bool sam                               = gp::is_sam(int32_t(convention));
    const std::vector<gm::OverlapRecord> records = as_records(overlaps);
    std::vector<int64_t> offsets(cigars.size() + 1, 0);
    for (size_t i = 0; i < cigars.size(); i++)
        offsets[i + 1] = offsets[i] + int64_t(cigars[i].size());
    std::vector<uint32_t> ops;
    ops.reserve(size_t(offsets.back()));
    for (const std::vector<uint32_t>& c : cigars)
        ops.insert(ops.end(), c.begin(), c.end());
    (void)gp::plan_records(records.data(), int64_t(records.size()), window_length);
    std::vector<gwamd_window_segment> out;
    if (!records.empty())
        gp::cut_cigars(records, ops.data(), offsets.data(), sam, window_length, allocator.budget(), out);
    return as_segments(out);
}

std::vector<WindowSegment> window_segments_cigar_host(const cudamapper::Overlap& overlap,
                                                      const std::vector<uint32_t>& cigar, int32_t window_length,
                                                      CigarConvention convention, uint32_t overlap_index)
{
    const bool sam                               = gp::is_sam(int32_t(convention));
    const std::vector<gm::OverlapRecord> records = as_records({overlap});
    const gp::RecordLayout layout                = gp::plan_records(records.data(), 1, window_length);
    std::vector<gwamd_window_segment> out(static_cast<size_t>(layout.total()));
    gp::walk_cigar_on_host(out.data(), uint32_t(out.size()), overlap_index, records[0], cigar.data(),
                           int64_t(cigar.size()), sam, window_length);
    return as_segments(out);
}

Windows build_windows(const io::FastaParser& targets, const io::FastaParser& queries,
                      const std::vector<cudamapper::Overlap>& overlaps, const std::vector<WindowSegment>& segments,
                      int32_t window_length, int32_t max_sequences_per_window)
{
    const gm::PackedReads t(targets), q(queries);
    const std::unique_ptr<gwamd_windows> h =
        group_windows(t.view(), q.view(), as_records(overlaps),
                      reinterpret_cast<const gwamd_window_segment*>(segments.data()), int64_t(segments.size()),
                      window_length, max_sequences_per_window);
    Windows out;
    const gwamd_window_slices& g = h->grouped;
    out.bases          = std::move(h->bases);
    out.target         = g.window_target;
    out.window         = g.window_index;
    out.dropped_by_cap = g.dropped_by_cap;
    size_t s           = 0;
    for (int32_t count : g.window_counts)
    {
        cudapoa::Group group;
        std::vector<Windows::Sequence> meta;
        for (int32_t j = 0; j < count; j++, s++)
        {
            group.push_back(cudapoa::Entry{out.bases.data() + h->sequence_offsets[s], nullptr,
                                           int32_t(h->sequence_offsets[s + 1] - h->sequence_offsets[s])});
            meta.push_back({g.sequence_overlap[s], g.sequence_t_begin[s], g.sequence_t_end[s]});
        }
        out.groups.push_back(std::move(group));
        out.sequence.push_back(std::move(meta));
    }
    return out;
}

namespace
{

WindowSlices as_window_slices(gwamd_window_slices&& h)
{
    static_assert(sizeof(ReadSlice) == sizeof(gwamd_read_slice), "ReadSlice is gwamd_read_slice");
    WindowSlices out;
    out.slices.resize(h.slices.size());
    if (!h.slices.empty())
        std::memcpy(static_cast<void*>(out.slices.data()), h.slices.data(), h.slices.size() * sizeof(ReadSlice));
    out.window_counts      = std::move(h.window_counts);
    out.window_target      = std::move(h.window_target);
    out.window_index       = std::move(h.window_index);
    out.sequence_overlap   = std::move(h.sequence_overlap);
    out.sequence_t_begin   = std::move(h.sequence_t_begin);
    out.sequence_t_end     = std::move(h.sequence_t_end);
    out.dropped_by_cap     = h.dropped_by_cap;
    out.dropped_by_quality = h.dropped_by_quality;
    return out;
}

} // namespace

WindowSlices build_window_slices_device(DefaultDeviceAllocator allocator, const io::FastaParser& targets,
                                        const io::FastaParser& queries,
                                        const std::vector<cudamapper::Overlap>& overlaps,
                                        const std::vector<WindowSegment>& segments, int32_t window_length,
                                        int32_t max_sequences_per_window, const cudamapper::DeviceReads* query_reads,
                                        int32_t quality_threshold_tenths)
{
    const gm::PackedReads t(targets), q(queries);
    return as_window_slices(std::move(*group_segments_on_device(
        t.view(), q.view(), query_reads ? query_reads->impl().reads.get() : nullptr, quality_threshold_tenths,
        as_records(overlaps), reinterpret_cast<const gwamd_window_segment*>(segments.data()),
        int64_t(segments.size()), window_length, max_sequences_per_window, -1, allocator.budget())));
}

WindowSlices window_slices_resident(const std::vector<cudamapper::Overlap>& overlaps,
                                    const cudamapper::DeviceReads& query_reads,
                                    const cudamapper::DeviceReads& target_reads, int32_t window_length,
                                    int32_t max_sequences_per_window, int32_t quality_threshold_tenths,
                                    int32_t num_alignment_engines, const std::vector<std::vector<uint32_t>>* cigars,
                                    CigarConvention convention)
{
    if (overlaps.size() > size_t(INT32_MAX))
        throw std::invalid_argument("too many overlaps for one call");
    std::vector<int64_t> offsets;
    std::vector<uint32_t> ops;
    if (cigars)
    {
        if (cigars->size() != overlaps.size())
            throw std::invalid_argument("window_slices_resident: one CIGAR per overlap expected");
        offsets.assign(1, 0);
        for (const std::vector<uint32_t>& c : *cigars)
        {
            ops.insert(ops.end(), c.begin(), c.end());
            offsets.push_back(int64_t(ops.size()));
        }
    }
    return as_window_slices(std::move(*slices_resident(
        *query_reads.impl().reads, *target_reads.impl().reads, as_records(overlaps), ops.data(),
        cigars ? offsets.data() : nullptr, int32_t(convention), window_length, max_sequences_per_window,
        quality_threshold_tenths, num_alignment_engines)));
}

} // namespace cudapolish
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

extern "C" {

int32_t gwamd_window_segments(const gwamd_overlap* overlaps, int64_t n, const int8_t* states,
                              const int64_t* state_offsets, int32_t window_length, int32_t device_id,
                              gwamd_device_allocator* allocator_or_null, gwamd_window_segment** out, int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        gp::check_states(records, states, state_offsets);
        (void)gp::plan_records(records.data(), n, window_length);
        if (n == 0)
            return int32_t(0);
        gwamd::host::ScopedDevice dev(device_id);
        std::vector<gwamd_window_segment> result;
        gp::cut_host_paths(records, states, state_offsets, window_length,
                           allocator_or_null ? allocator_or_null->alloc.budget() : nullptr, result);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_window_segments_host(const gwamd_overlap* overlap, const int8_t* states, int64_t num_states,
                                   int32_t window_length, uint32_t overlap_index, gwamd_window_segment** out,
                                   int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (!overlap)
            throw std::invalid_argument("overlap is NULL");
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlap, 1, records);
        gp::check_path_length(records[0], 0, num_states);
        if (num_states > 0 && !states)
            throw std::invalid_argument("states is NULL");
        const gp::RecordLayout layout = gp::plan_records(records.data(), 1, window_length);
        std::vector<gwamd_window_segment> result(static_cast<size_t>(layout.total()));
        gp::walk_on_host(result.data(), uint32_t(result.size()), overlap_index, records[0], states, num_states,
                         window_length);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_window_segments_cigar(const gwamd_overlap* overlaps, int64_t n, const uint32_t* ops,
                                    const int64_t* op_offsets, int32_t convention, int32_t window_length,
                                    int32_t device_id, gwamd_device_allocator* allocator_or_null,
                                    gwamd_window_segment** out, int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        const bool sam = gp::is_sam(convention);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        gp::check_cigars(n, ops, op_offsets);
        (void)gp::plan_records(records.data(), n, window_length);
        if (n == 0)
            return int32_t(0);
        gwamd::host::ScopedDevice dev(device_id);
        std::vector<gwamd_window_segment> result;
        gp::cut_cigars(records, ops, op_offsets, sam, window_length,
                       allocator_or_null ? allocator_or_null->alloc.budget() : nullptr, result);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_window_segments_cigar_host(const gwamd_overlap* overlap, const uint32_t* ops, int64_t num_ops,
                                         int32_t convention, int32_t window_length, uint32_t overlap_index,
                                         gwamd_window_segment** out, int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (!overlap)
            throw std::invalid_argument("overlap is NULL");
        const bool sam = gp::is_sam(convention);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlap, 1, records);
        if (num_ops < 0 || (num_ops > 0 && !ops))
            throw std::invalid_argument("ops: negative count or NULL");
        const gp::RecordLayout layout = gp::plan_records(records.data(), 1, window_length);
        std::vector<gwamd_window_segment> result(static_cast<size_t>(layout.total()));
        gp::walk_cigar_on_host(result.data(), uint32_t(result.size()), overlap_index, records[0], ops, num_ops, sam,
                               window_length);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_window_segments_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                       const gwamd_overlap* overlaps, int32_t n, int32_t window_length,
                                       int32_t num_alignment_engines, gwamd_window_segment** out, int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        if (!query_reads || !target_reads)
            throw std::invalid_argument("query_reads or target_reads is NULL");
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        std::vector<gwamd_window_segment> result;
        cut_resident(*query_reads->reads, *target_reads->reads, records, window_length, num_alignment_engines,
                     result);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

void gwamd_window_segments_free(gwamd_window_segment* segments) { delete[] segments; }

int32_t gwamd_internal_window_segments_strided(const gwamd_overlap* overlaps, int64_t n, const int8_t* paths,
                                               const int32_t* path_lengths, int64_t stride, int32_t window_length,
                                               gwamd_window_segment** out, int64_t* num_out)
{
    gp::clear_outputs(out, num_out);
    return gm::guarded_map([&] {
        if (!out || !num_out)
            throw std::invalid_argument("out or num_out is NULL");
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        if (stride < 4 || stride % 4 != 0 || stride >= (int64_t(1) << 31))
            throw std::invalid_argument("stride must be a positive multiple of 4 below 2^31");
        if (n > 0 && (!paths || !path_lengths))
            throw std::invalid_argument("paths or path_lengths is NULL");
        for (int64_t i = 0; i < n; i++)
            if (path_lengths[i] < 0 || path_lengths[i] > stride)
                throw std::invalid_argument("path " + std::to_string(i) + ": length outside 0..stride");
        (void)gp::plan_records(records.data(), n, window_length);
        if (n == 0)
            return int32_t(0);
        std::vector<gwamd_window_segment> result;
        gp::cut_on_device(records, paths, n * stride, nullptr, stride,
                          std::vector<int32_t>(path_lengths, path_lengths + n), int32_t(stride), true, window_length,
                          nullptr, result);
        gm::hand_over(result, out, num_out);
        return int32_t(0);
    });
}

int32_t gwamd_build_windows(const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                            const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                            const gwamd_overlap* overlaps, int64_t n, const gwamd_window_segment* segments,
                            int64_t num_segments, int32_t window_length, int32_t max_sequences_per_window,
                            gwamd_windows** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        const gm::ReadSet targets{target_bases, target_offsets, num_targets};
        const gm::ReadSet queries{query_bases, query_offsets, num_queries};
        gm::check_read_set("target", targets);
        gm::check_read_set("query", queries);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        *out = group_windows(targets, queries, records, segments, num_segments, window_length,
                             max_sequences_per_window)
                   .release();
        return int32_t(0);
    });
}

int32_t gwamd_windows_get(const gwamd_windows* windows, gwamd_windows_view* view)
{
    return gm::guarded_map([&] {
        if (!windows || !view)
            throw std::invalid_argument("windows or view is NULL");
        const gwamd_window_slices& g = windows->grouped;
        view->num_windows      = int64_t(g.window_counts.size());
        view->num_sequences    = int64_t(g.sequence_overlap.size());
        view->num_bases        = int64_t(windows->bases.size());
        view->dropped_by_cap   = g.dropped_by_cap;
        view->bases            = windows->bases.data();
        view->sequence_offsets = windows->sequence_offsets.data();
        view->window_counts    = g.window_counts.data();
        view->window_target    = g.window_target.data();
        view->window_index     = g.window_index.data();
        view->sequence_overlap = g.sequence_overlap.data();
        view->sequence_t_begin = g.sequence_t_begin.data();
        view->sequence_t_end   = g.sequence_t_end.data();
        return int32_t(0);
    });
}

void gwamd_windows_free(gwamd_windows* windows) { delete windows; }

int32_t gwamd_build_window_slices(const int64_t* target_offsets, int32_t num_targets, const int64_t* query_offsets,
                                  int32_t num_queries, const char* query_qualities_or_null,
                                  int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                  const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
                                  int32_t max_sequences_per_window, gwamd_window_slices** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        // only offsets are read: the bases pointer stands for "somewhere"
        static const char somewhere = 0;
        const gm::ReadSet targets{&somewhere, target_offsets, num_targets};
        const gm::ReadSet queries{&somewhere, query_offsets, num_queries};
        gm::check_read_set("target", targets);
        gm::check_read_set("query", queries);
        if (query_qualities_or_null)
            gm::check_qualities(queries, query_qualities_or_null);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        *out = group_slices(targets, queries, query_qualities_or_null, quality_threshold_tenths, records, segments,
                            num_segments, window_length, max_sequences_per_window)
                   .release();
        return int32_t(0);
    });
}

int32_t gwamd_build_window_slices_device(const int64_t* target_offsets, int32_t num_targets,
                                         const int64_t* query_offsets, int32_t num_queries,
                                         const gwamd_device_reads* query_reads_or_null,
                                         int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                         const gwamd_window_segment* segments, int64_t num_segments,
                                         int32_t window_length, int32_t max_sequences_per_window, int32_t device_id,
                                         gwamd_device_allocator* allocator_or_null, gwamd_window_slices** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (device_id < 0)
            throw std::invalid_argument("device_id must not be negative");
        static const char somewhere = 0; // only offsets are read
        const gm::ReadSet targets{&somewhere, target_offsets, num_targets};
        const gm::ReadSet queries{&somewhere, query_offsets, num_queries};
        gm::check_read_set("target", targets);
        gm::check_read_set("query", queries);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        *out = group_segments_on_device(targets, queries, query_reads_or_null ? query_reads_or_null->reads.get() : nullptr,
                                        quality_threshold_tenths, records, segments, num_segments, window_length,
                                        max_sequences_per_window, device_id,
                                        allocator_or_null ? allocator_or_null->alloc.budget() : nullptr)
                   .release();
        return int32_t(0);
    });
}

int32_t gwamd_internal_group_repeat(const int64_t* target_offsets, int32_t num_targets, const int64_t* query_offsets,
                                    int32_t num_queries, const gwamd_device_reads* query_reads_or_null,
                                    int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                    const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
                                    int32_t max_sequences_per_window, int32_t device_id, int32_t repeats,
                                    double* seconds)
{
    return gm::guarded_map([&] {
        if (repeats < 1 || !seconds || device_id < 0)
            throw std::invalid_argument("repeats below 1, NULL seconds or a negative device_id");
        static const char somewhere = 0;
        const gm::ReadSet targets{&somewhere, target_offsets, num_targets};
        const gm::ReadSet queries{&somewhere, query_offsets, num_queries};
        gm::check_read_set("target", targets);
        gm::check_read_set("query", queries);
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        (void)group_segments_on_device(targets, queries, query_reads_or_null ? query_reads_or_null->reads.get() : nullptr,
                                       quality_threshold_tenths, records, segments, num_segments, window_length,
                                       max_sequences_per_window, device_id, nullptr, repeats, seconds);
        return int32_t(0);
    });
}

int32_t gwamd_window_slices_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                     const gwamd_overlap* overlaps, int32_t n, const uint32_t* ops_or_null,
                                     const int64_t* op_offsets_or_null, int32_t convention, int32_t window_length,
                                     int32_t max_sequences_per_window, int32_t quality_threshold_tenths,
                                     int32_t num_alignment_engines, gwamd_window_slices** out)
{
    if (out)
        *out = nullptr;
    return gm::guarded_map([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (!query_reads || !target_reads)
            throw std::invalid_argument("query_reads or target_reads is NULL");
        if (ops_or_null && !op_offsets_or_null)
            throw std::invalid_argument("ops without op_offsets");
        std::vector<gm::OverlapRecord> records;
        gp::check_cut_overlaps(overlaps, n, records);
        *out = slices_resident(*query_reads->reads, *target_reads->reads, records, ops_or_null, op_offsets_or_null,
                               convention, window_length, max_sequences_per_window, quality_threshold_tenths,
                               num_alignment_engines)
                   .release();
        return int32_t(0);
    });
}

int32_t gwamd_window_slices_get(const gwamd_window_slices* windows, gwamd_window_slices_view* view)
{
    return gm::guarded_map([&] {
        if (!windows || !view)
            throw std::invalid_argument("windows or view is NULL");
        view->num_windows        = int64_t(windows->window_counts.size());
        view->num_sequences      = int64_t(windows->slices.size());
        view->dropped_by_cap     = windows->dropped_by_cap;
        view->dropped_by_quality = windows->dropped_by_quality;
        view->slices             = windows->slices.data();
        view->window_counts      = windows->window_counts.data();
        view->window_target      = windows->window_target.data();
        view->window_index       = windows->window_index.data();
        view->sequence_overlap   = windows->sequence_overlap.data();
        view->sequence_t_begin   = windows->sequence_t_begin.data();
        view->sequence_t_end     = windows->sequence_t_end.data();
        return int32_t(0);
    });
}

void gwamd_window_slices_free(gwamd_window_slices* windows) { delete windows; }

int32_t gwamd_trim_consensus(const uint16_t* coverage, int32_t length, int32_t num_sequences, int32_t* begin,
                             int32_t* past_the_end)
{
    return gm::guarded_map([&] {
        if (!begin || !past_the_end || length < 0 || num_sequences < 1 || (length > 0 && !coverage))
            throw std::invalid_argument("trim_consensus: NULL pointer, negative length or no sequence");
        const int32_t average = (num_sequences - 1) / 2;
        int32_t first = 0, last = length - 1;
        while (first < length && int32_t(coverage[first]) < average)
            first++;
        while (last >= 0 && int32_t(coverage[last]) < average)
            last--;
        const bool trim = first < last;
        *begin          = trim ? first : 0;
        *past_the_end   = trim ? last + 1 : length;
        return int32_t(0);
    });
}

} // extern "C"
