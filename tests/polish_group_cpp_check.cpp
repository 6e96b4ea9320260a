// The C++ side of cudapolish's grouping on the device (cudapolish/windows.hpp):
// window_slices_resident (aligned, and from CIGARs), build_window_slices_device
// and add_poa_groups_resident against the host grouping of the C ABI
// (gwamd_build_window_slices) and against add_poa_group_resident group by group.
// Needs a device.  Prints "ok <name>" per scenario
// (tests/test_polish_group_e2e_gpu.py).
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include <gwamd_polish.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace claragenomics;

static void expect(bool ok, const char* what)
{
    if (!ok)
    {
        std::printf("FAILED %s\n", what);
        std::exit(1);
    }
    std::printf("ok %s\n", what);
}

static std::string reverse_complement(const std::string& s)
{
    std::string out(s.rbegin(), s.rend());
    for (char& c : out)
        c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
    return out;
}

// the host grouping of the C ABI as a WindowSlices
static cudapolish::WindowSlices host_grouping(const std::vector<int64_t>& target_offsets,
                                              const std::vector<int64_t>& query_offsets,
                                              const std::vector<gwamd_overlap>& overlaps,
                                              const std::vector<cudapolish::WindowSegment>& segments, int32_t w,
                                              int32_t cap)
{
    gwamd_window_slices* handle = nullptr;
    const int32_t rc            = gwamd_build_window_slices(
        target_offsets.data(), int32_t(target_offsets.size()) - 1, query_offsets.data(),
        int32_t(query_offsets.size()) - 1, nullptr, 100, overlaps.data(), int64_t(overlaps.size()),
        reinterpret_cast<const gwamd_window_segment*>(segments.data()), int64_t(segments.size()), w, cap, &handle);
    gwamd_window_slices_view v;
    if (rc != 0 || gwamd_window_slices_get(handle, &v) != 0)
    {
        std::printf("FAILED host grouping\n");
        std::exit(1);
    }
    cudapolish::WindowSlices out;
    out.slices.resize(size_t(v.num_sequences));
    std::memcpy(static_cast<void*>(out.slices.data()), v.slices, size_t(v.num_sequences) * sizeof(gwamd_read_slice));
    out.window_counts.assign(v.window_counts, v.window_counts + v.num_windows);
    out.window_target.assign(v.window_target, v.window_target + v.num_windows);
    out.window_index.assign(v.window_index, v.window_index + v.num_windows);
    out.sequence_overlap.assign(v.sequence_overlap, v.sequence_overlap + v.num_sequences);
    out.sequence_t_begin.assign(v.sequence_t_begin, v.sequence_t_begin + v.num_sequences);
    out.sequence_t_end.assign(v.sequence_t_end, v.sequence_t_end + v.num_sequences);
    out.dropped_by_cap     = v.dropped_by_cap;
    out.dropped_by_quality = v.dropped_by_quality;
    gwamd_window_slices_free(handle);
    return out;
}

static bool same_counts(const cudapolish::WindowSlices& a, const cudapolish::WindowSlices& b)
{
    return a.window_counts == b.window_counts && a.window_target == b.window_target &&
           a.window_index == b.window_index && a.dropped_by_cap == b.dropped_by_cap &&
           a.dropped_by_quality == b.dropped_by_quality;
}

static bool same_slices(const cudapolish::WindowSlices& a, const cudapolish::WindowSlices& b)
{
    return a.slices.size() == b.slices.size() &&
           std::memcmp(a.slices.data(), b.slices.data(), a.slices.size() * sizeof(cudapolish::ReadSlice)) == 0 &&
           a.sequence_overlap == b.sequence_overlap && a.sequence_t_begin == b.sequence_t_begin &&
           a.sequence_t_end == b.sequence_t_end;
}

int main()
{
    // one target of 96 bases and five reads of it with substitutions, the last two stored reverse-complemented
    uint32_t state = 12345;
    auto next      = [&] { return (state = state * 1664525u + 1013904223u) >> 16; };
    std::string target;
    for (int i = 0; i < 96; i++)
        target += "ACGT"[next() % 4];
    std::vector<io::FastaSequence> reads;
    std::vector<cudamapper::Overlap> overlaps;
    std::vector<gwamd_overlap> c_overlaps;
    std::vector<int64_t> query_offsets{0};
    for (uint32_t q = 0; q < 5; q++)
    {
        std::string read = target;
        for (int j = 0; j < 6; j++)
            read[next() % read.size()] = "ACGT"[next() % 4];
        const bool reverse = q >= 3;
        reads.push_back({"q" + std::to_string(q), reverse ? reverse_complement(read) : read});
        cudamapper::Overlap o;
        o.query_read_id_                 = q;
        o.target_read_id_                = 0;
        o.query_start_position_in_read_  = 0;
        o.query_end_position_in_read_    = 96;
        o.target_start_position_in_read_ = 0;
        o.target_end_position_in_read_   = 96;
        o.relative_strand = reverse ? cudamapper::RelativeStrand::Reverse : cudamapper::RelativeStrand::Forward;
        overlaps.push_back(o);
        c_overlaps.push_back(gwamd_overlap{q, 0, 0, 0, 96, 96, static_cast<unsigned char>(reverse ? '-' : '+'), 0, 0});
        query_offsets.push_back(query_offsets.back() + 96);
    }
    const std::vector<int64_t> target_offsets{0, 96};
    auto target_parser = io::create_fasta_parser_from_sequences({{"t", target}});
    auto query_parser  = io::create_fasta_parser_from_sequences(reads);
    auto t_reads       = cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *target_parser);
    auto q_reads       = cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *query_parser);
    const int32_t w = 16, cap = 4;

    const auto segments = cudapolish::window_segments(DefaultDeviceAllocator(), overlaps, *q_reads, *t_reads, w, 1);
    const auto expected = host_grouping(target_offsets, query_offsets, c_overlaps, segments, w, cap);
    const auto fused    = cudapolish::window_slices_resident(overlaps, *q_reads, *t_reads, w, cap, 100, 2);
    expect(expected.window_counts.size() == 6 && expected.dropped_by_cap == 12 && same_counts(fused, expected),
           "fused_counts");
    expect(same_slices(fused, expected), "fused_slices");
    const auto grouped =
        cudapolish::build_window_slices_device(DefaultDeviceAllocator(), *target_parser, *query_parser, overlaps,
                                               segments, w, cap);
    expect(same_counts(grouped, expected) && same_slices(grouped, expected), "device_grouping");

    // substitutions only: 96M is every overlap's CIGAR, in either convention
    const std::vector<std::vector<uint32_t>> cigars(overlaps.size(), std::vector<uint32_t>{96u << 4 | 0u});
    const auto cut = cudapolish::window_segments_cigar(DefaultDeviceAllocator(), overlaps, cigars, w,
                                                       cudapolish::CigarConvention::sam);
    const auto from_cigars = cudapolish::window_slices_resident(overlaps, *q_reads, *t_reads, w, cap, 100, 1, &cigars,
                                                                cudapolish::CigarConvention::sam);
    const auto expected_cigars = host_grouping(target_offsets, query_offsets, c_overlaps, cut, w, cap);
    expect(same_counts(from_cigars, expected_cigars) && same_slices(from_cigars, expected_cigars), "cigar_route");

    // all groups in one call against one call per group
    const cudapoa::BatchSize size(256, 8, 256);
    auto one  = cudapoa::create_batch(0, nullptr, size_t(256) << 20, cudapoa::OutputType::consensus, size, -8, -6, 8, false);
    auto many = cudapoa::create_batch(0, nullptr, size_t(256) << 20, cudapoa::OutputType::consensus, size, -8, -6, 8, false);
    const std::vector<const cudamapper::DeviceReads*> sets{t_reads.get(), q_reads.get()};
    std::vector<cudapoa::StatusType> single_groups, single_seqs, seq_status;
    size_t at = 0;
    for (int32_t count : fused.window_counts)
    {
        const std::vector<cudapolish::ReadSlice> group(fused.slices.begin() + at, fused.slices.begin() + at + count);
        single_groups.push_back(cudapolish::add_poa_group_resident(*one, seq_status, sets, group));
        single_seqs.insert(single_seqs.end(), seq_status.begin(), seq_status.end());
        at += size_t(count);
    }
    std::vector<cudapoa::StatusType> group_status, per_seq_status;
    const int32_t added =
        cudapolish::add_poa_groups_resident(*many, group_status, per_seq_status, sets, fused.slices, fused.window_counts);
    expect(added == 6 && group_status == single_groups && per_seq_status == single_seqs &&
               many->get_total_poas() == one->get_total_poas(),
           "groups_added");
    one->generate_poa();
    many->generate_poa();
    std::vector<std::string> one_consensus, many_consensus;
    std::vector<std::vector<uint16_t>> one_coverage, many_coverage;
    std::vector<cudapoa::StatusType> one_out, many_out;
    one->get_consensus(one_consensus, one_coverage, one_out);
    many->get_consensus(many_consensus, many_coverage, many_out);
    expect(many_consensus == one_consensus && many_coverage == one_coverage && many_out == one_out &&
               many_out.size() == 6 && many_out[0] == cudapoa::StatusType::success && !many_consensus[0].empty(),
           "groups_consensus");
    return 0;
}
