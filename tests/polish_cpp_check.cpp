// The C++ interface of cudapolish (cudapolish/windows.hpp) under the legacy
// namespace alias: build_windows and the argument checks on the host; with the
// argument "gpu" also window_segments on host paths and on resident reads.
// Prints "ok <name>" per scenario (tests/test_polish_capi.py, tests/test_polish_gpu.py).
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace claragenomics;
using cudaaligner::AlignmentState;

static void expect(bool ok, const char* what)
{
    if (!ok)
    {
        std::printf("FAILED %s\n", what);
        std::exit(1);
    }
    std::printf("ok %s\n", what);
}

static cudamapper::Overlap overlap(uint32_t q, uint32_t t, uint32_t qs, uint32_t qe, uint32_t ts, uint32_t te, char strand)
{
    cudamapper::Overlap o{};
    o.query_read_id_                 = q;
    o.target_read_id_                = t;
    o.query_start_position_in_read_  = qs;
    o.query_end_position_in_read_    = qe;
    o.target_start_position_in_read_ = ts;
    o.target_end_position_in_read_   = te;
    o.relative_strand = strand == '-' ? cudamapper::RelativeStrand::Reverse : cudamapper::RelativeStrand::Forward;
    return o;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    auto targets = io::create_fasta_parser_from_sequences({{"t0", "ACGTACGTAC"}});
    auto queries = io::create_fasta_parser_from_sequences({{"q0", "TTTTACGAAGT"}, {"q1", "AACC"}});
    std::vector<cudamapper::Overlap> overlaps{overlap(0, 0, 4, 11, 0, 8, '+'), overlap(1, 0, 0, 4, 4, 8, '-')};
    std::vector<cudapolish::WindowSegment> segments{{0, 0, 4, 7, 0, 3, 0, 0},
                                                    {0, 1, 7, 11, 4, 8, 0, 0},
                                                    {1, 1, 0, 4, 4, 8, cudapolish::WindowSegment::reverse, 0}};
    cudapolish::Windows windows = cudapolish::build_windows(*targets, *queries, overlaps, segments, 4);
    auto text = [&](size_t g, size_t e) { return std::string(windows.groups[g][e].seq, size_t(windows.groups[g][e].length)); };
    expect(windows.groups.size() == 3 && windows.groups[0].size() == 2 && windows.groups[1].size() == 3 &&
               windows.groups[2].size() == 1,
           "group_sizes");
    expect(text(0, 0) == "ACGT" && text(0, 1) == "ACG" && text(1, 1) == "AAGT" && text(1, 2) == "GGTT" &&
               text(2, 0) == "AC",
           "group_sequences");
    expect(windows.window[1] == 1 && windows.target[1] == 0 && windows.sequence[1][2].overlap == 1 &&
               windows.sequence[1][0].overlap == -1 && windows.sequence[0][1].t_end == 3 && windows.dropped_by_cap == 0,
           "group_metadata");
    bool refused = false;
    try
    {
        cudapolish::window_segments(DefaultDeviceAllocator(), overlaps, {{}, {}}, 0);
    }
    catch (const std::invalid_argument&)
    {
        refused = true;
    }
    expect(refused, "window_length_refused");
    expect(cudapolish::window_segments(DefaultDeviceAllocator(), {}, std::vector<std::vector<AlignmentState>>{}, 4).empty(),
           "no_overlaps_no_device_call");
    if (!gpu)
        return 0;

    // eight matches over target [0, 8), windows of four; then the same through the aligner on resident reads
    auto same = io::create_fasta_parser_from_sequences({{"r", "ACGTTGCA"}});
    std::vector<cudamapper::Overlap> whole{overlap(0, 0, 0, 8, 0, 8, '+')};
    std::vector<std::vector<AlignmentState>> paths{std::vector<AlignmentState>(8, AlignmentState::match)};
    auto cut = cudapolish::window_segments(DefaultDeviceAllocator(), whole, paths, 4);
    expect(cut.size() == 2 && cut[0].q_begin == 0 && cut[0].q_end == 4 && cut[1].t_begin == 4 && cut[1].t_end == 8 &&
               cut[1].window == 1 && cut[1].flags == 0,
           "host_paths");
    auto reads    = cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *same);
    auto resident = cudapolish::window_segments(DefaultDeviceAllocator(), whole, *reads, *reads, 4, 1);
    expect(resident.size() == cut.size() &&
               std::memcmp(resident.data(), cut.data(), cut.size() * sizeof(cudapolish::WindowSegment)) == 0,
           "resident_reads");
    return 0;
}
