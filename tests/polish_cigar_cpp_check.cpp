// The C++ interface of cudapolish's cut from CIGAR runs (cudapolish/windows.hpp)
// under the legacy namespace alias: cigar_ops, the host walk in both
// conventions, read_paf and the argument checks on the host; with the argument
// "gpu" also window_segments_cigar against the host walk.
// Prints "ok <name>" per scenario (tests/test_polish_cigar_cpu.py, tests/test_polish_cigar_gpu.py).
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace claragenomics;
using cudapolish::CigarConvention;
using cudapolish::WindowSegment;

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

static bool same(const std::vector<WindowSegment>& a, const std::vector<WindowSegment>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(WindowSegment)) == 0);
}

template <typename F>
static bool refuses(F&& f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument&)
    {
        return true;
    }
    return false;
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    expect(cudapolish::cigar_ops("12M3I4D5=1X") ==
                   std::vector<uint32_t>{12u << 4, 3u << 4 | 1, 4u << 4 | 2, 5u << 4 | 7, 1u << 4 | 8} &&
               cudapolish::cigar_ops("").empty(),
           "cigar_ops");
    expect(refuses([] { cudapolish::cigar_ops("M"); }) && refuses([] { cudapolish::cigar_ops("3Q"); }) &&
               refuses([] { cudapolish::cigar_ops("268435456M"); }) && refuses([] { cudapolish::cigar_ops("3M4"); }),
           "cigar_refused");

    // "window covered only by insertion states" of tests/polish_cases.py, windows of four:
    // q 0..3 on t 0..3, t 4..7 without a query base, q 4..7 on t 8..11; and its Reverse mirror
    const auto forward = overlap(0, 0, 0, 8, 0, 12, '+'), mirror = overlap(0, 0, 0, 8, 0, 12, '-');
    const auto walked  = cudapolish::window_segments_cigar_host(forward, cudapolish::cigar_ops("4=4I4X"), 4);
    const auto walked_mirror =
        cudapolish::window_segments_cigar_host(mirror, cudapolish::cigar_ops("4=4I4X"), 4, CigarConvention::genomeworks, 5);
    expect(walked.size() == 3 && walked[0].q_end == 4 && walked[0].t_end == 4 && walked[1].flags == WindowSegment::empty &&
               walked[2].q_begin == 4 && walked[2].t_begin == 8 && walked[2].t_end == 12 && walked[2].window == 2 &&
               walked_mirror.size() == 3 && walked_mirror[0].overlap == 5 && walked_mirror[0].q_begin == 4 &&
               walked_mirror[0].q_end == 8 && walked_mirror[0].flags == WindowSegment::reverse &&
               walked_mirror[2].q_begin == 0 && walked_mirror[2].t_begin == 8,
           "host_walk");
    // SAM: the target-only run is a D, and the mirror's ops run the other way
    expect(same(walked, cudapolish::window_segments_cigar_host(forward, cudapolish::cigar_ops("4=4D4X"), 4,
                                                               CigarConvention::sam)) &&
               same(walked_mirror, cudapolish::window_segments_cigar_host(mirror, cudapolish::cigar_ops("4X4D4="), 4,
                                                                          CigarConvention::sam, 5)) &&
               cudapolish::window_segments_cigar_host(forward, cudapolish::cigar_ops("4=4I4X"), 4, CigarConvention::sam)[0]
                       .flags == (WindowSegment::empty | WindowSegment::bad_path),
           "host_walk_sam");

    auto targets = io::create_fasta_parser_from_sequences({{"t0", "ACGTACGTACGT"}});
    auto queries = io::create_fasta_parser_from_sequences({{"q0", "TTTTACGAAGT"}, {"q1", "AACCGGTT"}});
    const std::string paf = "q1\t8\t0\t8\t-\tt0\t12\t0\t12\t30\t12\t255\tNM:i:0\tcg:Z:4=4I4X\n"
                            "q0\t11\t4\t11\t+\tt0\t12\t0\t8\t15\t8\t255\n";
    const cudapolish::PafOverlaps read = cudapolish::read_paf(paf, *queries, *targets, 15);
    expect(read.overlaps.size() == 2 && read.overlaps[0].query_read_id_ == 1 && read.overlaps[0].num_residues_ == 2 &&
               read.overlaps[0].relative_strand == cudamapper::RelativeStrand::Reverse &&
               read.overlaps[1].query_start_position_in_read_ == 4 && read.overlaps[1].target_end_position_in_read_ == 8 &&
               read.cigars[0] == cudapolish::cigar_ops("4=4I4X") && read.cigars[1].empty() &&
               refuses([&] { cudapolish::read_paf("q2" + paf.substr(2), *queries, *targets); }),
           "read_paf");
    expect(refuses([&] {
               cudapolish::window_segments_cigar(DefaultDeviceAllocator(), {forward}, {cudapolish::cigar_ops("8M")}, 4,
                                                 static_cast<CigarConvention>(2));
           }) && refuses([&] { cudapolish::window_segments_cigar(DefaultDeviceAllocator(), {forward}, {}, 4); }) &&
               refuses([&] {
                   cudapolish::window_segments_cigar(DefaultDeviceAllocator(), {forward}, {cudapolish::cigar_ops("8M")}, 0);
               }),
           "convention_refused");
    expect(cudapolish::window_segments_cigar(DefaultDeviceAllocator(), {}, {}, 4).empty(), "no_overlaps_no_device_call");
    if (!gpu)
        return 0;

    const std::vector<cudamapper::Overlap> both{forward, mirror, forward};
    const std::vector<std::vector<uint32_t>> cigars{cudapolish::cigar_ops("4=4I4X"), cudapolish::cigar_ops("4=4I4X"),
                                                    cudapolish::cigar_ops("4=4I5X")};
    const auto cut = cudapolish::window_segments_cigar(DefaultDeviceAllocator(), both, cigars, 4);
    auto expected  = walked;
    auto second    = cudapolish::window_segments_cigar_host(mirror, cigars[1], 4, CigarConvention::genomeworks, 1);
    auto third     = cudapolish::window_segments_cigar_host(forward, cigars[2], 4, CigarConvention::genomeworks, 2);
    expected.insert(expected.end(), second.begin(), second.end());
    expected.insert(expected.end(), third.begin(), third.end());
    expect(same(cut, expected) && cut.size() == 9 && (cut[8].flags & WindowSegment::bad_path), "device_cut");
    const std::vector<std::vector<uint32_t>> sam{cudapolish::cigar_ops("4=4D4X"), cudapolish::cigar_ops("4X4D4="),
                                                 cudapolish::cigar_ops("4=4D5X")};
    expect(same(cudapolish::window_segments_cigar(DefaultDeviceAllocator(), both, sam, 4, CigarConvention::sam), expected),
           "device_cut_sam");
    return 0;
}
