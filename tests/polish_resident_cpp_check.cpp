// The C++ side of cudapolish's resident route: FASTQ qualities through
// io::FastaParser, cudamapper::DeviceReads::create with qualities and
// cudapolish::add_poa_group_resident (cudapolish/windows.hpp).  The host part
// needs no device; with the argument "gpu" one window is added to one batch
// from the host with weights and to another as slices, and the two consensus
// results are compared.  Prints "ok <name>" per scenario
// (tests/test_polish_resident_cpp.py).
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
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

template <typename F>
static bool refused(F&& f)
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
    // argv[1]: a scratch FASTQ path; argv[2]: "gpu"
    if (argc < 2)
        return 2;
    const bool gpu = argc > 2 && std::strcmp(argv[2], "gpu") == 0;
    {
        std::ofstream out(argv[1], std::ios::binary);
        out << "@a x\r\nACGT\r\nAC\r\n+\r\nIIII\r\n#!\r\n@b\nGG\n+\n@@\n";
    }
    auto parsed = io::create_kseq_fasta_parser(argv[1], 0, false);
    expect(parsed->get_num_seqences() == 2 && parsed->get_sequence_by_id(0).seq == "ACGTAC" &&
               parsed->get_quality_by_id(0) == "IIII#!" && parsed->get_quality_by_id(1) == "@@",
           "fastq_qualities");
    auto plain = io::create_fasta_parser_from_sequences({{"t", "ACGT"}});
    expect(plain->get_quality_by_id(0).empty(), "fasta_has_none");
    expect(refused([] { io::create_fasta_parser_from_sequences({{"t", "ACGT"}}, {"IIII", "I"}); }),
           "quality_count_refused");
    // a quality string of another length than its read, and a character below 33: refused before any device call
    auto short_quality = io::create_fasta_parser_from_sequences({{"t", "ACGT"}}, {"III"});
    auto blank_quality = io::create_fasta_parser_from_sequences({{"t", "ACGT"}}, {"II I"});
    expect(refused([&] {
               cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *short_quality,
                                               cudamapper::DeviceReads::with_qualities_t{});
           }) && refused([&] {
               cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *blank_quality,
                                               cudamapper::DeviceReads::with_qualities_t{});
           }),
           "bad_qualities_refused");
    if (!gpu)
        return 0;

    // one window of four sequences; the third is stored reverse-complemented inside a longer read
    const std::vector<std::string> seqs{"ACGTTGCAACGTAGGCTAAC", "ACGTTGCATCGTAGGCTAAC", "ACGTTGCAACGTAGCTAAC",
                                        "ACGTTGAACGTAGGCTAAC"};
    const std::vector<std::string> quals{"IIIIIIIIIIIIIIIIIIII", "5555555555+555555555", "?>=<;:9876543210/.-",
                                         "&&&&&&IIIIIII&&&&&&"};
    auto weights_of = [](const std::string& q) {
        std::vector<int8_t> w(q.size());
        for (size_t i = 0; i < q.size(); i++)
            w[i] = int8_t(q[i] - 33);
        return w;
    };
    // read 2 as stored: "TT" + reverse complement of seqs[2] + "G", its qualities turned round
    const std::string rc2 = "GTTAGCTACGTTGCAACGT";
    const std::string q2(quals[2].rbegin(), quals[2].rend());
    auto reads = io::create_fasta_parser_from_sequences(
        {{"r0", seqs[0]}, {"r1", "N" + seqs[1]}, {"r2", "TT" + rc2 + "G"}, {"r3", seqs[3]}},
        {quals[0], "#" + quals[1], "##" + q2 + "#", quals[3]});
    auto resident = cudamapper::DeviceReads::create(DefaultDeviceAllocator(), *reads,
                                                    cudamapper::DeviceReads::with_qualities_t{});
    expect(resident->has_qualities() && resident->number_of_reads() == 4, "device_reads_with_qualities");

    const cudapoa::BatchSize size(256, 8, 256);
    auto host   = cudapoa::create_batch(0, nullptr, size_t(256) << 20, cudapoa::OutputType::consensus, size, -8, -6, 8, false);
    auto device = cudapoa::create_batch(0, nullptr, size_t(256) << 20, cudapoa::OutputType::consensus, size, -8, -6, 8, false);
    std::vector<std::vector<int8_t>> weights;
    cudapoa::Group group;
    for (size_t i = 0; i < seqs.size(); i++)
    {
        weights.push_back(weights_of(quals[i]));
        group.push_back(cudapoa::Entry{seqs[i].data(), weights.back().data(), int32_t(seqs[i].size())});
    }
    std::vector<cudapoa::StatusType> host_status, device_status;
    const auto host_rc = host->add_poa_group(host_status, group);
    const std::vector<cudapolish::ReadSlice> slices{{0, 0, 0, 20, 0},
                                                    {0, 1, 1, 21, 0},
                                                    {0, 2, 2, 21, cudapolish::ReadSlice::reverse},
                                                    {0, 3, 0, 19, 0}};
    const auto device_rc = cudapolish::add_poa_group_resident(*device, device_status, {resident.get()}, slices);
    expect(host_rc == cudapoa::StatusType::success && device_rc == host_rc && device_status == host_status &&
               device_status.size() == 4,
           "statuses_equal");
    expect(refused([&] {
               cudapolish::add_poa_group_resident(*device, device_status, {resident.get()}, {{0, 4, 0, 1, 0}});
           }) && refused([&] {
               cudapolish::add_poa_group_resident(*device, device_status, {resident.get()}, {{0, 3, 0, 20, 0}});
           }) && refused([&] {
               cudapolish::add_poa_group_resident(*device, device_status, {nullptr}, {{0, 0, 0, 1, 0}});
           }) && device->get_total_poas() == 1,
           "bad_slices_refused");
    host->generate_poa();
    device->generate_poa();
    std::vector<std::string> host_consensus, device_consensus;
    std::vector<std::vector<uint16_t>> host_coverage, device_coverage;
    std::vector<cudapoa::StatusType> host_out, device_out;
    host->get_consensus(host_consensus, host_coverage, host_out);
    device->get_consensus(device_consensus, device_coverage, device_out);
    expect(device_consensus == host_consensus && device_coverage == host_coverage && device_out == host_out &&
               device_out.size() == 1 && device_out[0] == cudapoa::StatusType::success &&
               !device_consensus[0].empty(),
           "consensus_equal");
    return 0;
}
