// cudamapper command-line tool (reference cudamapper/src/main.cu,
// application_parameters.cpp), linked to libgwamd.so: all-to-all or
// query-to-target overlaps of two FASTA/FASTQ files in PAF.
//
// The query x target matrix of indices is cut into host batches and device
// batches (index_batcher.hpp).  One worker thread per device takes host batches
// from a shared list, builds their indices once through IndexCacheHost /
// IndexCacheDevice and, per pair of indices, matches and chains overlaps; writer
// threads take it from there.  Where this tool departs from the reference:
//   - stage order: per index pair the overlaps are fused (post_process_overlaps),
//     rescued (-R) and then aligned (-a), so the CIGARs belong to the overlaps
//     that are printed; the reference aligns first and prints the fused and
//     rescued list with the old CIGARs;
//   - the reads of each parser are put on each device once (DeviceReads); the
//     rescue and the alignment read them there;
//   - -R rescues at an extension of 50 and a similarity of 0.5, the numbers the
//     reference passes (and then ignores for 100 / 0.9);
//   - -m is the capacity of the worker's device budget, nothing is allocated ahead;
//   - --target-indices-in-device-memory sets the target value (the reference's
//     table maps it to -q);
//   - the writer threads per device are clamp(usable / devices - 1, 1, 4), usable
//     being the CPUs of the process's affinity mask, 16 at the most, and one
//     alignment call is in flight per device (its batch sizing assumes it has the
//     device's free memory).
#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_batcher.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_cache.hpp>
#include <claraparabricks/genomeworks/cudamapper/matcher.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>
#include <claraparabricks/genomeworks/cudamapper/overlapper_triggered.hpp>

#include "diag_env.hpp"

#include <hip/hip_runtime_api.h>

#include <getopt.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <exception>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudamapper;

namespace
{

struct Parameters
{
    int32_t kmer_size = 15, window_size = 10, num_devices = 1, max_cached_memory = 0;
    int32_t index_size = 30, target_index_size = 30; // MB
    double filtering_parameter = 1e-5;
    int32_t alignment_engines = 0;
    int32_t min_residues = 3, min_overlap_len = 250, min_bases_per_residue = 1000;
    float min_overlap_fraction = 0.8f;
    bool rescue = false, drop_fused = false, all_to_all = false;
    int32_t query_host = 10, query_device = 5, target_host = 10, target_device = 5;
    std::string query_path, target_path;
    std::shared_ptr<io::FastaParser> query_parser, target_parser;
    int64_t index_bases = 0, target_index_bases = 0; // basepairs per index
};

[[noreturn]] void usage(int code)
{
    std::cerr << "Usage: cudamapper [options ...] <query_sequences> <target_sequences>\n"
                 "  <sequences>: FASTA/FASTQ files; the same path twice maps the reads all-to-all\n"
                 "  options:\n"
                 "    -k, --kmer-size                        length of kmer to use for minimizers [15] (Max="
              << Index::maximum_kmer_size()
              << ")\n"
                 "    -w, --window-size                      length of window to use for minimizers [10]\n"
                 "    -d, --num-devices                      number of GPUs to use [1]\n"
                 "    -m, --max-cached-memory                limit of device memory per device in GiB, 0 = no limit;\n"
                 "                                           nothing is allocated ahead [0]\n"
                 "    -i, --index-size                       bases per query index in MB [30]\n"
                 "    -t, --target-index-size                bases per target index in MB [30]\n"
                 "    -F, --filtering-parameter              remove representations whose share of all sketch elements\n"
                 "                                           is >= this; 1.0 disables filtering (0.0 .. 1.0) [1e-5]\n"
                 "    -a, --alignment-engines                alignment engines per device for CIGAR strings,\n"
                 "                                           0 = no alignment [0]\n"
                 "    -r, --min-residues                     minimum number of matching residues in an overlap [3]\n"
                 "    -l, --min-overlap-length               minimum length of an overlap [250]\n"
                 "    -b, --min-bases-per-residue            minimum number of bases in an overlap per match [1000]\n"
                 "    -z, --min-overlap-fraction             minimum ratio of overlap length to alignment length [0.8]\n"
                 "    -R, --rescue-overlap-ends              extend overlaps at their ends where the reads stay similar\n"
                 "                                           (three rounds, extension 50, similarity 0.5)\n"
                 "    -D, --drop-fused-overlaps              remove overlaps that were joined into larger ones\n"
                 "    -Q, --query-indices-in-host-memory     number of query indices to keep in host memory [10]\n"
                 "    -q, --query-indices-in-device-memory   number of query indices to keep in device memory [5]\n"
                 "    -C, --target-indices-in-host-memory    number of target indices to keep in host memory [-Q]\n"
                 "    -c, --target-indices-in-device-memory  number of target indices to keep in device memory [-q]\n"
                 "    -v, --version                          version information\n"
                 "    -h, --help                             this text\n";
    std::exit(code);
}

[[noreturn]] void fail(const std::string& message)
{
    std::cerr << message << std::endl;
    std::exit(1);
}

// The two diagnostic overrides of the index size, in bases (GWAMD_DIAG=1 only):
// the command line's unit, a whole MB, is too coarse for a small input.
void read_index_size_overrides(Parameters& p)
{
    p.index_bases        = int64_t(p.index_size) * 1000000;
    p.target_index_bases = int64_t(p.target_index_size) * 1000000;
    if (const char* v = gwamd::host::diag_env("GWAMD_MAPPER_INDEX_BASES"))
        p.index_bases = std::atoll(v);
    if (const char* v = gwamd::host::diag_env("GWAMD_MAPPER_TARGET_INDEX_BASES"))
        p.target_index_bases = std::atoll(v);
}

Parameters parse(int argc, char** argv)
{
    static const option options[] = {{"kmer-size", required_argument, nullptr, 'k'},
                                     {"window-size", required_argument, nullptr, 'w'},
                                     {"num-devices", required_argument, nullptr, 'd'},
                                     {"max-cached-memory", required_argument, nullptr, 'm'},
                                     {"index-size", required_argument, nullptr, 'i'},
                                     {"target-index-size", required_argument, nullptr, 't'},
                                     {"filtering-parameter", required_argument, nullptr, 'F'},
                                     {"alignment-engines", required_argument, nullptr, 'a'},
                                     {"min-residues", required_argument, nullptr, 'r'},
                                     {"min-overlap-length", required_argument, nullptr, 'l'},
                                     {"min-bases-per-residue", required_argument, nullptr, 'b'},
                                     {"min-overlap-fraction", required_argument, nullptr, 'z'},
                                     {"rescue-overlap-ends", no_argument, nullptr, 'R'},
                                     {"drop-fused-overlaps", no_argument, nullptr, 'D'},
                                     {"query-indices-in-host-memory", required_argument, nullptr, 'Q'},
                                     {"query-indices-in-device-memory", required_argument, nullptr, 'q'},
                                     {"target-indices-in-host-memory", required_argument, nullptr, 'C'},
                                     {"target-indices-in-device-memory", required_argument, nullptr, 'c'},
                                     {"version", no_argument, nullptr, 'v'},
                                     {"help", no_argument, nullptr, 'h'},
                                     {nullptr, 0, nullptr, 0}};
    Parameters p;
    bool target_host_set = false, target_device_set = false;
    int c = 0;
    while ((c = getopt_long(argc, argv, "k:w:d:m:i:t:F:a:r:l:b:z:RDQ:q:C:c:vh", options, nullptr)) != -1)
    {
        switch (c)
        {
        case 'k': p.kmer_size = std::stoi(optarg); break;
        case 'w': p.window_size = std::stoi(optarg); break;
        case 'd': p.num_devices = std::stoi(optarg); break;
        case 'm': p.max_cached_memory = std::stoi(optarg); break;
        case 'i': p.index_size = std::stoi(optarg); break;
        case 't': p.target_index_size = std::stoi(optarg); break;
        case 'F': p.filtering_parameter = std::stod(optarg); break;
        case 'a':
            p.alignment_engines = std::stoi(optarg);
            if (p.alignment_engines < 0)
                throw std::invalid_argument("Number of alignment engines should be non-negative");
            break;
        case 'r': p.min_residues = std::stoi(optarg); break;
        case 'l': p.min_overlap_len = std::stoi(optarg); break;
        case 'b': p.min_bases_per_residue = std::stoi(optarg); break;
        case 'z': p.min_overlap_fraction = std::stof(optarg); break;
        case 'R': p.rescue = true; break;
        case 'D': p.drop_fused = true; break;
        case 'Q': p.query_host = std::stoi(optarg); break;
        case 'q': p.query_device = std::stoi(optarg); break;
        case 'C':
            p.target_host   = std::stoi(optarg);
            target_host_set = true;
            break;
        case 'c':
            p.target_device   = std::stoi(optarg);
            target_device_set = true;
            break;
        case 'v': std::cerr << "cudamapper (claragenomicsanalysis_amd, gfx950)" << std::endl; std::exit(1);
        case 'h': usage(0);
        default: std::exit(1);
        }
    }
    if (p.kmer_size < 1 || uint64_t(p.kmer_size) > Index::maximum_kmer_size())
        fail("kmer of size " + std::to_string(p.kmer_size) +
             " is not allowed, maximum k = " + std::to_string(Index::maximum_kmer_size()));
    if (p.filtering_parameter > 1.0 || p.filtering_parameter < 0.0)
        fail("-F / --filtering-parameter must be in range [0.0, 1.0]");
    if (p.max_cached_memory < 0)
        fail("-m / --max-cached-memory must not be negative");
    if (argc - optind < 2)
    {
        std::cerr << "Invalid inputs. Please refer to the help function." << std::endl;
        usage(1);
    }
    if (!target_host_set)
    {
        std::cerr << "-C / --target-indices-in-host-memory not set, using -Q / --query-indices-in-host-memory value: "
                  << p.query_host << std::endl;
        p.target_host = p.query_host;
    }
    if (!target_device_set)
    {
        std::cerr << "-c / --target-indices-in-device-memory not set, using -q / --query-indices-in-device-memory "
                     "value: "
                  << p.query_device << std::endl;
        p.target_device = p.query_device;
    }
    if (p.target_host < p.target_device)
        fail("-C / --target-indices-in-host-memory has to be larger or equal than -c / "
             "--target-indices-in-device-memory");
    if (p.query_host < p.query_device)
        fail("-Q / --query-indices-in-host-memory has to be larger or equal than -q / "
             "--query-indices-in-device-memory");
    if (p.query_device < 1 || p.target_device < 1)
        fail("the numbers of indices in host and device memory must be at least 1");
    if (p.num_devices < 1)
        fail("-d / --num-devices must be at least 1");
    p.query_path  = argv[optind];
    p.target_path = argv[optind + 1];
    if (p.query_path == p.target_path)
    {
        p.all_to_all        = true;
        p.target_index_size = p.index_size;
        std::cerr << "NOTE - Since query and target files are same, activating all_to_all mode. Query index size "
                     "used for both files."
                  << std::endl;
    }
    read_index_size_overrides(p);
    if (p.all_to_all)
        p.target_index_bases = p.index_bases;
    if (p.index_bases < 0 || p.target_index_bases < 0 || p.index_bases >= (int64_t(1) << 32) ||
        p.target_index_bases >= (int64_t(1) << 32))
        fail("-i / --index-size and -t / --target-index-size must be between 0 and 4294 MB");
    const uint32_t min_length = uint32_t(p.kmer_size + p.window_size - 1);
    p.query_parser            = io::create_kseq_fasta_parser(p.query_path, min_length);
    p.target_parser = p.all_to_all ? p.query_parser
                                   : std::shared_ptr<io::FastaParser>(io::create_kseq_fasta_parser(p.target_path, min_length));
    std::cerr << "Query file: " << p.query_path << ", number of reads: " << p.query_parser->get_num_seqences()
              << std::endl;
    std::cerr << "Target file: " << p.target_path << ", number of reads: " << p.target_parser->get_num_seqences()
              << std::endl;
    return p;
}

void check_hip(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " at " + what);
}

// the overlaps of index pairs on their way from a worker to its writers
class Queue
{
public:
    void push(std::vector<Overlap>&& overlaps)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            items_.push_back(std::move(overlaps));
        }
        cv_.notify_one();
    }
    void close()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            closed_ = true;
        }
        cv_.notify_all();
    }
    bool pop(std::vector<Overlap>& out)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return closed_ || !items_.empty(); });
        if (items_.empty())
            return false;
        out = std::move(items_.front());
        items_.pop_front();
        return true;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::vector<Overlap>> items_;
    bool closed_ = false;
};

int usable_cpus()
{
    cpu_set_t set;
    CPU_ZERO(&set);
    int n = 1;
    if (sched_getaffinity(0, sizeof(set), &set) == 0)
        n = std::max(1, CPU_COUNT(&set));
    return std::min(n, 16);
}

struct Shared
{
    const Parameters& p;
    std::vector<BatchOfIndices> batches;
    std::atomic<size_t> next{0};
    std::mutex output_mutex;
    std::mutex error_mutex;
    std::exception_ptr error;
    std::atomic<bool> failed{false};
    void fail(std::exception_ptr e)
    {
        std::lock_guard<std::mutex> lk(error_mutex);
        if (!error)
            error = e;
        failed = true;
    }
};

struct DeviceState
{
    DefaultDeviceAllocator allocator;
    std::unique_ptr<DeviceReads> query_reads, target_reads_own;
    const DeviceReads* target_reads = nullptr;
    std::mutex align_mutex; // one alignment call in flight per device
    Queue queue;
};

// fuse, rescue, align, print: one index pair at a time
void writer(int device_id, Shared& shared, DeviceState& state)
{
    try
    {
        check_hip(hipSetDevice(device_id), "hipSetDevice");
        const Parameters& p = shared.p;
        std::vector<Overlap> overlaps;
        while (state.queue.pop(overlaps))
        {
            if (shared.failed)
                continue; // drain
            Overlapper::post_process_overlaps(overlaps, p.drop_fused);
            if (p.rescue)
                Overlapper::rescue_overlap_ends(overlaps, *state.query_reads, *state.target_reads, 50, 0.5f);
            std::vector<std::string> cigars;
            if (p.alignment_engines > 0)
            {
                std::lock_guard<std::mutex> lk(state.align_mutex);
                align_overlaps(state.allocator, overlaps, *state.query_reads, *state.target_reads,
                               p.alignment_engines, cigars);
            }
            print_paf(overlaps, cigars, *p.query_parser, *p.target_parser, p.kmer_size, shared.output_mutex);
        }
    }
    catch (...)
    {
        shared.fail(std::current_exception());
        std::vector<Overlap> rest;
        while (state.queue.pop(rest))
        {
        }
    }
}

void worker(int device_id, Shared& shared)
{
    DeviceState state;
    std::vector<std::thread> writers;
    try
    {
        check_hip(hipSetDevice(device_id), "hipSetDevice");
        const Parameters& p = shared.p;
        hipStream_t stream  = nullptr;
        check_hip(hipStreamCreate(&stream), "hipStreamCreate");
        struct StreamGuard
        {
            hipStream_t s;
            ~StreamGuard() { (void)hipStreamDestroy(s); }
        } guard{stream};
        state.allocator =
            DefaultDeviceAllocator(p.max_cached_memory == 0 ? int64_t(-1) : int64_t(p.max_cached_memory) << 30);
        if (p.rescue || p.alignment_engines > 0)
        {
            state.query_reads = DeviceReads::create(state.allocator, *p.query_parser, stream);
            if (!p.all_to_all)
                state.target_reads_own = DeviceReads::create(state.allocator, *p.target_parser, stream);
            state.target_reads = p.all_to_all ? state.query_reads.get() : state.target_reads_own.get();
        }
        auto host_cache = std::make_shared<IndexCacheHost>(p.all_to_all, state.allocator, p.query_parser,
                                                           p.target_parser, p.kmer_size, p.window_size, true,
                                                           p.filtering_parameter, stream);
        IndexCacheDevice device_cache(p.all_to_all, host_cache);
        const int per_device = std::min(4, std::max(1, usable_cpus() / p.num_devices - 1));
        for (int i = 0; i < per_device; i++)
            writers.emplace_back(writer, device_id, std::ref(shared), std::ref(state));

        for (size_t b = shared.next.fetch_add(1); b < shared.batches.size() && !shared.failed;
             b        = shared.next.fetch_add(1))
        {
            std::cerr << "Device " + std::to_string(device_id) + " took batch " + std::to_string(b + 1) + " out of " +
                             std::to_string(shared.batches.size()) + " batches in total\n";
            const BatchOfIndices& batch = shared.batches[b];
            // one device batch equal to the host batch: its indices are used once, no copy to the host
            const bool skip_copy_to_host = batch.device_batches.size() == 1;
            host_cache->generate_query_cache_content(batch.host_batch.query_indices,
                                                     batch.device_batches.front().query_indices, skip_copy_to_host);
            host_cache->generate_target_cache_content(batch.host_batch.target_indices,
                                                      batch.device_batches.front().target_indices, skip_copy_to_host);
            for (const IndexBatch& device_batch : batch.device_batches)
            {
                device_cache.generate_query_cache_content(device_batch.query_indices);
                device_cache.generate_target_cache_content(device_batch.target_indices);
                for (const IndexDescriptor& q : device_batch.query_indices)
                    for (const IndexDescriptor& t : device_batch.target_indices)
                    {
                        // all-to-all: a pair whose target comes before its query is covered by its mirror
                        if (p.all_to_all && t.first_read() < q.first_read())
                            continue;
                        std::shared_ptr<Index> query_index  = device_cache.get_index_from_query_cache(q);
                        std::shared_ptr<Index> target_index = device_cache.get_index_from_target_cache(t);
                        auto matcher = Matcher::create_matcher(state.allocator, *query_index, *target_index, stream);
                        std::vector<Overlap> overlaps;
                        OverlapperTriggered overlapper(state.allocator, stream);
                        overlapper.get_overlaps(overlaps, matcher->anchors(), p.min_residues, p.min_overlap_len,
                                                p.min_bases_per_residue, p.min_overlap_fraction);
                        matcher.reset();
                        state.queue.push(std::move(overlaps));
                    }
            }
        }
        check_hip(hipStreamSynchronize(stream), "hipStreamSynchronize");
    }
    catch (...)
    {
        shared.fail(std::current_exception());
    }
    state.queue.close();
    for (std::thread& t : writers)
        t.join();
}

} // namespace

int main(int argc, char** argv)
{
    try
    {
        const Parameters p = parse(argc, argv);
        int visible        = 0;
        check_hip(hipGetDeviceCount(&visible), "hipGetDeviceCount");
        if (p.num_devices > visible)
            throw std::invalid_argument("-d / --num-devices is " + std::to_string(p.num_devices) + ", but " +
                                        std::to_string(visible) + " device(s) are visible");
        Shared shared{p};
        shared.batches = generate_batches_of_indices(p.query_host, p.query_device, p.target_host, p.target_device,
                                                     p.query_parser, p.target_parser,
                                                     number_of_basepairs_t(p.index_bases),
                                                     number_of_basepairs_t(p.target_index_bases), p.all_to_all);
        std::vector<std::thread> workers;
        for (int d = 0; d < p.num_devices; d++)
            workers.emplace_back(worker, d, std::ref(shared));
        for (std::thread& t : workers)
            t.join();
        if (shared.error)
            std::rethrow_exception(shared.error);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << "cudamapper: " << e.what() << std::endl;
        return 1;
    }
}
