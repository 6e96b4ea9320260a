// Scenarios of the index caches, the host copy of an index and the aligner's
// device-added batches, run on the GPU by tests/test_index_cache_gpu.py, which
// compiles this file against the public headers and libgwamd.so.  Expected
// index contents are those of Index::create_index on the same read range in
// this process (pinned by tests/test_mapper_gpu.py), array by array and getter
// by getter.  Prints "ok <scenario>" per scenario; the first failure ends the
// program with a message and status 1.
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>
#include <claraparabricks/genomeworks/cudamapper/device_reads.hpp>
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_cache.hpp>
#include <claraparabricks/genomeworks/cudamapper/index_descriptor.hpp>
#include <claraparabricks/genomeworks/cudamapper/matcher.hpp>

#include "aligner_resident.hpp" // internal: the aligner's device-add entry (csrc/)

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudamapper;

#define CHECK(cond)                                                                  \
    do                                                                               \
    {                                                                                \
        if (!(cond))                                                                 \
        {                                                                            \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

namespace
{

constexpr std::uint64_t K = 3, W = 2;

template <typename T>
std::vector<T> to_host(const device_buffer<T>& d)
{
    std::vector<T> h(static_cast<size_t>(d.size()));
    if (!h.empty())
        CHECK(hipMemcpy(h.data(), d.data(), h.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    return h;
}

struct Content
{
    std::vector<representation_t> representations, unique_representations;
    std::vector<read_id_t> read_ids;
    std::vector<position_in_read_t> positions_in_reads;
    std::vector<SketchElement::DirectionOfRepresentation> directions_of_reads;
    std::vector<std::uint32_t> first_occurrence_of_representations;
    read_id_t number_of_reads;
    position_in_read_t longest;
    bool arrays_equal(const Content& o) const
    {
        return representations == o.representations && unique_representations == o.unique_representations &&
               read_ids == o.read_ids && positions_in_reads == o.positions_in_reads &&
               directions_of_reads == o.directions_of_reads &&
               first_occurrence_of_representations == o.first_occurrence_of_representations &&
               number_of_reads == o.number_of_reads && longest == o.longest;
    }
};

Content content_of(const Index& index)
{
    return {to_host(index.representations()),
            to_host(index.unique_representations()),
            to_host(index.read_ids()),
            to_host(index.positions_in_reads()),
            to_host(index.directions_of_reads()),
            to_host(index.first_occurrence_of_representations()),
            index.number_of_reads(),
            index.number_of_basepairs_in_longest_read()};
}

Content content_of(const IndexHostCopyBase& copy)
{
    return {copy.representations(),
            copy.unique_representations(),
            copy.read_ids(),
            copy.positions_in_reads(),
            copy.directions_of_reads(),
            copy.first_occurrence_of_representations(),
            copy.number_of_reads(),
            copy.number_of_basepairs_in_longest_read()};
}

// every array and every getter
bool same_index(const Index& a, const Index& b)
{
    return content_of(a).arrays_equal(content_of(b)) && a.smallest_read_id() == b.smallest_read_id() &&
           a.largest_read_id() == b.largest_read_id();
}

std::unique_ptr<Index> direct(const io::FastaParser& parser, const IndexDescriptor& d)
{
    return Index::create_index(DefaultDeviceAllocator(), parser, d.first_read(), d.first_read() + d.number_of_reads(),
                               K, W);
}

template <typename F>
bool throws_out_of_range(F&& f)
{
    try
    {
        f();
    }
    catch (const std::out_of_range&)
    {
        return true;
    }
    return false;
}

std::vector<Anchor> anchors_of(const Index& q, const Index& t)
{
    auto matcher = Matcher::create_matcher(DefaultDeviceAllocator(), q, t);
    return to_host(matcher->anchors());
}

bool same_anchors(const std::vector<Anchor>& a, const std::vector<Anchor>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].query_read_id_ != b[i].query_read_id_ || a[i].target_read_id_ != b[i].target_read_id_ ||
            a[i].query_position_in_read_ != b[i].query_position_in_read_ ||
            a[i].target_position_in_read_ != b[i].target_position_in_read_)
            return false;
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    CHECK(argc == 3);
    std::shared_ptr<io::FastaParser> query_parser  = io::create_kseq_fasta_parser(argv[1], 1, false);
    std::shared_ptr<io::FastaParser> target_parser = io::create_kseq_fasta_parser(argv[2], 1, false);
    CHECK(query_parser->get_num_seqences() == 2 && target_parser->get_num_seqences() == 2);
    const IndexDescriptor d0(0, 1), d1(1, 1), d01(0, 2), missing(0, 3);
    DefaultDeviceAllocator allocator;
    auto q0 = direct(*query_parser, d0), q1 = direct(*query_parser, d1), q01 = direct(*query_parser, d01);
    auto t0 = direct(*target_parser, d0), t1 = direct(*target_parser, d1);
    CHECK(content_of(*q0).representations.size() > 1 && !same_index(*q0, *q1) && !same_index(*q0, *t0));

    // ---- the host copy of an index
    {
        auto copy = IndexHostCopyBase::create_cache(*q01, 0, K, W);
        CHECK(content_of(*copy).arrays_equal(content_of(*q01)));
        CHECK(copy->first_read_id() == 0 && copy->kmer_size() == K && copy->window_size() == W);
        CHECK(copy->number_of_reads() == 2 && copy->number_of_basepairs_in_longest_read() == 7);
        DefaultDeviceAllocator pool(int64_t(1) << 20);
        CHECK(pool.budget()->used() == 0);
        {
            auto back = copy->copy_index_to_device(pool);
            CHECK(same_index(*back, *q01));
            // the six arrays count against the pool while the index lives
            const int64_t n = int64_t(copy->representations().size()), u = int64_t(copy->unique_representations().size());
            CHECK(pool.budget()->used() == n * (8 + 4 + 4 + 1) + u * 8 + (u + 1) * 4);
            // matching the copied-back index gives the anchors of the original
            auto t01 = direct(*target_parser, d01);
            const std::vector<Anchor> want = anchors_of(*q01, *t01);
            CHECK(!want.empty() && same_anchors(anchors_of(*back, *t01), want));
            auto target_back = IndexHostCopyBase::create_cache(*t01, 0, K, W)->copy_index_to_device(pool);
            CHECK(same_anchors(anchors_of(*back, *target_back), want));
        }
        CHECK(pool.budget()->used() == 0);
        // a second index from the same copy, and a copy of a later range
        CHECK(same_index(*copy->copy_index_to_device(allocator), *q01));
        auto later = IndexHostCopyBase::create_cache(*q1, 1, K, W);
        CHECK(later->first_read_id() == 1 && same_index(*later->copy_index_to_device(allocator), *q1));
        // an empty index round-trips
        auto empty      = Index::create_index(allocator, *query_parser, 0, 0, K, W);
        auto empty_copy = IndexHostCopyBase::create_cache(*empty, 0, K, W);
        CHECK(empty_copy->representations().empty() && empty_copy->first_occurrence_of_representations().empty());
        auto empty_back = empty_copy->copy_index_to_device(pool);
        CHECK(same_index(*empty_back, *empty) && empty_back->number_of_reads() == 0 && pool.budget()->used() == 0);
        CHECK(anchors_of(*empty_back, *q0).empty());
        std::printf("ok host_copy\n");
    }

    // ---- host cache, query and target not the same
    {
        IndexCacheHost cache(false, allocator, query_parser, target_parser, K, W);
        cache.generate_query_cache_content({d0, d1});
        cache.generate_target_cache_content({d0});
        CHECK(same_index(*cache.get_index_from_query_cache(d0), *q0));
        CHECK(same_index(*cache.get_index_from_query_cache(d1), *q1));
        CHECK(same_index(*cache.get_index_from_target_cache(d0), *t0));
        CHECK(throws_out_of_range([&] { cache.get_index_from_target_cache(d1); }));
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(missing); }));
        // a fetch is a fresh copy each time
        CHECK(cache.get_index_from_query_cache(d0) != cache.get_index_from_query_cache(d0));
        // new content: what is no longer named is gone, what is named again is kept
        cache.generate_query_cache_content({d1, d01});
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(d0); }));
        CHECK(same_index(*cache.get_index_from_query_cache(d1), *q1));
        CHECK(same_index(*cache.get_index_from_query_cache(d01), *q01));
        cache.generate_target_cache_content({d1});
        CHECK(same_index(*cache.get_index_from_target_cache(d1), *t1));
        std::printf("ok host_cache_not_the_same\n");
    }

    // ---- host cache, the same query and target; keep on device; skip_copy_to_host
    {
        IndexCacheHost cache(true, allocator, query_parser, query_parser, K, W);
        cache.generate_query_cache_content({d0, d1}, {d0});
        cache.generate_target_cache_content({d0, d1}, {d0, d1});
        // d0 is kept on the device by both sides: one object, handed out once per side
        auto from_query  = cache.get_index_from_query_cache(d0);
        auto from_target = cache.get_index_from_target_cache(d0);
        CHECK(from_query == from_target && same_index(*from_query, *q0));
        auto again = cache.get_index_from_query_cache(d0);
        CHECK(again != from_query && same_index(*again, *q0));
        // d1 was kept by the target side only
        auto kept = cache.get_index_from_target_cache(d1);
        CHECK(same_index(*kept, *q1) && same_index(*cache.get_index_from_query_cache(d1), *q1));
        CHECK(cache.get_index_from_target_cache(d1) != kept);
        // no host copy: the index kept on the device is the only one
        cache.generate_query_cache_content({d01}, {d01}, true);
        CHECK(same_index(*cache.get_index_from_query_cache(d01), *q01));
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(d01); }));
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(d0); }));
        CHECK(same_index(*cache.get_index_from_target_cache(d0), *q0)); // the other side is untouched
        std::printf("ok host_cache_the_same\n");
    }

    // ---- device cache
    for (const bool same : {false, true})
    {
        auto host = std::make_shared<IndexCacheHost>(same, allocator, query_parser,
                                                     same ? query_parser : target_parser, K, W);
        host->generate_query_cache_content({d0, d1});
        host->generate_target_cache_content({d0, d1});
        IndexCacheDevice cache(same, host);
        cache.generate_query_cache_content({d0});
        auto first = cache.get_index_from_query_cache(d0);
        CHECK(same_index(*first, *q0) && cache.get_index_from_query_cache(d0) == first);
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(d1); }));
        CHECK(throws_out_of_range([&] { cache.get_index_from_target_cache(d0); }));
        // a second generate keeps what it can: the same object
        cache.generate_query_cache_content({d0, d1});
        CHECK(cache.get_index_from_query_cache(d0) == first && same_index(*cache.get_index_from_query_cache(d1), *q1));
        cache.generate_target_cache_content({d0, d1});
        auto target0 = cache.get_index_from_target_cache(d0);
        CHECK(same_index(*target0, same ? *q0 : *t0) && same_index(*cache.get_index_from_target_cache(d1), same ? *q1 : *t1));
        // the same query and target share the object, two parsers do not
        CHECK((target0 == first) == same);
        cache.generate_query_cache_content({d1});
        CHECK(throws_out_of_range([&] { cache.get_index_from_query_cache(d0); }));
        std::printf("ok device_cache_%s\n", same ? "the_same" : "not_the_same");
    }

    // ---- the aligner: device-added and host-added batches
    {
        namespace ca = cudaaligner;
        std::mt19937 rng(5);
        auto random_read = [&](int n) {
            std::string s;
            for (int i = 0; i < n; i++)
                s += "ACGT"[rng() % 4];
            return s;
        };
        const std::string a = random_read(300);
        std::string b       = a.substr(20, 250);
        b[100]              = b[100] == 'A' ? 'C' : 'A';
        b.erase(40, 3);
        auto reads_parser = io::create_fasta_parser_from_sequences({{"a", a}, {"b", b}});
        auto reads        = DeviceReads::create(allocator, *reads_parser);
        CHECK(reads->number_of_reads() == 2 && reads->number_of_basepairs() == int64_t(a.size() + b.size()));
        const gwamd::mapper::DeviceReads& resident = *reads->impl().reads;
        // read 0 [20, 270) against read 1, forward; and read 1 against the reverse complement of itself
        const gwamd::mapper::OverlapRecord overlaps[2] = {
            {0, 1, 20, 0, 270, uint32_t(b.size()), '+', 0, 0}, {1, 1, 5, 5, 205, 205, '-', 0, 0}};
        gwamd::mapper::check_overlaps(resident, resident, overlaps, 2);
        auto aligner = ca::create_aligner(300, 300, 4, ca::AlignmentType::global_alignment, allocator, nullptr, 0);
        auto cigars  = [&] {
            CHECK(aligner->align_all() == ca::StatusType::success);
            CHECK(aligner->sync_alignments() == ca::StatusType::success);
            std::vector<std::string> out;
            for (const auto& alignment : aligner->get_alignments())
                out.push_back(alignment->convert_to_cigar());
            return out;
        };
        // a batch is all host-added or all device-added
        CHECK(aligner->add_alignment(a.data() + 20, 250, b.data(), int32_t(b.size())) == ca::StatusType::success);
        CHECK(gwamd::aln::add_device_overlaps(*aligner, resident, resident, overlaps, 2) ==
              ca::StatusType::generic_error);
        CHECK(aligner->get_alignments().size() == 1);
        aligner->reset();
        CHECK(gwamd::aln::add_device_overlaps(*aligner, resident, resident, overlaps, 2) == ca::StatusType::success);
        CHECK(aligner->add_alignment(a.data(), 10, b.data(), 10) == ca::StatusType::generic_error);
        CHECK(aligner->get_alignments().size() == 2 && aligner->get_alignments()[0]->get_query_sequence().empty());
        const std::vector<std::string> from_device = cigars();
        CHECK(from_device.size() == 2 && !from_device[0].empty() && !from_device[1].empty());
        // all or none: a range that does not fit adds nothing
        const gwamd::mapper::OverlapRecord three[3] = {overlaps[0], overlaps[1], overlaps[0]};
        CHECK(gwamd::aln::add_device_overlaps(*aligner, resident, resident, three, 3) ==
              ca::StatusType::exceeded_max_alignments);
        CHECK(aligner->get_alignments().size() == 2);
        // after reset() the same aligner takes a host-added batch: the same pairs, the same CIGARs
        aligner->reset();
        CHECK(aligner->add_alignment(a.data() + 20, 250, b.data(), int32_t(b.size())) == ca::StatusType::success);
        CHECK(aligner->add_alignment(b.data() + 5, 200, b.data() + 5, 200, false, true) == ca::StatusType::success);
        const std::vector<std::string> from_host = cigars();
        CHECK(from_host == from_device);
        CHECK(!aligner->get_alignments()[0]->get_query_sequence().empty());
        // and a device-added one again
        aligner->reset();
        CHECK(gwamd::aln::add_device_overlaps(*aligner, resident, resident, overlaps + 1, 1) ==
              ca::StatusType::success);
        CHECK(cigars() == std::vector<std::string>{from_device[1]});
        std::printf("ok aligner_batches\n");
    }
    return 0;
}
