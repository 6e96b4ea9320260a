// PAF output of overlaps and their CIGARs (reference
// cudamapper/src/cudamapper_utils.cpp:30-112), and the parts of the C ABI
// (include/gwamd_cudamapper.h) that only move text: gwamd_format_paf,
// gwamd_read_fasta and the gwamd_text_list a call hands its texts back in.
#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>

#include "mapper_capi.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <mutex>

namespace gm = gwamd::mapper;

namespace
{

// qname, qlen, tname, tlen: the name and the length of a read by its id
template <typename QueryName, typename QueryLen, typename TargetName, typename TargetLen>
std::string format_paf_impl(const std::vector<gm::OverlapRecord>& overlaps, const std::vector<std::string>& cigars,
                            QueryName qname, QueryLen qlen, TargetName tname, TargetLen tlen, int32_t kmer_size)
{
    if (!cigars.empty() && cigars.size() != overlaps.size())
        throw std::invalid_argument("print_paf: one CIGAR per overlap expected");
    std::string out;
    out.reserve(overlaps.size() * 150);
    char buf[256];
    for (size_t i = 0; i < overlaps.size(); i++)
    {
        const gm::OverlapRecord& o = overlaps[i];
        // cudamapper_utils.cpp:74-89: name, length, start, end, strand, name,
        // length, start, end, residues x k, longer span, mapping quality 255
        const int64_t span = std::max(std::abs(int64_t(o.target_start) - int64_t(o.target_end)),
                                      std::abs(int64_t(o.query_start) - int64_t(o.query_end)));
        out += qname(o.query_read_id);
        std::snprintf(buf, sizeof(buf), "\t%lu\t%i\t%i\t%c\t", (unsigned long)qlen(o.query_read_id),
                      int(o.query_start), int(o.query_end), o.relative_strand);
        out += buf;
        out += tname(o.target_read_id);
        std::snprintf(buf, sizeof(buf), "\t%lu\t%i\t%i\t%i\t%" PRId64 "\t%i", (unsigned long)tlen(o.target_read_id),
                      int(o.target_start), int(o.target_end), int(o.num_residues * uint32_t(kmer_size)), span, 255);
        out += buf;
        if (!cigars.empty() && !cigars[i].empty()) // no CIGAR: overlap not aligned
        {
            out += "\tcg:Z:";
            out += cigars[i];
        }
        out += '\n';
    }
    return out;
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

std::string format_paf(const std::vector<Overlap>& overlaps, const std::vector<std::string>& cigars,
                       const io::FastaParser& query_parser, const io::FastaParser& target_parser,
                       int32_t kmer_size)
{
    return format_paf_impl(
        gm::to_records(overlaps.data(), int64_t(overlaps.size())), cigars,
        [&](read_id_t id) -> const std::string& { return query_parser.get_sequence_by_id(id).name; },
        [&](read_id_t id) { return query_parser.get_sequence_by_id(id).seq.size(); },
        [&](read_id_t id) -> const std::string& { return target_parser.get_sequence_by_id(id).name; },
        [&](read_id_t id) { return target_parser.get_sequence_by_id(id).seq.size(); }, kmer_size);
}

void print_paf(const std::vector<Overlap>& overlaps, const std::vector<std::string>& cigars,
               const io::FastaParser& query_parser, const io::FastaParser& target_parser, int32_t kmer_size,
               std::mutex& write_output_mutex)
{
    const std::string text = format_paf(overlaps, cigars, query_parser, target_parser, kmer_size);
    std::lock_guard<std::mutex> lg(write_output_mutex);
    std::fwrite(text.data(), 1, text.size(), stdout);
}

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

extern "C" {

int32_t gwamd_format_paf(const char* query_names, const int64_t* query_name_offsets, const int64_t* query_lengths,
                         int32_t num_queries, const char* target_names, const int64_t* target_name_offsets,
                         const int64_t* target_lengths, int32_t num_targets, const gwamd_overlap* overlaps,
                         int32_t num_overlaps, const gwamd_text_list* cigars, int32_t kmer_size,
                         gwamd_text_list** paf)
{
    *paf = nullptr;
    return gm::guarded_map([&] {
        gm::check_offsets(query_name_offsets, num_queries, "query names");
        gm::check_offsets(target_name_offsets, num_targets, "target names");
        const std::vector<gm::OverlapRecord> ov = gm::to_records(overlaps, std::max(num_overlaps, 0));
        for (const auto& o : ov)
            if (o.relative_strand != '+' && o.relative_strand != '-')
                throw std::invalid_argument("relative_strand must be '+' or '-'");
        for (const auto& o : ov)
            if (o.query_read_id >= uint32_t(num_queries) || o.target_read_id >= uint32_t(num_targets))
                throw std::invalid_argument("overlap read id out of range");
        auto names = [](const char* base, const int64_t* off, int32_t n) {
            std::vector<std::string> v(static_cast<size_t>(n));
            for (int32_t i = 0; i < n; i++)
                v[size_t(i)].assign(base + off[i], size_t(off[i + 1] - off[i]));
            return v;
        };
        const auto qn = names(query_names, query_name_offsets, num_queries);
        const auto tn = names(target_names, target_name_offsets, num_targets);
        static const std::vector<std::string> none;
        auto list = std::make_unique<gwamd_text_list>();
        list->items.push_back(format_paf_impl(
            ov, cigars ? cigars->items : none, [&](uint32_t i) -> const std::string& { return qn[i]; },
            [&](uint32_t i) { return size_t(query_lengths[i]); },
            [&](uint32_t i) -> const std::string& { return tn[i]; },
            [&](uint32_t i) { return size_t(target_lengths[i]); }, kmer_size));
        *paf = list.release();
        return 0;
    });
}

namespace
{

// qualities: null for gwamd_read_fasta
int32_t read_fasta(const char* path, uint32_t min_sequence_length, int32_t shuffle, gwamd_text_list** names,
                   gwamd_text_list** sequences, gwamd_text_list** qualities)
{
    return gm::guarded_map([&] {
        namespace io = claraparabricks::genomeworks::io;
        auto parser  = io::create_kseq_fasta_parser(path ? path : "", min_sequence_length, shuffle != 0);
        auto nl      = std::make_unique<gwamd_text_list>();
        auto sl      = std::make_unique<gwamd_text_list>();
        auto ql      = std::make_unique<gwamd_text_list>();
        for (uint32_t i = 0; i < parser->get_num_seqences(); i++)
        {
            const auto& r = parser->get_sequence_by_id(i);
            nl->items.push_back(r.name);
            sl->items.push_back(r.seq);
            if (qualities)
                ql->items.push_back(parser->get_quality_by_id(i));
        }
        *names     = nl.release();
        *sequences = sl.release();
        if (qualities)
            *qualities = ql.release();
        return 0;
    });
}

} // namespace

int32_t gwamd_read_fasta(const char* path, uint32_t min_sequence_length, int32_t shuffle, gwamd_text_list** names,
                         gwamd_text_list** sequences)
{
    *names     = nullptr;
    *sequences = nullptr;
    return read_fasta(path, min_sequence_length, shuffle, names, sequences, nullptr);
}

int32_t gwamd_read_fasta_with_qualities(const char* path, uint32_t min_sequence_length, int32_t shuffle,
                                        gwamd_text_list** names, gwamd_text_list** sequences,
                                        gwamd_text_list** qualities)
{
    if (!names || !sequences || !qualities)
        return gm::guarded_map([]() -> int32_t { throw std::invalid_argument("an output list is NULL"); });
    *names = *sequences = *qualities = nullptr;
    return read_fasta(path, min_sequence_length, shuffle, names, sequences, qualities);
}

int32_t gwamd_text_list_create(const char* const* texts, const int64_t* lengths, int32_t n, gwamd_text_list** out)
{
    *out = nullptr;
    return gm::guarded_map([&] {
        if (n < 0 || (n > 0 && (!texts || !lengths)))
            throw std::invalid_argument("text list: bad count or pointers");
        auto list = std::make_unique<gwamd_text_list>();
        list->items.resize(static_cast<size_t>(n));
        for (int32_t i = 0; i < n; i++)
        {
            if (lengths[i] < 0)
                throw std::invalid_argument("text list: negative length");
            list->items[size_t(i)].assign(texts[i], size_t(lengths[i]));
        }
        *out = list.release();
        return 0;
    });
}

int32_t gwamd_text_list_size(const gwamd_text_list* list) { return list ? int32_t(list->items.size()) : 0; }

int32_t gwamd_text_list_get(const gwamd_text_list* list, int32_t i, const char** text, int64_t* length)
{
    if (!list || i < 0 || i >= int32_t(list->items.size()))
        return GWAMD_E_INVALID_ARGUMENT;
    *text   = list->items[size_t(i)].data();
    *length = int64_t(list->items[size_t(i)].size());
    return 0;
}

void gwamd_text_list_free(gwamd_text_list* list) { delete list; }

} // extern "C"
