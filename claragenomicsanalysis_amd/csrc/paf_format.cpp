// PAF output of overlaps and their CIGARs (reference
// cudamapper/src/cudamapper_utils.cpp:30-112), and the parts of the C ABI
// (include/gwamd_cudamapper.h) that only move text: gwamd_format_paf,
// gwamd_read_fasta and the gwamd_text_list a call hands its texts back in.
// The way back (include/gwamd_polish.h, cudapolish/windows.hpp): CIGAR text
// as packed ops (gwamd_cigar_ops) and PAF text as overlaps and their ops
// (gwamd_read_paf), for the cut from CIGAR runs.
#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>

#include "../../include/gwamd_polish.h"
#include "mapper_capi.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <mutex>
#include <unordered_map>

namespace gm = gwamd::mapper;

// what gwamd_read_paf read
struct gwamd_paf
{
    std::vector<gwamd_overlap> overlaps;
    std::vector<uint32_t> ops;
    std::vector<int64_t> op_offsets{0};
};

namespace
{

// The ops of CIGAR text, appended to out
void parse_cigar(const char* text, size_t length, std::vector<uint32_t>& out)
{
    static const char letters[] = "MIDNSHP=X"; // BAM numbering
    size_t i                    = 0;
    while (i < length)
    {
        uint64_t value = 0;
        size_t digits  = 0;
        for (; i < length && text[i] >= '0' && text[i] <= '9'; i++, digits++)
        {
            value = value * 10 + uint64_t(text[i] - '0');
            if (value >= (uint64_t(1) << 28))
                throw std::invalid_argument("CIGAR: a length of 2^28 or more");
        }
        if (i == length)
            throw std::invalid_argument("CIGAR: digits at the end");
        const void* at = std::memchr(letters, text[i], sizeof(letters) - 1);
        if (!at)
            throw std::invalid_argument("CIGAR: unknown letter at character " + std::to_string(i));
        if (digits == 0)
            throw std::invalid_argument("CIGAR: a letter without a number at character " + std::to_string(i));
        out.push_back(uint32_t(value << 4) | uint32_t(static_cast<const char*>(at) - letters));
        i++;
    }
}

using NameIds = std::unordered_map<std::string, uint32_t>;

// a column that is a number below 2^32 and nothing else
uint32_t paf_number(const std::string& column, const char* what)
{
    uint64_t value = 0;
    if (column.empty())
        throw std::invalid_argument(std::string(what) + " is empty");
    for (char c : column)
    {
        if (c < '0' || c > '9')
            throw std::invalid_argument(std::string(what) + " is not a number: " + column);
        value = value * 10 + uint64_t(c - '0');
        if (value >= (uint64_t(1) << 32))
            throw std::invalid_argument(std::string(what) + " is 2^32 or more");
    }
    return uint32_t(value);
}

void parse_paf_line(const std::string& line, const NameIds& query_ids, const NameIds& target_ids, int32_t kmer_size,
                    gwamd_paf& out)
{
    std::vector<std::string> columns;
    for (size_t at = 0;;)
    {
        const size_t tab = line.find('\t', at);
        columns.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at));
        if (tab == std::string::npos)
            break;
        at = tab + 1;
    }
    if (columns.size() < 12)
        throw std::invalid_argument("fewer than 12 columns");
    const auto query = query_ids.find(columns[0]), target = target_ids.find(columns[5]);
    if (query == query_ids.end())
        throw std::invalid_argument("unknown query name " + columns[0]);
    if (target == target_ids.end())
        throw std::invalid_argument("unknown target name " + columns[5]);
    if (columns[4] != "+" && columns[4] != "-")
        throw std::invalid_argument("the strand is neither + nor -");
    gwamd_overlap o{};
    o.query_read_id  = query->second;
    o.target_read_id = target->second;
    o.query_start    = paf_number(columns[2], "query start");
    o.query_end      = paf_number(columns[3], "query end");
    o.target_start   = paf_number(columns[7], "target start");
    o.target_end     = paf_number(columns[8], "target end");
    if (o.query_start > o.query_end || o.target_start > o.target_end)
        throw std::invalid_argument("start > end");
    if (o.query_end > paf_number(columns[1], "query length") || o.target_end > paf_number(columns[6], "target length"))
        throw std::invalid_argument("an end beyond its read's length");
    o.relative_strand  = static_cast<unsigned char>(columns[4][0]);
    o.num_residues     = paf_number(columns[9], "column 10") / uint32_t(kmer_size);
    o.overlap_complete = 0;
    out.overlaps.push_back(o);
    for (size_t c = 12; c < columns.size(); c++)
        if (columns[c].compare(0, 5, "cg:Z:") == 0)
        {
            parse_cigar(columns[c].data() + 5, columns[c].size() - 5, out.ops);
            break;
        }
    out.op_offsets.push_back(int64_t(out.ops.size()));
}

std::unique_ptr<gwamd_paf> parse_paf(const char* text, size_t length, const NameIds& query_ids,
                                     const NameIds& target_ids, int32_t kmer_size)
{
    if (kmer_size < 1)
        throw std::invalid_argument("kmer_size must be at least 1");
    auto out       = std::make_unique<gwamd_paf>();
    int64_t number = 0;
    for (size_t at = 0; at < length;)
    {
        const void* nl   = std::memchr(text + at, '\n', length - at);
        const size_t end = nl ? size_t(static_cast<const char*>(nl) - text) : length;
        std::string line(text + at, end - at);
        at = end + 1;
        number++;
        if (!line.empty() && line.back() == '\r')
            line.pop_back();
        if (line.empty())
            continue;
        try
        {
            parse_paf_line(line, query_ids, target_ids, kmer_size, *out);
        }
        catch (const std::invalid_argument& e)
        {
            throw std::invalid_argument("PAF line " + std::to_string(number) + ": " + e.what());
        }
    }
    return out;
}

NameIds name_ids(const char* names, const int64_t* offsets, int32_t n, const char* what)
{
    gm::check_offsets(offsets, n, what);
    if (n > 0 && offsets[n] > 0 && !names)
        throw std::invalid_argument(std::string(what) + " is NULL");
    NameIds ids;
    for (int32_t i = 0; i < n; i++)
        ids.emplace(std::string(names + offsets[i], size_t(offsets[i + 1] - offsets[i])), uint32_t(i));
    return ids;
}

NameIds name_ids(const claraparabricks::genomeworks::io::FastaParser& parser)
{
    NameIds ids;
    for (uint32_t i = 0; i < uint32_t(parser.get_num_seqences()); i++)
        ids.emplace(parser.get_sequence_by_id(i).name, i);
    return ids;
}

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

namespace cudapolish
{

std::vector<uint32_t> cigar_ops(const std::string& text)
{
    std::vector<uint32_t> ops;
    parse_cigar(text.data(), text.size(), ops);
    return ops;
}

PafOverlaps read_paf(const std::string& text, const io::FastaParser& query_parser,
                     const io::FastaParser& target_parser, int32_t kmer_size)
{
    const std::unique_ptr<gwamd_paf> paf =
        parse_paf(text.data(), text.size(), name_ids(query_parser), name_ids(target_parser), kmer_size);
    PafOverlaps out;
    for (size_t i = 0; i < paf->overlaps.size(); i++)
    {
        out.overlaps.push_back(gm::overlap_as<cudamapper::Overlap>(paf->overlaps[i]));
        out.cigars.emplace_back(paf->ops.begin() + paf->op_offsets[i], paf->ops.begin() + paf->op_offsets[i + 1]);
    }
    return out;
}

} // namespace cudapolish
} // namespace genomeworks
} // namespace claraparabricks

// ---- C ABI ------------------------------------------------------------------

extern "C" {

int32_t gwamd_cigar_ops(const char* text, int64_t text_length, uint32_t* out_or_null, int64_t capacity,
                        int64_t* num_ops)
{
    if (num_ops)
        *num_ops = 0;
    return gm::guarded_map([&] {
        if (!num_ops)
            throw std::invalid_argument("num_ops is NULL");
        if (text_length < 0 || (text_length > 0 && !text))
            throw std::invalid_argument("CIGAR: negative length or NULL text");
        std::vector<uint32_t> ops;
        parse_cigar(text, size_t(text_length), ops);
        *num_ops = int64_t(ops.size());
        if (out_or_null)
        {
            if (capacity < int64_t(ops.size()))
                throw std::invalid_argument("CIGAR: " + std::to_string(ops.size()) + " ops for a capacity of " +
                                            std::to_string(capacity));
            std::copy(ops.begin(), ops.end(), out_or_null);
        }
        return int32_t(0);
    });
}

int32_t gwamd_read_paf(const char* path_or_null, const char* text_or_null, int64_t text_length,
                       const char* query_names, const int64_t* query_name_offsets, int32_t num_queries,
                       const char* target_names, const int64_t* target_name_offsets, int32_t num_targets,
                       int32_t kmer_size, gwamd_paf** handle_out)
{
    if (handle_out)
        *handle_out = nullptr;
    return gm::guarded_map([&] {
        if (!handle_out)
            throw std::invalid_argument("handle_out is NULL");
        if ((path_or_null != nullptr) == (text_or_null != nullptr))
            throw std::invalid_argument("read_paf: one of path and text expected");
        if (text_or_null && text_length < 0)
            throw std::invalid_argument("read_paf: negative text_length");
        const NameIds query_ids  = name_ids(query_names, query_name_offsets, num_queries, "query names");
        const NameIds target_ids = name_ids(target_names, target_name_offsets, num_targets, "target names");
        std::string file;
        if (path_or_null)
        {
            std::ifstream in(path_or_null, std::ios::binary);
            if (!in)
                throw std::runtime_error(std::string("read_paf: cannot open ") + path_or_null);
            file.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
        }
        *handle_out = parse_paf(path_or_null ? file.data() : text_or_null,
                                path_or_null ? file.size() : size_t(text_length), query_ids, target_ids, kmer_size)
                          .release();
        return int32_t(0);
    });
}

int32_t gwamd_paf_get(const gwamd_paf* paf, gwamd_paf_view* view)
{
    return gm::guarded_map([&] {
        if (!paf || !view)
            throw std::invalid_argument("paf or view is NULL");
        view->num_overlaps = int64_t(paf->overlaps.size());
        view->num_ops      = int64_t(paf->ops.size());
        view->overlaps     = paf->overlaps.data();
        view->ops          = paf->ops.data();
        view->op_offsets   = paf->op_offsets.data();
        return int32_t(0);
    });
}

void gwamd_paf_free(gwamd_paf* paf) { delete paf; }

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
