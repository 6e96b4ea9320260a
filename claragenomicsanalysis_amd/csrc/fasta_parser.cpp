// The FASTA/FASTQ reader behind io::FastaParser (reference
// common/io/src/kseqpp_fasta_parser.cpp:31-72): the whole file is read into
// memory, filtered by length and, on request, shuffled in a fixed order.
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>

#include <algorithm>
#include <fstream>
#include <random>
#include <stdexcept>

namespace claraparabricks
{
namespace genomeworks
{
namespace io
{
namespace
{

class FastaParserMem : public FastaParser
{
public:
    explicit FastaParserMem(std::vector<FastaSequence> reads, std::vector<std::string> qualities = {})
        : reads_(std::move(reads))
        , qualities_(std::move(qualities))
    {
        if (!qualities_.empty() && qualities_.size() != reads_.size())
            throw std::invalid_argument("one quality string per record expected");
    }
    number_of_reads_t get_num_seqences() const override { return number_of_reads_t(reads_.size()); }
    const FastaSequence& get_sequence_by_id(read_id_t sequence_id) const override
    {
        return reads_.at(sequence_id);
    }
    const std::string& get_quality_by_id(read_id_t sequence_id) const override
    {
        if (qualities_.empty())
            return FastaParser::get_quality_by_id(sequence_id);
        return qualities_.at(sequence_id);
    }

private:
    std::vector<FastaSequence> reads_;
    std::vector<std::string> qualities_; // empty, or one per record
};

std::string first_word(const std::string& header)
{
    const size_t end = header.find_first_of(" \t\r");
    return header.substr(1, end == std::string::npos ? std::string::npos : end - 1);
}

// FASTA and FASTQ records as kseq reads them: '>' or '@' header, sequence
// lines up to the next header ('+' separator and quality lines for FASTQ).
// qualities receives one string per record, empty for a FASTA record.
std::vector<FastaSequence> read_records(const std::string& path, std::vector<std::string>& qualities)
{
    std::ifstream in(path);
    if (!in.good())
        throw std::invalid_argument("Error: non-existent or empty file " + path + " !");
    std::vector<FastaSequence> out;
    std::string line;
    bool fastq = false;
    while (std::getline(in, line))
    {
        if (!line.empty() && line.back() == '\r')
            line.pop_back();
        if (line.empty())
            continue;
        if (line[0] == '>' || line[0] == '@')
        {
            fastq = line[0] == '@';
            out.push_back(FastaSequence{first_word(line), std::string()});
            qualities.emplace_back();
            if (fastq)
            {
                // sequence lines up to '+', then as many quality characters
                while (std::getline(in, line) && !(line.size() && line[0] == '+'))
                {
                    if (!line.empty() && line.back() == '\r')
                        line.pop_back();
                    out.back().seq += line;
                }
                std::string& qual = qualities.back();
                while (qual.size() < out.back().seq.size() && std::getline(in, line))
                    qual.append(line, 0, line.size() - (line.size() && line.back() == '\r' ? 1 : 0));
            }
        }
        else if (!out.empty() && !fastq)
            out.back().seq += line;
    }
    if (out.empty())
        throw std::invalid_argument("Error: non-existent or empty file " + path + " !");
    return out;
}

} // namespace

std::unique_ptr<FastaParser> create_kseq_fasta_parser(const std::string& fasta_file,
                                                      number_of_basepairs_t min_sequence_length, bool shuffle)
{
    std::vector<std::string> all_qualities;
    std::vector<FastaSequence> all = read_records(fasta_file, all_qualities);
    std::vector<size_t> kept;
    kept.reserve(all.size());
    for (size_t i = 0; i < all.size(); i++)
        if (number_of_basepairs_t(all[i].seq.size()) >= min_sequence_length)
            kept.push_back(i);
    if (shuffle) // kseqpp_fasta_parser.cpp:58-63: deterministic order
    {
        // the permutation std::shuffle gives the records themselves: it looks at positions only
        std::mt19937 g(0);
        std::shuffle(kept.begin(), kept.end(), g);
    }
    std::vector<FastaSequence> reads;
    std::vector<std::string> qualities;
    reads.reserve(kept.size());
    qualities.reserve(kept.size());
    for (size_t i : kept)
    {
        reads.push_back(std::move(all[i]));
        qualities.push_back(std::move(all_qualities[i]));
    }
    return std::make_unique<FastaParserMem>(std::move(reads), std::move(qualities));
}

std::unique_ptr<FastaParser> create_fasta_parser_from_sequences(std::vector<FastaSequence> records,
                                                                std::vector<std::string> qualities)
{
    if (qualities.size() != records.size())
        throw std::invalid_argument("one quality string per record expected");
    return std::make_unique<FastaParserMem>(std::move(records), std::move(qualities));
}

std::unique_ptr<FastaParser> create_fasta_parser_from_sequences(std::vector<FastaSequence> records)
{
    return std::make_unique<FastaParserMem>(std::move(records));
}

} // namespace io
} // namespace genomeworks
} // namespace claraparabricks
