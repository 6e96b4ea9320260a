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
    explicit FastaParserMem(std::vector<FastaSequence> reads)
        : reads_(std::move(reads))
    {
    }
    number_of_reads_t get_num_seqences() const override { return number_of_reads_t(reads_.size()); }
    const FastaSequence& get_sequence_by_id(read_id_t sequence_id) const override
    {
        return reads_.at(sequence_id);
    }

private:
    std::vector<FastaSequence> reads_;
};

std::string first_word(const std::string& header)
{
    const size_t end = header.find_first_of(" \t\r");
    return header.substr(1, end == std::string::npos ? std::string::npos : end - 1);
}

// FASTA and FASTQ records as kseq reads them: '>' or '@' header, sequence
// lines up to the next header ('+' separator and quality lines for FASTQ)
std::vector<FastaSequence> read_records(const std::string& path)
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
            if (fastq)
            {
                // sequence lines up to '+', then as many quality characters
                while (std::getline(in, line) && !(line.size() && line[0] == '+'))
                {
                    if (!line.empty() && line.back() == '\r')
                        line.pop_back();
                    out.back().seq += line;
                }
                size_t qual = 0;
                while (qual < out.back().seq.size() && std::getline(in, line))
                    qual += line.size() - (line.size() && line.back() == '\r' ? 1 : 0);
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
    std::vector<FastaSequence> all = read_records(fasta_file);
    std::vector<FastaSequence> kept;
    kept.reserve(all.size());
    for (auto& r : all)
        if (number_of_basepairs_t(r.seq.size()) >= min_sequence_length)
            kept.push_back(std::move(r));
    if (shuffle) // kseqpp_fasta_parser.cpp:58-63: deterministic order
    {
        std::mt19937 g(0);
        std::shuffle(kept.begin(), kept.end(), g);
    }
    return std::make_unique<FastaParserMem>(std::move(kept));
}

std::unique_ptr<FastaParser> create_fasta_parser_from_sequences(std::vector<FastaSequence> records)
{
    return std::make_unique<FastaParserMem>(std::move(records));
}

} // namespace io
} // namespace genomeworks
} // namespace claraparabricks
