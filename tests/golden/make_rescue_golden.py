"""Writes tests/golden/rescue_kat.json: the known answers the reference's own
tests hold for the overlap-end rescue.  The data below was transcribed from
the cited reference test files; no reference source is reproduced.  Re-run
with ``python tests/golden/make_rescue_golden.py`` (needs no GPU and no
reference tree).
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# cudamapper/tests/Test_CudamapperOverlapper.cpp:24-78
# (TestOverlapExtension.short_forward_head_overlap_properly_extended): two
# sequences of 1,000 bases, query[0:660] == target[340:1000]
QUERY = (
    "ACCGCCACCAATATCCATGTGACCTCGCACGGTACGGAATTTACCCTACAAACCCCAACCGGTAGCGTCGATGTTCTGCTGCCGTTGCCGGGGCGTCACA"
    "ATATTGCGAATGCGCTGGCAGCCGCTGCGCTCTCCATGTCCGTGGGCGCAACGCTTGATGCTATCAAAGCGGGGCTGGCAAATCTGAAAGCTGTTCCAGG"
    "CCGTCTGTTCCCCATCCAACTGGCAGAAAACCAGTTGCTGCTCGACGACTCCTACAACGCCAATGTCGGTTCAATGACTGCAGCAGTCCAGGTACTGGCT"
    "GAAATGCCGGGCTACCGCGTGCTGGTGGTGGGCGATATGGCGGAACTGGGCGCTGAAAGCGAAGCCTGCCATGTACAGGTGGGCGAGGCGGCAAAAGCTG"
    "CTGGTATTGACCGCGTGTTAAGCGTGGGTAAACAAAGCCATGCTATCAGCACCGCCAGCGGCGTTGGCGAACATTTTGCTGATAAAACTGCGTTAATTAC"
    "GCGTCTTAAATTACTGATTGCTGAGCAACAGGTAATTACGATTTTAGTTAAGGGTTCACGTAGTGCCGCCATGGAAGAGGTAGTACGCGCTTTACAGGAG"
    "AATGGGACATGTTAGTTTGGCTGGCCGAACATTTGGTCAAATATTATTCCGGCTTTAACGTCTTTTCCTATCTGACGTTTCGCGCCATCGTCAGCCTGCT"
    "GACCGCGCTGTTCATCTCATTGTGGATGGGCCCGCGTATGATTGCTCATTTGCAAAAACTTTCCTTTGGTCAGGTGGTGCGTAACGACGGTCCTGAATCA"
    "CACTTCAGCAAGCGCGGTACGCCGACCATGGGCGGGATTATGATCCTGACGGCGATTGTGATCTCCGTACTGCTGTGGGCTTACCCGTCCAATCCGTACG"
    "TCTGGTGCGTGTTGGTGGTGCTGGTAGGTTACGGTGTTATTGGCTTTGTTGATGATTATCGCAAAGTGGTGCGTAAAGACACCAAAGGGTTGATCGCTCG"
)
TARGET = (
    "CAACAACGACATCGGTGTACCGATGACGCTGTTGCGCTTAACGCCGGAATACGATTACGCAGTTATTGAACTTGGCGCGAACCATCAGGGCGAAATAGCC"
    "TGGACTGTGAGTCTGACTCGCCCGGAAGCTGCGCTGGTCAACAACCTGGCAGCGGCGCATCTGGAAGGTTTTGGCTCGCTTGCGGGTGTCGCGAAAGCGA"
    "AAGGTGAAATCTTTAGCGGCCTGCCGGAAAACGGTATCGCCATTATGAACGCCGACAACAACGACTGGCTGAACTGGCAGAGCGTAATTGGCTCACGCAA"
    "AGTGTGGCGTTTCTCACCCAATGCCGCCAACAGCGATTTCACCGCCACCAATATCCATGTGACCTCGCACGGTACGGAATTTACCCTACAAACCCCAACC"
    "GGTAGCGTCGATGTTCTGCTGCCGTTGCCGGGGCGTCACAATATTGCGAATGCGCTGGCAGCCGCTGCGCTCTCCATGTCCGTGGGCGCAACGCTTGATG"
    "CTATCAAAGCGGGGCTGGCAAATCTGAAAGCTGTTCCAGGCCGTCTGTTCCCCATCCAACTGGCAGAAAACCAGTTGCTGCTCGACGACTCCTACAACGC"
    "CAATGTCGGTTCAATGACTGCAGCAGTCCAGGTACTGGCTGAAATGCCGGGCTACCGCGTGCTGGTGGTGGGCGATATGGCGGAACTGGGCGCTGAAAGC"
    "GAAGCCTGCCATGTACAGGTGGGCGAGGCGGCAAAAGCTGCTGGTATTGACCGCGTGTTAAGCGTGGGTAAACAAAGCCATGCTATCAGCACCGCCAGCG"
    "GCGTTGGCGAACATTTTGCTGATAAAACTGCGTTAATTACGCGTCTTAAATTACTGATTGCTGAGCAACAGGTAATTACGATTTTAGTTAAGGGTTCACG"
    "TAGTGCCGCCATGGAAGAGGTAGTACGCGCTTTACAGGAGAATGGGACATGTTAGTTTGGCTGGCCGAACATTTGGTCAAATATTATTCCGGCTTTAACG"
)

EXTENSION_CASE = {
    "source": "cudamapper/tests/Test_CudamapperOverlapper.cpp:24-78",
    "query": QUERY,
    "target": TARGET,
    # :65-70, in the order of the models' tuples; the ids, residues and
    # overlap_complete are not set by the reference's test
    "overlap": {"query_start": 1, "query_end": 636, "target_start": 341, "target_end": 976, "strand": "+"},
    "extension": 50,  # :72
    "required_similarity": 0.8,
    # :74-77
    "expected": {"query_start": 0, "query_end": 660, "target_start": 340, "target_end": 1000},
}

# cudamapper/tests/Test_CudamapperUtilsKmerFunctions.cpp:73-95
# (sequence_jaccard_similarity(a, b, 4, 1)); the third is only bounded there
SIMILARITY_CASES = [
    {"name": "identical", "source": "Test_CudamapperUtilsKmerFunctions.cpp:73-80", "a": "AAACCTATGAGGG",
     "b": "AAACCTATGAGGG", "kmer_size": 4, "equals": 1.0},
    {"name": "disjoint", "source": "Test_CudamapperUtilsKmerFunctions.cpp:81-87", "a": "AAACCTATGAGGG",
     "b": "CCCAATTTAAATT", "kmer_size": 4, "equals": 0.0},
    {"name": "similar", "source": "Test_CudamapperUtilsKmerFunctions.cpp:88-95", "a": "AAACCTATGAGGG",
     "b": "AAACCTAAGAGGG", "kmer_size": 4, "greater_than": 0.0, "less_than": 1.0},
]

# cudamapper/tests/Test_CudamapperUtilsKmerFunctions.cpp:25-42: 8 substrings of AAACCTTCTCT at k = 4,
# the first AAAC and the last CTCT; the empty string gives one empty substring
KMER_CASES = [
    {"source": "Test_CudamapperUtilsKmerFunctions.cpp:25-34", "s": "AAACCTTCTCT", "kmer_size": 4, "count": 8,
     "first": "AAAC", "last": "CTCT"},
    {"source": "Test_CudamapperUtilsKmerFunctions.cpp:36-42", "s": "", "kmer_size": 4, "count": 1, "first": "",
     "last": ""},
]

# complement_array, cudamapper/src/overlapper.cpp:94-99, as the letters its 26 numbers stand for
COMPLEMENT = "TBGDEFCHIJKLMNOPQRSAUVWXYZ"


def main():
    assert len(QUERY) == len(TARGET) == 1000 and QUERY[:660] == TARGET[340:]
    kat = {"source": "GenomeWorks 0.5.0 reference tests and sources (see make_rescue_golden.py for file:line)",
           "extension_case": EXTENSION_CASE, "similarity_cases": SIMILARITY_CASES, "kmer_cases": KMER_CASES,
           "complement": COMPLEMENT}
    with open(os.path.join(HERE, "rescue_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
