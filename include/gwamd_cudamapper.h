/*
 * gwamd_cudamapper.h -- C ABI of cudamapper's minimizer index, anchor matcher,
 * overlapper, overlap-end rescue and overlap-alignment caller (libgwamd.so).
 *
 * The reference aligns cudamapper overlaps inside its cudamapper executable
 * (cudamapper/src/main.cu:48-175: run_alignment_batch / align_overlaps) and
 * prints them with print_paf (cudamapper/src/cudamapper_utils.cpp:30-112).
 * A reference-side binding would call these in place of those two functions:
 *
 *   gwamd_align_overlaps   align_overlaps(allocator, overlaps, query_parser,
 *                          target_parser, num_alignment_engines, cigars)   main.cu:125-175
 *   gwamd_read_fasta       io::create_kseq_fasta_parser(path, min_len, shuffle) fasta_parser.hpp:62-64
 *   gwamd_format_paf       print_paf(overlaps, cigars, query_parser,
 *                          target_parser, kmer_size, mutex)                cudamapper_utils.cpp:30-112
 *   gwamd_index_create     Index::create_index(allocator, parser, first, past,
 *                          kmer_size, window_size, hash, filtering)        index.hpp:97-106
 *   gwamd_match_anchors    Matcher::create_matcher(allocator, query_index,
 *                          target_index)->anchors()                        matcher.hpp:45-48
 *   gwamd_get_overlaps     OverlapperTriggered(allocator).get_overlaps(overlaps,
 *                          d_anchors, min_residues, min_overlap_len,
 *                          min_bases_per_residue, min_overlap_fraction)    overlapper_triggered.hpp:49-57
 *   gwamd_match_overlaps   create_matcher + get_overlaps on its anchors    main.cu:227-240
 *   gwamd_post_process_overlaps
 *                          Overlapper::post_process_overlaps(overlaps,
 *                          drop_fused_overlaps)                            overlapper.hpp:93
 *   gwamd_rescue_overlap_ends
 *                          Overlapper::rescue_overlap_ends(overlaps, query_parser,
 *                          target_parser, extension, required_similarity)  overlapper.hpp:95-106
 *   gwamd_extend_overlap_by_sequence_similarity
 *                          details::overlapper::extend_overlap_by_sequence_similarity(
 *                          overlap, query, target, extension, required_similarity) overlapper.hpp:35-47
 *   gwamd_group_reads_into_indices
 *                          group_reads_into_indices(parser, max_basepairs_per_index) index_descriptor.hpp:80-87
 *   gwamd_generate_batches_of_indices
 *                          generate_batches_of_indices(...)                    index_batcher.cuh:102-110
 *   gwamd_device_reads_create
 *                          no counterpart: the reads of one parser put on the device
 *                          once (DeviceReads::create, device_reads.hpp)
 *   gwamd_rescue_overlap_ends_resident
 *                          Overlapper::rescue_overlap_ends on two DeviceReads  overlapper.hpp:95-106
 *   gwamd_align_overlaps_resident
 *                          align_overlaps on two DeviceReads                   main.cu:125-175
 *
 * Reads are passed as one byte array per side with n+1 offsets (read i is
 * bases[offsets[i], offsets[i+1])); names as NUL-separated strings with n+1
 * offsets.  gwamd_overlap has the layout of cudamapper::Overlap
 * (cudamapper/include/.../types.hpp:68-89).  Results are returned in a
 * gwamd_text_list owned by the library (free with gwamd_text_list_free).
 *
 * Error convention: 0 on success, or a negative GWAMD_E_* code where the
 * reference throws (message in gwamd_last_error()).
 */
#ifndef GWAMD_CUDAMAPPER_H
#define GWAMD_CUDAMAPPER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GWAMD_E_INVALID_ARGUMENT
#define GWAMD_E_INVALID_ARGUMENT (-1)
#define GWAMD_E_RUNTIME (-2)
#define GWAMD_E_HIP (-3)
#endif

/* cudamapper::Overlap; relative_strand is '+' (Forward) or '-' (Reverse). */
typedef struct gwamd_overlap
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_start;
    uint32_t target_start;
    uint32_t query_end;
    uint32_t target_end;
    unsigned char relative_strand;
    uint32_t num_residues;
    uint8_t overlap_complete;
} gwamd_overlap;

typedef struct gwamd_text_list gwamd_text_list;

const char* gwamd_last_error(void);

/* One CIGAR per overlap, in overlap order.  num_alignment_engines host threads
 * (>= 1) share the overlaps; device_id selects the GPU. */
int32_t gwamd_align_overlaps(const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                             const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                             const gwamd_overlap* overlaps, int32_t num_overlaps, int32_t num_alignment_engines,
                             int32_t device_id, gwamd_text_list** cigars);

/* The PAF text of print_paf as one entry; cigars may be NULL (no cg:Z: tag). */
int32_t gwamd_format_paf(const char* query_names, const int64_t* query_name_offsets, const int64_t* query_lengths,
                         int32_t num_queries, const char* target_names, const int64_t* target_name_offsets,
                         const int64_t* target_lengths, int32_t num_targets, const gwamd_overlap* overlaps,
                         int32_t num_overlaps, const gwamd_text_list* cigars, int32_t kmer_size,
                         gwamd_text_list** paf);

/* Reads of a FASTA/FASTQ file as io::create_kseq_fasta_parser(path, min_sequence_length,
 * shuffle) holds them (fasta_parser.hpp:62-64; kseqpp_fasta_parser.cpp:31-72): names and
 * sequences in parser order (shuffled with std::mt19937(0) when shuffle != 0). */
int32_t gwamd_read_fasta(const char* path, uint32_t min_sequence_length, int32_t shuffle, gwamd_text_list** names,
                         gwamd_text_list** sequences);
/* The same, and the records' quality strings: one per record, of its sequence's length for a
 * FASTQ record and empty for a FASTA record. */
int32_t gwamd_read_fasta_with_qualities(const char* path, uint32_t min_sequence_length, int32_t shuffle,
                                        gwamd_text_list** names, gwamd_text_list** sequences,
                                        gwamd_text_list** qualities);
/* A list holding copies of n texts (e.g. CIGARs from another aligner run for gwamd_format_paf). */
int32_t gwamd_text_list_create(const char* const* texts, const int64_t* lengths, int32_t n, gwamd_text_list** out);
/* Entry i of a list (text and length, not NUL terminated beyond length). */
int32_t gwamd_text_list_size(const gwamd_text_list* list);
int32_t gwamd_text_list_get(const gwamd_text_list* list, int32_t i, const char** text, int64_t* length);
void gwamd_text_list_free(gwamd_text_list* list);

/* ---- (k,w)-minimizer index and anchor matcher -------------------------------
 *
 * The index of the reads [first_read_id, past_the_last_read_id) of the given
 * reads holds one sketch element per distinct window minimizer, ordered by
 * (representation, read_id, position_in_read).  A read shorter than
 * window_size + kmer_size - 1 contributes nothing but keeps its id (the
 * reference shifts the ids of the reads after it, index_gpu.cuh:720-734).
 * Limits, each GWAMD_E_INVALID_ARGUMENT before any device call:
 * 1 <= kmer_size <= 32, 1 <= window_size <= 255, 0 <= filtering_parameter <= 1,
 * 0 <= first_read_id <= past_the_last_read_id <= num_reads, reads shorter than
 * 2^31 bases.  An index holds fewer than 2^32 sketch elements and a match at
 * most max_anchors anchors (GWAMD_E_RUNTIME beyond). */
typedef struct gwamd_index gwamd_index;
struct gwamd_device_allocator; /* the pool handle of gwamd_cudaaligner.h (gwamd_device_allocator_create) */

/* cudamapper::Anchor (types.hpp:52-62) */
typedef struct gwamd_anchor
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_position_in_read;
    uint32_t target_position_in_read;
} gwamd_anchor;

typedef struct gwamd_index_info_t
{
    int64_t num_elements;
    int64_t num_unique_representations;
    uint32_t number_of_reads; /* past - first, or 0 when no read is long enough */
    uint32_t smallest_read_id;
    uint32_t largest_read_id;
    uint32_t number_of_basepairs_in_longest_read;
} gwamd_index_info_t;

int32_t gwamd_index_create(const char* bases, const int64_t* offsets, int32_t num_reads, int32_t first_read_id,
                           int32_t past_the_last_read_id, int32_t kmer_size, int32_t window_size,
                           int32_t hash_representations, double filtering_parameter, int32_t device_id,
                           gwamd_index** out);
/* ... with every device byte (the index's arrays for its lifetime, scratch
 * while it is built) counted against the allocator's pool */
int32_t gwamd_index_create_with_allocator(const char* bases, const int64_t* offsets, int32_t num_reads,
                                          int32_t first_read_id, int32_t past_the_last_read_id, int32_t kmer_size,
                                          int32_t window_size, int32_t hash_representations,
                                          double filtering_parameter, int32_t device_id,
                                          struct gwamd_device_allocator* allocator, gwamd_index** out);
void gwamd_index_free(gwamd_index* index);
int32_t gwamd_index_info(const gwamd_index* index, gwamd_index_info_t* info);
/* Copies the arrays to host buffers sized by gwamd_index_info (num_elements
 * for the first four, num_unique_representations for the fifth and, unless
 * the index is empty, one more than that for the last).  A NULL pointer skips
 * its array. */
int32_t gwamd_index_copy(const gwamd_index* index, uint64_t* representations, uint32_t* read_ids,
                         uint32_t* positions_in_reads, uint8_t* directions_of_reads,
                         uint64_t* unique_representations, uint32_t* first_occurrence_of_representations);

/* All pairs of a query and a target sketch element of equal representation,
 * sorted by (query_read_id, target_read_id, query_position_in_read,
 * target_position_in_read), in a host array owned by the library (free with
 * gwamd_anchors_free; NULL when there are none).  The two indices may be the
 * same; self-matches are kept.  max_anchors: -1 for the default of 2^31. */
int32_t gwamd_match_anchors(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
                            gwamd_anchor** anchors, int64_t* num_anchors);
int32_t gwamd_match_anchors_with_allocator(const gwamd_index* query_index, const gwamd_index* target_index,
                                           int64_t max_anchors, struct gwamd_device_allocator* allocator,
                                           gwamd_anchor** anchors, int64_t* num_anchors);
void gwamd_anchors_free(gwamd_anchor* anchors);

/* ---- overlapper: sorted anchors to overlaps -----------------------------------
 *
 * OverlapperTriggered::get_overlaps (overlapper_triggered.cu:232-427) on the
 * GPU.  Neighbouring anchors of the same two reads whose query positions are
 * less than 150 apart and whose target positions differ by less than 150 form
 * a chain; chains of three anchors or more are kept; a kept chain joins the
 * kept chain before it when their first anchors are on the same reads and
 * |query distance - target distance| < 300; every such group becomes one
 * overlap from its first anchor to its last, Reverse ('-') with the target
 * positions swapped when they fall.  An overlap is returned when
 *   num_residues >= min_residues,
 *   max(query span, target span) / num_residues < min_bases_per_residue,
 *   query span >= min_overlap_len and target span >= min_overlap_len,
 *   query_read_id != target_read_id, and
 *   target span / longer span > min_overlap_fraction, the same for the query
 *   span (float32 quotients),
 * in anchor order, in a host array owned by the library (free with
 * gwamd_overlaps_free; NULL when there are none).  The reference's defaults
 * are 20, 50, 50 and 0.9f (overlapper_triggered.hpp:49-54).
 * GWAMD_E_INVALID_ARGUMENT, before any device call: a negative n or min_*, a
 * NaN fraction, n > 2^31; and after the first kernel, with nothing returned:
 * anchors that are not sorted as gwamd_match_anchors sorts them, or a
 * position of 2^31 or more.  n == 0 gives no overlaps without a device call. */

/* OverlapperTriggered(allocator).get_overlaps(overlaps, d_anchors, min_residues, min_overlap_len,
 * min_bases_per_residue, min_overlap_fraction) (overlapper_triggered.hpp:49-57) on n host anchors */
int32_t gwamd_get_overlaps(const gwamd_anchor* anchors, int64_t n, int64_t min_residues, int64_t min_overlap_len,
                           int64_t min_bases_per_residue, float min_overlap_fraction, int32_t device_id,
                           gwamd_overlap** overlaps, int64_t* num_overlaps);
int32_t gwamd_get_overlaps_with_allocator(const gwamd_anchor* anchors, int64_t n, int64_t min_residues,
                                          int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, int32_t device_id,
                                          struct gwamd_device_allocator* allocator, gwamd_overlap** overlaps,
                                          int64_t* num_overlaps);
/* Matcher::create_matcher followed by get_overlaps on matcher->anchors() (main.cu:227-240): the
 * anchors stay on the device; num_anchors (may be NULL) receives their number. */
int32_t gwamd_match_overlaps(const gwamd_index* query_index, const gwamd_index* target_index, int64_t max_anchors,
                             int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                             float min_overlap_fraction, gwamd_overlap** overlaps, int64_t* num_overlaps,
                             int64_t* num_anchors);
int32_t gwamd_match_overlaps_with_allocator(const gwamd_index* query_index, const gwamd_index* target_index,
                                            int64_t max_anchors, int64_t min_residues, int64_t min_overlap_len,
                                            int64_t min_bases_per_residue, float min_overlap_fraction,
                                            struct gwamd_device_allocator* allocator, gwamd_overlap** overlaps,
                                            int64_t* num_overlaps, int64_t* num_anchors);
/* Overlapper::post_process_overlaps(overlaps, drop_fused_overlaps) (overlapper.cpp:127-228), host
 * only: the n overlaps (without those fused, if drop_fused_overlaps != 0) followed by the fusions. */
int32_t gwamd_post_process_overlaps(const gwamd_overlap* in, int64_t n, int32_t drop_fused_overlaps,
                                    gwamd_overlap** out, int64_t* num_out);
void gwamd_overlaps_free(gwamd_overlap* overlaps);

/* ---- overlap-end rescue ---------------------------------------------------------
 *
 * Overlapper::rescue_overlap_ends (overlapper.cpp:295-365) on the GPU, one
 * wave per overlap: three rounds of extend_overlap_by_sequence_similarity.
 * A round looks at the h = min(query_start, target_start, extension) bases
 * before the overlap on both reads and at the t = min(extension, bases left on
 * the query, bases left on the target) bases after it, and moves an end out by
 * its whole window when the two windows' similarity is at least
 * required_similarity (float32 quotient, float32 threshold).  The similarity
 * is sequence_jaccard_similarity(a, b, 15, 1) as the reference computes it
 * (cudamapper_utils.cpp:114-170): shared / (|A| + |B| - shared) over the
 * multisets of substrings s[i, min(L, 2i + 15)), i = 0 .. L - 15 (substr is
 * given i + 15 as its count), or over the whole windows when L < 15, so two
 * empty windows are similar.  A Reverse overlap is rescued against the
 * reverse complement of its target as the reference makes it
 * (overlapper.cpp:94-109): A<->T and C<->G, every other letter kept, the
 * middle base of a target of odd length not complemented; a byte outside
 * 'A'..'Z', undefined behaviour there, is kept too.  Read ids, strand,
 * num_residues and overlap_complete come back unchanged.
 *
 * Unlike the reference's C++ entry point, which runs every round with 100 and
 * 0.9f whatever it is given, these honour extension and required_similarity.
 * GWAMD_E_INVALID_ARGUMENT, before any device call: a NULL array with a
 * positive count, a negative count, offsets that fall, a read of 2^31 bases or
 * more, a read id at or beyond its side's count, start > end or end > read
 * length on either side, a strand other than '+' and '-', extension outside
 * 0..128, a NaN required_similarity.  n == 0 gives nothing without a device
 * call.  Query and target arguments that are the same pointers are uploaded
 * once. */

/* The n overlaps with their ends rescued, in a host array owned by the library (gwamd_overlaps_free). */
int32_t gwamd_rescue_overlap_ends(const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                                  const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                                  const gwamd_overlap* overlaps, int64_t n, int32_t extension,
                                  float required_similarity, int32_t device_id, gwamd_overlap** out,
                                  int64_t* num_out);
int32_t gwamd_rescue_overlap_ends_with_allocator(const char* query_bases, const int64_t* query_offsets,
                                                 int32_t num_queries, const char* target_bases,
                                                 const int64_t* target_offsets, int32_t num_targets,
                                                 const gwamd_overlap* overlaps, int64_t n, int32_t extension,
                                                 float required_similarity, int32_t device_id,
                                                 struct gwamd_device_allocator* allocator, gwamd_overlap** out,
                                                 int64_t* num_out);
/* One round on one overlap in place, on the host, with no limit on extension (a negative one is
 * converted to unsigned, as in the reference).  The strand is not looked at: for a Reverse overlap
 * the caller passes the reverse complement and the mirrored target positions. */
int32_t gwamd_extend_overlap_by_sequence_similarity(gwamd_overlap* overlap, const char* query, int64_t query_len,
                                                    const char* target, int64_t target_len, int32_t extension,
                                                    float required_similarity);

/* ---- index descriptors and batches of indices (host only) -------------------------
 *
 * An index descriptor is the range of reads one index is built from.  The
 * reads are given by their lengths (0 <= length < 2^31); basepairs per index
 * is below 2^32.  GWAMD_E_INVALID_ARGUMENT for those, for a negative count or
 * a NULL array with a positive one, for a NULL output, for a number of indices
 * per batch below 1, and for the four cases of generate_batches_of_indices with
 * same_query_and_target != 0: the two sides differ in indices per host batch,
 * in indices per device batch, in the parser (here: query_lengths and
 * target_lengths are not the same pointer and count) or in basepairs per
 * index. */
typedef struct gwamd_index_descriptor
{
    uint32_t first_read;
    uint32_t number_of_reads;
} gwamd_index_descriptor;

/* group_reads_into_indices(parser, max_basepairs_per_index) (index_descriptor.cpp:76-109), in a
 * library-owned array (gwamd_index_descriptors_free).  As there, the first descriptor is {0, 0}
 * when read 0 alone is over the limit, and no reads give the one descriptor {0, 0}. */
int32_t gwamd_group_reads_into_indices(const int64_t* lengths, int32_t n, int64_t max_basepairs,
                                       gwamd_index_descriptor** descriptors, int64_t* count);
void gwamd_index_descriptors_free(gwamd_index_descriptor* descriptors);
/* IndexDescriptor::get_hash (index_descriptor.cpp:43-59): first_read | number_of_reads << 32 */
uint64_t gwamd_index_descriptor_hash(uint32_t first_read, uint32_t number_of_reads);

/* generate_batches_of_indices (index_batcher.cu:24-88), flattened into `count` 64-bit values in a
 * library-owned array (gwamd_batches_of_indices_free).  With a list of descriptors written as its
 * length followed by (first_read, number_of_reads) per descriptor, the array holds the number of
 * host batches and then per host batch: its query descriptors, its target descriptors, the number
 * of its device batches and, per device batch, its query and its target descriptors. */
int32_t gwamd_generate_batches_of_indices(int32_t query_indices_per_host_batch, int32_t query_indices_per_device_batch,
                                          int32_t target_indices_per_host_batch,
                                          int32_t target_indices_per_device_batch, const int64_t* query_lengths,
                                          int32_t num_queries, const int64_t* target_lengths, int32_t num_targets,
                                          int64_t query_basepairs_per_index, int64_t target_basepairs_per_index,
                                          int32_t same_query_and_target, int64_t** batches, int64_t* count);
void gwamd_batches_of_indices_free(int64_t* batches);

/* ---- host copy of an index ---------------------------------------------------------
 *
 * IndexHostCopyBase (reference index.hpp:109-182): the six arrays and the scalars of an
 * index in host memory, from which the index goes back to a device without being built
 * again.  The index that comes back equals the original in every array and getter and is
 * accepted wherever a gwamd_index is.  GWAMD_E_INVALID_ARGUMENT for a NULL handle or
 * output, a kmer_size outside 1..32, a window_size outside 1..255, a negative device_id. */
typedef struct gwamd_index_host_copy gwamd_index_host_copy;

/* IndexHostCopyBase::create_cache(index, first_read_id, kmer_size, window_size, stream) */
int32_t gwamd_index_host_copy_create(const gwamd_index* index, uint32_t first_read_id, int32_t kmer_size,
                                     int32_t window_size, gwamd_index_host_copy** out);
/* copy_index_to_device(allocator, stream) on device_id; the bytes count against the pool (NULL: none) */
int32_t gwamd_index_host_copy_to_device(const gwamd_index_host_copy* copy, int32_t device_id,
                                        struct gwamd_device_allocator* allocator_or_null, gwamd_index** out);
/* the sizes and getters of the copy (a NULL output other than info is skipped) */
int32_t gwamd_index_host_copy_info(const gwamd_index_host_copy* copy, gwamd_index_info_t* info,
                                   uint32_t* first_read_id, int32_t* kmer_size, int32_t* window_size);
void gwamd_index_host_copy_free(gwamd_index_host_copy* copy);

/* ---- reads resident on the device -----------------------------------------------
 *
 * The reference reads the parsers on the host in every call of
 * rescue_overlap_ends and align_overlaps.  A gwamd_device_reads holds the
 * packed bases and the n + 1 offsets of one read set on one device, uploaded
 * once; the _resident entries below then move only the overlaps.  The bytes
 * are counted against the allocator's pool (NULL: none) until the handle is
 * freed.  The argument checks of gwamd_device_reads_create are those of the
 * reads of gwamd_rescue_overlap_ends, and a negative device_id; the checks of
 * the _resident entries are those of their host-read twins, with the lengths
 * taken from the handle's host copy of the offsets, and in addition a NULL
 * handle and a handle on another device than the current one, each
 * GWAMD_E_INVALID_ARGUMENT.  The same handle may be given for both sides. */
typedef struct gwamd_device_reads gwamd_device_reads;

/* DeviceReads::create(allocator, parser, stream) (device_reads.hpp) on device_id */
int32_t gwamd_device_reads_create(const char* bases, const int64_t* offsets, int32_t num_reads, int32_t device_id,
                                  struct gwamd_device_allocator* allocator_or_null, gwamd_device_reads** out);
/* The same with the reads' quality characters in a second device array of the same layout:
 * qualities[offsets[i], offsets[i + 1]) belongs to read i, one character per base (Phred + 33).
 * GWAMD_E_INVALID_ARGUMENT, before any device call, also for a character outside 33..126 and
 * NULL qualities with a base to describe.  gwamd_poa_add_poa_group_resident (gwamd_polish.h)
 * turns them into base weights; every other entry treats the handle as one without. */
int32_t gwamd_device_reads_create_with_qualities(const char* bases, const char* qualities, const int64_t* offsets,
                                                 int32_t num_reads, int32_t device_id,
                                                 struct gwamd_device_allocator* allocator_or_null,
                                                 gwamd_device_reads** out);
/* 1 when the handle carries qualities, 0 when not */
int32_t gwamd_device_reads_has_qualities(const gwamd_device_reads* reads);
void gwamd_device_reads_free(gwamd_device_reads* reads);
/* number of reads, of bases, and the device; a NULL output is skipped */
int32_t gwamd_device_reads_info(const gwamd_device_reads* reads, int64_t* num_reads, int64_t* num_bases,
                                int32_t* device_id);

/* Overlapper::rescue_overlap_ends(overlaps, query_reads, target_reads, extension,
 * required_similarity) (overlapper.hpp, the DeviceReads overload; reference overlapper.hpp:95-106) */
int32_t gwamd_rescue_overlap_ends_resident(const gwamd_device_reads* query_reads,
                                           const gwamd_device_reads* target_reads, const gwamd_overlap* overlaps,
                                           int64_t n, int32_t extension, float required_similarity,
                                           struct gwamd_device_allocator* allocator_or_null, gwamd_overlap** out,
                                           int64_t* num_out);

/* align_overlaps(allocator, overlaps, query_reads, target_reads, num_alignment_engines, cigars)
 * (overlap_alignment.hpp, the DeviceReads overload; reference main.cu:125-175): the CIGARs of
 * gwamd_align_overlaps, with the overlap regions gathered into the aligner on the device. */
int32_t gwamd_align_overlaps_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                      const gwamd_overlap* overlaps, int32_t n, int32_t num_alignment_engines,
                                      gwamd_text_list** cigars);

/* Test hook, not used by the library itself: gather_overlap_regions_kernel on n overlaps
 * into a device buffer of 2 n stride bytes, copied to seqs_out (2 n stride bytes) and
 * lens_out (2 n entries).  Overlap i's query region lies at seqs_out + 2 i stride, its target
 * region, reverse-complemented for '-', at seqs_out + (2 i + 1) stride.  The hook clears the
 * device buffer before the launch and the kernel writes nothing outside a region, so the
 * bytes of a slot past its region's length are zero.  Every argument is checked before any device call: NULL handles or
 * outputs, a negative n, 2 n stride of 2^31 or more, overlaps outside their reads, a
 * stride below 1 or shorter than a region.  n == 0 returns without a launch. */
int32_t gwamd_internal_gather_overlap_regions(const gwamd_device_reads* query_reads,
                                              const gwamd_device_reads* target_reads, const gwamd_overlap* overlaps,
                                              int64_t n, int64_t stride, char* seqs_out, int32_t* lens_out);

#ifdef __cplusplus
}
#endif

#endif /* GWAMD_CUDAMAPPER_H */
