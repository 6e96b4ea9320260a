/* C ABI of cudapolish: aligned overlaps cut into target windows on the GPU and
 * grouped into cudapoa groups (a racon-style polisher's middle step; racon's
 * find_breaking_points).
 *
 * Path states are cudaaligner AlignmentState values, start -> end:
 *   0 match, 1 mismatch   advance the query and the target,
 *   3 deletion            advances ONLY THE QUERY,
 *   2 insertion           advances ONLY THE TARGET.
 * This is the reference's convention (alignment_impl.cpp:94-103) and the
 * opposite of SAM's I / D.
 *
 * Overlap i aligns query[query_start, query_end) against target[target_start,
 * target_end), forward coordinates with start <= end; for relative_strand '-'
 * the target region is aligned as its reverse complement, as
 * gwamd_align_overlaps does.  With u the target offset and v the query offset
 * before a state, its target position is t = reverse ? target_end - 1 - u :
 * target_start + u and its query position q = query_start + v.  The segment of
 * the overlap in target window k (window_length w) is taken over the match and
 * mismatch states with t / w == k: q_begin = min q, q_end = max q + 1,
 * t_begin = min t, t_end = max t + 1.
 *
 * Overlap i owns the consecutive records of windows target_start / w ..
 * (target_end - 1) / w, ascending (none when target_start == target_end);
 * overlaps come in input order.  A window the overlap spans without a match or
 * mismatch state in it is empty: positions 0 and GWAMD_SEGMENT_EMPTY.  A path
 * with a state outside 0..3, or that does not advance the query by exactly
 * query_end - query_start and the target by exactly target_end - target_start,
 * does not fit: every record of its overlap is empty with
 * GWAMD_SEGMENT_BAD_PATH, the records of the other overlaps are unaffected.
 *
 * Errors as in gwamd_cudamapper.h; every argument is checked before any device call. */
#ifndef GWAMD_POLISH_H
#define GWAMD_POLISH_H

#include "gwamd_cudapoa.h"

#include "gwamd_cudamapper.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GWAMD_SEGMENT_REVERSE 1u     /* the overlap's relative_strand is '-' */
#define GWAMD_SEGMENT_EMPTY 2u       /* no match or mismatch state in the window */
#define GWAMD_SEGMENT_BAD_PATH 4u    /* the path does not fit the overlap */
#define GWAMD_SEGMENT_NOT_ALIGNED 8u /* the overlap is beyond the aligner's limits */

typedef struct gwamd_window_segment
{
    uint32_t overlap; /* index into the overlaps of the call */
    uint32_t window;  /* k */
    uint32_t q_begin;
    uint32_t q_end;
    uint32_t t_begin;
    uint32_t t_end;
    uint32_t flags;
    uint32_t reserved; /* 0 */
} gwamd_window_segment;

/* The records of n overlaps whose paths are states[state_offsets[i], state_offsets[i + 1])
 * (start -> end), cut by one kernel launch on device_id, in a host array owned by the library
 * (gwamd_window_segments_free; NULL when there are none).  Device arrays are counted against
 * allocator_or_null's pool for the duration of the call.  GWAMD_E_INVALID_ARGUMENT: a NULL
 * pointer with something behind it, n < 0 or >= 2^31, window_length <= 0, offsets that fall, an
 * overlap with start > end or a strand other than '+' / '-', a path longer than
 * (query_end - query_start) + (target_end - target_start), more than 2^31 records.  n == 0
 * returns without a device call. */
int32_t gwamd_window_segments(const gwamd_overlap* overlaps, int64_t n, const int8_t* states,
                              const int64_t* state_offsets, int32_t window_length, int32_t device_id,
                              struct gwamd_device_allocator* allocator_or_null, gwamd_window_segment** out,
                              int64_t* num_out);

/* The same walk for one overlap on the host; the records carry overlap_index. */
int32_t gwamd_window_segments_host(const gwamd_overlap* overlap, const int8_t* states, int64_t num_states,
                                   int32_t window_length, uint32_t overlap_index, gwamd_window_segment** out,
                                   int64_t* num_out);

/* The overlaps aligned as gwamd_align_overlaps_resident aligns them and cut where the aligner
 * leaves its paths on the device: only overlaps go up and records come back.  An overlap beyond
 * the aligner's limits gets GWAMD_SEGMENT_NOT_ALIGNED (and the warning of gwamd_align_overlaps).
 * The reads are on the current device. */
int32_t gwamd_window_segments_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                       const gwamd_overlap* overlaps, int32_t n, int32_t window_length,
                                       int32_t num_alignment_engines, gwamd_window_segment** out, int64_t* num_out);

void gwamd_window_segments_free(gwamd_window_segment* segments);

/* ---- the cut from CIGAR runs ------------------------------------------------------
 *
 * A CIGAR is an array of 32-bit words length << 4 | op, op in BAM numbering: M 0, I 1, D 2,
 * = 7, X 8; the length is below 2^28, and a length of 0 contributes nothing.  The records of
 * an overlap and its CIGAR are those of the state path the CIGAR stands for: the CIGAR is
 * normalised to GWAMD_CIGAR_GENOMEWORKS, every run of length n written as n states (M, = and
 * X: 0 or 1, which the records do not tell apart; I: 2; D: 3) and the definition at the top of
 * this file applied.  No entry point expands a run: the work is per run and per window
 * boundary.  Any other op code (N, S, H, P, 9..15), of any length, makes the overlap a misfit
 * (GWAMD_SEGMENT_BAD_PATH), as do advances that are not exactly the overlap's two spans,
 * whatever they sum to (the sums do not wrap); the call does not fail.
 *
 * GWAMD_CIGAR_GENOMEWORKS: what gwamd_align_overlaps and cudamapper -a emit.  I advances only
 * the target, D only the query; for a '-' overlap the ops run along the query forward and the
 * reverse complement of the target region.
 * GWAMD_CIGAR_SAM: minimap2's PAF and SAM.  I advances only the query, D only the target; for
 * a '-' overlap the ops run along the target forward and the reverse complement of the query
 * region (t = target_start + u, q = query_end - 1 - v).  Normalised by exchanging I and D
 * and, for '-', reversing the order of the ops: the same records. */
#define GWAMD_CIGAR_GENOMEWORKS 0
#define GWAMD_CIGAR_SAM 1

/* gwamd_window_segments for n overlaps whose CIGARs are ops[op_offsets[i], op_offsets[i + 1]):
 * one kernel launch over the runs.  Errors, ownership and the checks of the overlaps,
 * window_length, device_id and the outputs as there; besides, GWAMD_E_INVALID_ARGUMENT for a
 * convention other than the two above, op_offsets that are negative or fall, and NULL ops with
 * an op behind it.  Every argument is checked before any device call; n == 0 makes none. */
int32_t gwamd_window_segments_cigar(const gwamd_overlap* overlaps, int64_t n, const uint32_t* ops,
                                    const int64_t* op_offsets, int32_t convention, int32_t window_length,
                                    int32_t device_id, struct gwamd_device_allocator* allocator_or_null,
                                    gwamd_window_segment** out, int64_t* num_out);

/* The same walk over runs for one overlap on the host; the records carry overlap_index. */
int32_t gwamd_window_segments_cigar_host(const gwamd_overlap* overlap, const uint32_t* ops, int64_t num_ops,
                                         int32_t convention, int32_t window_length, uint32_t overlap_index,
                                         gwamd_window_segment** out, int64_t* num_out);

/* CIGAR text such as 12M3I4D5=1X as ops: *num_ops receives their number, and with
 * out_or_null they are written to out_or_null[0, *num_ops).  Every letter of MIDNSHP=X is
 * taken (BAM numbering); empty text gives 0 ops.  GWAMD_E_INVALID_ARGUMENT: a letter without
 * a number, an unknown letter, a length of 2^28 or more, digits at the end, NULL text with
 * text_length > 0, NULL num_ops, and a capacity below the number of ops (which *num_ops then
 * still holds). */
int32_t gwamd_cigar_ops(const char* text, int64_t text_length, uint32_t* out_or_null, int64_t capacity,
                        int64_t* num_ops);

/* Overlaps and their CIGARs read from PAF text: the file path_or_null, or text_or_null of
 * text_length bytes (exactly one of the two).  Every non-empty line is one overlap, in order.
 * The read ids are the indices of columns 1 and 6 among the names (names[offsets[i],
 * offsets[i + 1]), as gwamd_format_paf takes them; of two equal names the first), the
 * positions come from columns 3-4 and 8-9, the strand from column 5, num_residues is column 10
 * divided by kmer_size and overlap_complete 0.  The ops are those of the cg:Z: tag, wherever
 * it stands among the tags; a line without one has none.
 * GWAMD_E_INVALID_ARGUMENT, with the number of the line (from 1) in gwamd_last_error(): a
 * name that is not among the names, fewer than 12 columns, a number that is not one, a strand
 * other than + and -, start > end, an end beyond the length in column 2 or 7, a CIGAR
 * gwamd_cigar_ops refuses; and kmer_size < 1, both or neither of path and text.  A file that
 * cannot be read is GWAMD_E_RUNTIME. */
typedef struct gwamd_paf gwamd_paf;

typedef struct gwamd_paf_view
{
    int64_t num_overlaps;
    int64_t num_ops;
    const gwamd_overlap* overlaps;
    const uint32_t* ops;       /* num_ops */
    const int64_t* op_offsets; /* num_overlaps + 1 */
} gwamd_paf_view;

int32_t gwamd_read_paf(const char* path_or_null, const char* text_or_null, int64_t text_length,
                       const char* query_names, const int64_t* query_name_offsets, int32_t num_queries,
                       const char* target_names, const int64_t* target_name_offsets, int32_t num_targets,
                       int32_t kmer_size, gwamd_paf** handle_out);
/* Pointers into the handle, valid until gwamd_paf_free. */
int32_t gwamd_paf_get(const gwamd_paf* paf, gwamd_paf_view* view);
void gwamd_paf_free(gwamd_paf* paf);

/* POA windows (host only).  Target r of length T has windows k = 0 .. ceil(T / w) - 1 with
 * backbone target[k w, min((k + 1) w, T)) as their first sequence.  A segment is kept when it has
 * no EMPTY, BAD_PATH or NOT_ALIGNED flag and (q_end - q_begin) * 50 >= w (racon's 2 % rule); kept
 * segments are appended to the window of their overlap's target in the order given, a REVERSE one
 * reverse-complemented (A<->T, C<->G, every position), at most max_sequences_per_window - 1 per
 * window.  GWAMD_E_INVALID_ARGUMENT for a segment whose overlap, window or query range is outside
 * the overlaps, the target's windows or the query read. */
typedef struct gwamd_windows gwamd_windows;

typedef struct gwamd_windows_view
{
    int64_t num_windows;
    int64_t num_sequences;
    int64_t num_bases;
    int64_t dropped_by_cap;          /* kept segments the cap left out */
    const char* bases;               /* the sequences, window after window, backbone first */
    const int64_t* sequence_offsets; /* num_sequences + 1 */
    const int32_t* window_counts;    /* sequences per window */
    const uint32_t* window_target;   /* target read id per window */
    const uint32_t* window_index;    /* k per window */
    const int32_t* sequence_overlap; /* overlap index per sequence, -1 for a backbone */
    const int32_t* sequence_t_begin; /* t_begin - k w (backbone: 0) */
    const int32_t* sequence_t_end;   /* t_end - k w (backbone: its length) */
} gwamd_windows_view;

int32_t gwamd_build_windows(const char* target_bases, const int64_t* target_offsets, int32_t num_targets,
                            const char* query_bases, const int64_t* query_offsets, int32_t num_queries,
                            const gwamd_overlap* overlaps, int64_t n, const gwamd_window_segment* segments,
                            int64_t num_segments, int32_t window_length, int32_t max_sequences_per_window,
                            gwamd_windows** out);
/* Pointers into the handle, valid until gwamd_windows_free. */
int32_t gwamd_windows_get(const gwamd_windows* windows, gwamd_windows_view* view);
void gwamd_windows_free(gwamd_windows* windows);

/* ---- windows as slices of resident reads ---------------------------------------
 *
 * A sequence of a POA group named, not copied: bases [begin, end) of read `read` of the set
 * sets[set], reverse-complemented (A<->T, C<->G, every other byte kept, every position) when
 * bit 0 of flags is set. */
#define GWAMD_SLICE_REVERSE 1u

typedef struct gwamd_read_slice
{
    int32_t set; /* index into the sets of the call */
    uint32_t read;
    uint32_t begin;
    uint32_t end;
    uint32_t flags;
} gwamd_read_slice;

/* gwamd_poa_add_poa_group for sequences that are slices of reads resident on the batch's
 * device: no base crosses the bus.  The bookkeeping is that of gwamd_poa_add_poa_group, so the
 * returned group status, per_seq_status (n entries), the batch's capacity and the window order
 * are those of adding the same sequences from the host.  gwamd_poa_upload / _generate_poa then
 * writes the bases on the device into the batch's input and, as base weights, quality - 33 of a
 * set that carries qualities (gwamd_device_reads_create_with_qualities; reversed, not
 * complemented, for a reverse slice) and the constant 1, cudapoa's default, of a set that does
 * not.  Host-added and resident groups may be mixed in one batch.
 *
 * The read sets must outlive the batch's use of them: until gwamd_poa_reset or
 * gwamd_poa_destroy_batch after the last gwamd_poa_generate_poa that uses them has completed.
 *
 * GWAMD_E_INVALID_ARGUMENT, before any device call and with the batch unchanged: a NULL batch,
 * sets array or set, NULL slices or per_seq_status with n > 0, n < 0, a set index outside
 * [0, num_sets), a read id outside its set, begin > end or end beyond the read's length (from
 * the handle's host copy of the offsets), a set on another device than the batch. */
int32_t gwamd_poa_add_poa_group_resident(gwamd_poa_batch* batch, const gwamd_device_reads* const* sets,
                                         int32_t num_sets, const gwamd_read_slice* slices, int32_t n,
                                         int32_t* per_seq_status);

/* gwamd_poa_add_poa_group_resident for num_groups groups in one call: group g is the next
 * group_counts[g] slices, and the call is equivalent to adding them one by one, in order.  It
 * stops before the first group the single call would answer exceeded_maximum_poas (1) for: the
 * batch is then as that call leaves it, *num_added counts the groups before it, and the caller
 * runs the batch and goes on from there.  A group with any other status is consumed (counted in
 * *num_added) and its status written to group_status[g]; per_seq_status has one entry per slice,
 * as the single call fills it.  Entries of the groups that were not reached are not written.
 * Every slice of every group is validated before the first group is added: an invalid one
 * (above), a negative count, or a NULL array with something behind it is
 * GWAMD_E_INVALID_ARGUMENT with the batch unchanged.  Returns 0, or 1 when it stopped early. */
int32_t gwamd_poa_add_poa_groups_resident(gwamd_poa_batch* batch, const gwamd_device_reads* const* sets,
                                          int32_t num_sets, const gwamd_read_slice* slices,
                                          const int32_t* group_counts, int32_t num_groups, int32_t* group_status,
                                          int32_t* per_seq_status, int32_t* num_added);

/* Test hook: the batch's packed bases and weights as gwamd_poa_upload left them on the device,
 * num_bases + 16 bytes each (the 16 bytes after the last base are zero); returns that count,
 * and only that with both outputs NULL. */
int32_t gwamd_internal_poa_download_inputs(gwamd_poa_batch* batch, uint8_t* seqs_out, int8_t* wts_out);

/* The grouping of gwamd_build_windows without the bases (host only): the same windows, keep
 * rule, order, cap and dropped_by_cap, each sequence a slice of set 0 (the targets: backbones)
 * or set 1 (the queries).  With query_qualities_or_null (one character per query base, at the
 * base's offset) a segment that passes the keep rule is dropped, before the cap is looked at,
 * when the mean of quality - 33 over [q_begin, q_end) is below quality_threshold_tenths / 10
 * (racon's rule), decided in integers: sum * 10 < quality_threshold_tenths * (q_end - q_begin).
 * A mean equal to the threshold keeps the segment. */
typedef struct gwamd_window_slices gwamd_window_slices;

typedef struct gwamd_window_slices_view
{
    int64_t num_windows;
    int64_t num_sequences;
    int64_t dropped_by_cap;
    int64_t dropped_by_quality;
    const gwamd_read_slice* slices;  /* num_sequences, window after window, backbone first */
    const int32_t* window_counts;    /* as in gwamd_windows_view */
    const uint32_t* window_target;
    const uint32_t* window_index;
    const int32_t* sequence_overlap;
    const int32_t* sequence_t_begin;
    const int32_t* sequence_t_end;
} gwamd_window_slices_view;

int32_t gwamd_build_window_slices(const int64_t* target_offsets, int32_t num_targets, const int64_t* query_offsets,
                                  int32_t num_queries, const char* query_qualities_or_null,
                                  int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                  const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
                                  int32_t max_sequences_per_window, gwamd_window_slices** out);
/* ---- the grouping on the device ---------------------------------------------------
 *
 * gwamd_build_window_slices with the work done by kernels on device_id: the given segments go
 * up, are classified, sorted stably by window and written out as slices; the view of the handle
 * equals gwamd_build_window_slices' in every array and both counters, and the same input gives
 * the same bytes.  The quality filter applies exactly when query_reads_or_null is given and
 * carries qualities (gwamd_device_reads_create_with_qualities): the characters are read where
 * they are resident.  Device arrays are counted against allocator_or_null's pool for the
 * duration of the call; an allocation the pool refuses is GWAMD_E_RUNTIME with the pool as it
 * was.  GWAMD_E_INVALID_ARGUMENT, before any device call, for what gwamd_build_window_slices
 * refuses and for a negative quality_threshold_tenths (with or without qualities), a negative
 * device_id, a handle on another device than device_id or whose reads are not those of
 * query_offsets, 2^31 or more windows, and windows plus segments (each of which may become a
 * sequence) of 2^31 or more. */
int32_t gwamd_build_window_slices_device(const int64_t* target_offsets, int32_t num_targets,
                                         const int64_t* query_offsets, int32_t num_queries,
                                         const gwamd_device_reads* query_reads_or_null,
                                         int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                         const gwamd_window_segment* segments, int64_t num_segments,
                                         int32_t window_length, int32_t max_sequences_per_window, int32_t device_id,
                                         struct gwamd_device_allocator* allocator_or_null, gwamd_window_slices** out);

/* Cut, then group, without a record on the host: only the overlaps (and the ops) go up and only
 * the grouped arrays come back.  With op_offsets_or_null NULL the overlaps are aligned on the
 * resident reads and cut as gwamd_window_segments_resident cuts them (an overlap beyond the
 * aligner's limits contributes nothing; num_alignment_engines engines); otherwise they are cut
 * from ops[op_offsets[i], op_offsets[i + 1]) in `convention` as gwamd_window_segments_cigar cuts
 * them, and num_alignment_engines is not looked at.  The records of the whole call lie in one
 * device array and are grouped once; the view equals that of gwamd_build_window_slices on the
 * records of the matching entry above, with the quality filter when query_reads carries
 * qualities.  The reads are on the current device.  GWAMD_E_INVALID_ARGUMENT, before any device
 * call: what those two entries refuse, an overlap that names a read or a position outside the
 * two sets, max_sequences_per_window < 1, a negative threshold, ops without op_offsets, and the
 * limits of gwamd_build_window_slices_device. */
int32_t gwamd_window_slices_resident(const gwamd_device_reads* query_reads, const gwamd_device_reads* target_reads,
                                     const gwamd_overlap* overlaps, int32_t n, const uint32_t* ops_or_null,
                                     const int64_t* op_offsets_or_null, int32_t convention, int32_t window_length,
                                     int32_t max_sequences_per_window, int32_t quality_threshold_tenths,
                                     int32_t num_alignment_engines, gwamd_window_slices** out);

/* Pointers into the handle, valid until gwamd_window_slices_free. */
int32_t gwamd_window_slices_get(const gwamd_window_slices* windows, gwamd_window_slices_view* view);
void gwamd_window_slices_free(gwamd_window_slices* windows);

/* racon's trimming of a window's consensus by coverage (window.cpp): with average =
 * (num_sequences - 1) / 2 (integer division; num_sequences counts the backbone), *begin is the
 * first index with coverage >= average and *past_the_end one past the last such index: the
 * trimmed consensus is consensus[*begin, *past_the_end).  When no index qualifies, or the first
 * is not before the last, the consensus is kept whole (0, length), where racon warns. */
int32_t gwamd_trim_consensus(const uint16_t* coverage, int32_t length, int32_t num_sequences, int32_t* begin,
                             int32_t* past_the_end);

/* Measurement hook (scripts/polish_group_bench.py): the arguments and checks of
 * gwamd_build_window_slices_device without a pool; the segments go up once and the records, then
 * resident, are grouped `repeats` times, each timed from the first launch to the grouped arrays'
 * arrival in host memory: seconds[0, repeats).  (When no target has a window nothing is timed.) */
int32_t gwamd_internal_group_repeat(const int64_t* target_offsets, int32_t num_targets, const int64_t* query_offsets,
                                    int32_t num_queries, const gwamd_device_reads* query_reads_or_null,
                                    int32_t quality_threshold_tenths, const gwamd_overlap* overlaps, int64_t n,
                                    const gwamd_window_segment* segments, int64_t num_segments, int32_t window_length,
                                    int32_t max_sequences_per_window, int32_t device_id, int32_t repeats,
                                    double* seconds);

/* Test hook: gwamd_window_segments on paths laid out as the aligner leaves them on the device,
 * end -> start, path i at paths[i * stride, i * stride + path_lengths[i]), stride a positive
 * multiple of 4.  The buffer is uploaded at its own size, n * stride bytes. */
int32_t gwamd_internal_window_segments_strided(const gwamd_overlap* overlaps, int64_t n, const int8_t* paths,
                                               const int32_t* path_lengths, int64_t stride,
                                               int32_t window_length, gwamd_window_segment** out,
                                               int64_t* num_out);

#ifdef __cplusplus
}
#endif

#endif
