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
