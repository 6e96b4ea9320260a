// The aligner's internal entry for overlaps whose reads are resident on its
// device (aligner_batch.cpp, AlignerGlobalHip::add_device_overlaps); used by
// the alignment engines (overlap_engines.hpp, overlap_align.cpp) and by
// cudapolish's cut on the device paths (polish_windows_host.cpp), not part of
// the public Aligner interface.
#pragma once

#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>

#include "mapper_reads.hpp"

namespace gwamd
{
namespace aln
{

// Adds the regions of `count` overlaps to the aligner's batch, all or none.
// generic_error when the batch already holds host-added pairs (and
// add_alignment returns it on a batch that holds device-added ones), or when
// the reads are on another device than the aligner; otherwise the status
// add_alignment would give the first pair that cannot be added.  The overlaps
// have been checked against the reads (gwamd::mapper::check_overlaps).
claraparabricks::genomeworks::cudaaligner::StatusType
add_device_overlaps(claraparabricks::genomeworks::cudaaligner::Aligner& aligner, const gwamd::mapper::DeviceReads& query,
                    const gwamd::mapper::DeviceReads& target, const gwamd::mapper::OverlapRecord* overlaps,
                    int32_t count);

// Where the aligner's kernels leave the paths of its batch: path i, emitted
// end -> start, at paths + i * max_path_length (a multiple of 4), its length at
// lengths[i]; `bytes` is the allocation behind paths.  Work queued on stream
// after align_all() finds them complete.
struct DevicePaths
{
    const int8_t* paths;
    int64_t bytes;
    const int32_t* lengths;
    int32_t max_path_length;
    hipStream_t stream;
};
DevicePaths device_paths(claraparabricks::genomeworks::cudaaligner::Aligner& aligner);

// With keep == true align_all() leaves the paths on the device: nothing is
// copied to the host, and the caller reads them through device_paths() and
// calls reset() without sync_alignments().
void keep_paths_on_device(claraparabricks::genomeworks::cudaaligner::Aligner& aligner, bool keep);

} // namespace aln
} // namespace gwamd
