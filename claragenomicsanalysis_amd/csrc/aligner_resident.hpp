// The aligner's internal entry for overlaps whose reads are resident on its
// device (aligner_batch.cpp, AlignerGlobalHip::add_device_overlaps); used by
// the overlap-alignment caller (overlap_align.cpp), not part of the public
// Aligner interface.
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

} // namespace aln
} // namespace gwamd
