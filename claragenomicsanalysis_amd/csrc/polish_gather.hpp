// The POA batch's input arrays filled on the device (polish_gather.hip): the
// sequences a batch was given as slices of resident reads
// (gwamd_poa_add_poa_group_resident, poa_batch.cpp) are written into its packed
// bases and weights at their seq_off, from the reads and qualities of
// mapper::DeviceReads.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gwamd
{
namespace polish
{

// One resident sequence of a batch, as the kernel reads it: eight 32-bit words.
// The host forms the two source addresses from the handle's own copy of the
// offsets after it has checked the slice against them.
struct SliceJob
{
    const uint8_t* bases; // device: the slice's first base, read[begin]
    const uint8_t* quals; // device: its first quality character, or null (every weight is 1)
    int64_t dst;          // seq_off of the sequence in the batch's packed arrays
    uint32_t len;         // end - begin
    uint32_t reverse;     // 1: reverse-complemented bases, reversed weights
};
static_assert(sizeof(SliceJob) == 32, "SliceJob is eight 32-bit words");

// Sequence i of the n device jobs: seqs[dst, dst + len) receives the slice's
// bases, reverse-complemented (A<->T, C<->G, every other byte kept, every
// position) when reverse is set, and wts[dst, dst + len) quality - 33 per base
// in the same order, or 1 without qualities.  Nothing outside these ranges is
// written.  max_len: the longest of the n slices.  seqs and wts are 16-byte
// aligned.  Asynchronous on stream.
void gather_poa_slices(uint8_t* seqs, int8_t* wts, const SliceJob* d_jobs, int64_t n, int64_t max_len,
                       hipStream_t stream);

} // namespace polish
} // namespace gwamd
