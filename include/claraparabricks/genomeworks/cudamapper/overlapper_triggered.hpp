// OverlapperTriggered of cudamapper on the MI355X (reference
// cudamapper/src/overlapper_triggered.hpp:34-62): anchors are chained while
// neighbours stay within reach of each other, chains of three or more are
// fused into overlaps and the overlaps filtered, all on the GPU.  hipStream_t
// stands where the reference has cudaStream_t.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/overlapper.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <hip/hip_runtime_api.h>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class OverlapperTriggered : public Overlapper
{
public:
    explicit OverlapperTriggered(DefaultDeviceAllocator allocator, const hipStream_t stream = 0);

    /// Device memory is counted against the allocator's pool.
    void get_overlaps(std::vector<Overlap>& fused_overlaps, const device_buffer<Anchor>& d_anchors,
                      int64_t min_residues = 20, int64_t min_overlap_len = 50, int64_t min_bases_per_residue = 50,
                      float min_overlap_fraction = 0.9) override;

private:
    DefaultDeviceAllocator allocator_;
    hipStream_t stream_;
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks
