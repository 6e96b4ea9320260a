// Anchor matcher of cudamapper on the MI355X (reference
// cudamapper/include/claraparabricks/genomeworks/cudamapper/matcher.hpp:29-49).
#pragma once

#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include <memory>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class Matcher
{
public:
    virtual ~Matcher() = default;

    /// All pairs of a query and a target sketch element of equal
    /// representation, sorted by (query_read_id, target_read_id,
    /// query_position_in_read, target_position_in_read).
    virtual device_buffer<Anchor>& anchors() = 0;

    /// Matches two indices built by Index::create_index (they may be the same
    /// index; self-matches are kept).  Throws std::runtime_error for more than
    /// 2^31 anchors.
    static std::unique_ptr<Matcher> create_matcher(DefaultDeviceAllocator allocator, const Index& query_index,
                                                   const Index& target_index, const hipStream_t stream = 0);
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

namespace claragenomics = claraparabricks::genomeworks;
