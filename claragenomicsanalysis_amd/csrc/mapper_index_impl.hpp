// The Index that Index::create_index and IndexHostCopyBase::copy_index_to_device
// make (mapper_batch.cpp, mapper_index_cache.cpp): gwamd::mapper::IndexData behind the
// public accessors.
#pragma once

#include <claraparabricks/genomeworks/cudamapper/index.hpp>

#include "mapper_common.hpp"

#include <cstddef>
#include <memory>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class IndexHip : public Index
{
public:
    using Direction = SketchElement::DirectionOfRepresentation;
    static_assert(sizeof(Direction) == 1, "directions are stored as bytes");

    gwamd::mapper::IndexData data;

    void refresh_views()
    {
        representations_    = {data.representations.data(), std::ptrdiff_t(data.representations.size())};
        read_ids_           = {data.read_ids.data(), std::ptrdiff_t(data.read_ids.size())};
        positions_in_reads_ = {data.positions_in_reads.data(), std::ptrdiff_t(data.positions_in_reads.size())};
        directions_         = {reinterpret_cast<Direction*>(data.directions_of_reads.data()),
                       std::ptrdiff_t(data.directions_of_reads.size())};
        unique_             = {data.unique_representations.data(), std::ptrdiff_t(data.unique_representations.size())};
        first_occurrence_   = {data.first_occurrence_of_representations.data(),
                             std::ptrdiff_t(data.first_occurrence_of_representations.size())};
    }

    const device_buffer<representation_t>& representations() const override { return representations_; }
    const device_buffer<read_id_t>& read_ids() const override { return read_ids_; }
    const device_buffer<position_in_read_t>& positions_in_reads() const override { return positions_in_reads_; }
    const device_buffer<Direction>& directions_of_reads() const override { return directions_; }
    const device_buffer<representation_t>& unique_representations() const override { return unique_; }
    const device_buffer<std::uint32_t>& first_occurrence_of_representations() const override
    {
        return first_occurrence_;
    }
    read_id_t number_of_reads() const override { return data.number_of_reads; }
    read_id_t smallest_read_id() const override { return data.smallest_read_id; }
    read_id_t largest_read_id() const override { return data.largest_read_id; }
    position_in_read_t number_of_basepairs_in_longest_read() const override
    {
        return data.number_of_basepairs_in_longest_read;
    }

private:
    device_buffer<representation_t> representations_, unique_;
    device_buffer<read_id_t> read_ids_;
    device_buffer<position_in_read_t> positions_in_reads_;
    device_buffer<Direction> directions_;
    device_buffer<std::uint32_t> first_occurrence_;
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks

// the C ABI's index handle (include/gwamd_cudamapper.h)
struct gwamd_index
{
    std::unique_ptr<claraparabricks::genomeworks::cudamapper::IndexHip> impl;
};
