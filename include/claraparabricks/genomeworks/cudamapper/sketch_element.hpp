// Direction of a sketch element's representation (reference
// cudamapper/include/claraparabricks/genomeworks/cudamapper/sketch_element.hpp:29-37).
#pragma once

#include <cstdint>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudamapper
{

class SketchElement
{
public:
    /// Whether the representation was read from the read as given or from its reverse complement.
    /// One byte wide: Index::directions_of_reads() is an array of these.
    enum class DirectionOfRepresentation : std::uint8_t
    {
        FORWARD = 0,
        REVERSE = 1
    };
};

} // namespace cudamapper
} // namespace genomeworks
} // namespace claraparabricks
