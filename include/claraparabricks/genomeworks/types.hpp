// Basic id/position types (reference common/base/include/claraparabricks/genomeworks/types.hpp:30-58).
#pragma once

#include <cstdint>
#include <string_view>

namespace claraparabricks
{
namespace genomeworks
{

using read_id_t             = std::uint32_t; ///< read index within a parser
using number_of_reads_t     = read_id_t;
using position_in_read_t    = std::uint32_t; ///< base position within a read
using number_of_basepairs_t = position_in_read_t;
using gw_string_view_t      = std::string_view; ///< this build is C++17 throughout

} // namespace genomeworks
} // namespace claraparabricks
