// The POA kernel plan (poa_plan.cpp): pure functions of the batch capacities
// and the tuning switches.
#pragma once

#include "poa_common.hpp"
#include "poa_tuning.hpp"

namespace gwamd
{
namespace poa
{

// Plans the LDS-resident full-alignment kernel into `dims` (capacities filled
// by the caller); dims.lds_kernel stays 0 when it does not apply or fit.
void plan_lds_layout(Dims& dims, bool banded, int size_bits, int score_bits, const PoaTuning& tune);
// The bound of that kernel's packed 16-bit rows: E[i][j] = H[i][j] - j * gap fits int16 over the batch's columns
bool lds_e_domain_fits16(const Dims& dims, const Scores& sc);
// ... the banded kernel (dims.lds_kernel = 3), where the LDS kernel was not planned
void plan_band_kernel(Dims& dims, bool banded, int gap, int score_bits, const PoaTuning& tune);
// Both, and the diagnostic bits: all the batch constructor plans.  No LDS kernel for a full-alignment batch
// with 16-bit scores whose E range does not fit (it runs the global-memory kernel)
void plan_kernels(Dims& dims, bool banded, const Scores& sc, int score_bits, int size_bits, const PoaTuning& tune);

} // namespace poa
} // namespace gwamd
