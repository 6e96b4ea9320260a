// The gate of the tuning and diagnostic switches (no HIP in here: the POA
// planner's tuning parser includes it).
#pragma once

#include <cstdlib>

namespace gwamd
{
namespace host
{

// Tuning and diagnostic switches (GWAMD_POA_KERNEL, GWAMD_TB_WALK,
// GWAMD_BAND_FWD, ...): read only when GWAMD_DIAG=1 is set, so a drop-in
// user's environment never changes which kernel runs.  The parity tests set
// GWAMD_DIAG=1 (tests/conftest.py).  GWAMD_SPOA_ACCURATE is not one of them:
// it is the runtime form of the reference's spoa_accurate build option.
inline bool diag_enabled()
{
    const char* d = std::getenv("GWAMD_DIAG");
    return d && d[0] == '1' && d[1] == '\0';
}
inline const char* diag_env(const char* name) { return diag_enabled() ? std::getenv(name) : nullptr; }

} // namespace host
} // namespace gwamd
