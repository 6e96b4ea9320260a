// The aligner path's tuning and diagnostic switches: every GWAMD_* variable
// that changes the aligner's plan or its launches, read in one function (and
// only with GWAMD_DIAG=1, diag_env.hpp).  An aligner reads them once, when it
// is constructed.  DESIGN.md has the table of variables.
#pragma once

#include "diag_env.hpp"

#include <cerrno>
#include <cstdlib>
#include <string>

namespace gwamd
{
namespace aln
{

// One variable as given: unset is not the same as any value.  Range checks
// belong to the code that uses the value (aligner_plan.cpp), so a switch of
// one algorithm never refuses an aligner of another.
struct Switch
{
    bool set = false;
    std::string text;
    // the value when the text is one whole decimal number and lies in [lo, hi]
    bool number_in(long lo, long hi, long& v) const
    {
        char* end = nullptr;
        errno     = 0;
        v         = std::strtol(text.c_str(), &end, 10);
        return set && end != text.c_str() && *end == '\0' && errno == 0 && v >= lo && v <= hi;
    }
};

struct AlignerTuning
{
    Switch band_tile_bytes;  // GWAMD_BAND_TILE_BYTES: banded Myers, LDS bytes of the chunk state / backtrace tile
    Switch band_waves;       // GWAMD_BAND_WAVES: banded Myers, waves per pair at every launch
    Switch uk_tile_bytes;    // GWAMD_UK_TILE_BYTES: Ukkonen, LDS bytes of the single-wave kernel's backtrace tile
    Switch hm_stripe_blocks; // GWAMD_HM_STRIPE_BLOCKS: Hirschberg-Myers, long mode with stripes of this many blocks
    Switch grid;             // GWAMD_ALIGNER_GRID: workspace slots per CU instead of the occupancy query's answer
    Switch band_spec;        // GWAMD_BAND_SPEC: banded Myers, sweeps of the band doubling run ahead
    Switch pipeline;         // GWAMD_ALIGNER_PIPELINE: stages of align_all()
};

inline AlignerTuning read_aligner_tuning()
{
    auto given = [](const char* name) {
        const char* v = gwamd::host::diag_env(name);
        return v ? Switch{true, v} : Switch{};
    };
    AlignerTuning t;
    t.band_tile_bytes  = given("GWAMD_BAND_TILE_BYTES");
    t.band_waves       = given("GWAMD_BAND_WAVES");
    t.uk_tile_bytes    = given("GWAMD_UK_TILE_BYTES");
    t.hm_stripe_blocks = given("GWAMD_HM_STRIPE_BLOCKS");
    t.grid             = given("GWAMD_ALIGNER_GRID");
    t.band_spec        = given("GWAMD_BAND_SPEC");
    t.pipeline         = given("GWAMD_ALIGNER_PIPELINE");
    return t;
}

} // namespace aln
} // namespace gwamd
