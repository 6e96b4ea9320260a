// The POA path's tuning and diagnostic switches: every GWAMD_* variable that
// changes the kernel plan or the launch, read in one function (and only with
// GWAMD_DIAG=1, diag_env.hpp).  DESIGN.md has the table of variables.
#pragma once

#include "diag_env.hpp"
#include "poa_common.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace gwamd
{
namespace poa
{

struct PoaTuning
{
    bool force_v1     = false;       // GWAMD_POA_KERNEL=v1: no LDS or banded kernel
    bool lds_shape    = false;       // GWAMD_POA_LDS_SHAPE="cpl,waves": forward-pass shape of the LDS kernel
    int lds_cpl       = 0;
    int lds_waves     = 0;
    int lds_pad       = 0;           // GWAMD_POA_LDS_PAD: LDS bytes added to the image (fewer windows per CU)
    int band_fwd      = 0;           // GWAMD_BAND_FWD=ad | row: 1 forces the anti-diagonal pass, 2 forbids it
    int band_ad_waves = kAdMaxWaves; // GWAMD_BAND_AD_WAVES: waves of that pass (1..kAdMaxWaves)
    int tb_rank       = kTbDefault;  // GWAMD_TB_WALK, GWAMD_TB_ABOVE: Dims::tb_rank
    int diag          = 0;           // Dims::diag (kDiag*)
    int slots         = 0;           // GWAMD_POA_SLOTS: a smaller persistent grid (0: as many as are resident)
    int order_cus     = 0;           // GWAMD_LAUNCH_ORDER_CUS: plan the launch order for this many CUs (0: the device's)
};

inline PoaTuning read_poa_tuning()
{
    using gwamd::host::diag_env;
    struct Choice
    {
        const char *name, *value; // value == nullptr: any non-zero integer
        int bits;
    };
    static const Choice kWalk[] = {{"GWAMD_TB_WALK", "scalar", kTbStrips},
                                   {"GWAMD_TB_WALK", "rect", kTbRanked},
                                   {"GWAMD_TB_WALK", "scalar_rect", 0},
                                   {"GWAMD_TB_WALK", "strip32", kTbRanked | kTbStrips | kTbStrip32},
                                   {"GWAMD_TB_WALK", "scalar_strip32", kTbStrips | kTbStrip32}};
    static const Choice kDiag[] = {{"GWAMD_TOPSORT_RING", nullptr, kDiagTopsortRing},
                                   {"GWAMD_POA_FWD", "v1", kDiagFwdV1},
                                   {"GWAMD_TOPSORT", "fifo", kDiagTopsortFifo},
                                   {"GWAMD_RACON", "v1", kDiagRaconV1},
                                   {"GWAMD_CONSENSUS", "hbm", kDiagConsensusHbm},
                                   {"GWAMD_POA_ADD", "wave0", kDiagAddWave0},
                                   {"GWAMD_POA_ADD", "serial", kDiagAddSerial},
                                   {"GWAMD_POA_ORDER", "kahn", kDiagOrderKahn},
                                   {"GWAMD_POA_SINK_CAP", "2", kDiagSinkCap2}};
    static const Choice kFwd[]  = {{"GWAMD_BAND_FWD", "ad", 1}, {"GWAMD_BAND_FWD", "row", 2}};
    auto is = [](const Choice& c) {
        const char* v = diag_env(c.name);
        return v && (c.value ? std::strcmp(v, c.value) == 0 : std::atoi(v) != 0);
    };
    auto number = [](const char* name, int unset) {
        const char* v = diag_env(name);
        return v ? std::atoi(v) : unset;
    };
    PoaTuning t;
    t.force_v1 = is({"GWAMD_POA_KERNEL", "v1", 0});
    if (const char* sh = diag_env("GWAMD_POA_LDS_SHAPE"))
        t.lds_shape = std::sscanf(sh, "%d,%d", &t.lds_cpl, &t.lds_waves) == 2;
    t.lds_pad = number("GWAMD_POA_LDS_PAD", 0);
    for (const Choice& c : kFwd)
        if (is(c))
            t.band_fwd = c.bits;
    t.band_ad_waves = std::max(1, std::min(kAdMaxWaves, number("GWAMD_BAND_AD_WAVES", kAdMaxWaves)));
    for (const Choice& c : kWalk)
        if (is(c))
            t.tb_rank = c.bits;
    if (diag_env("GWAMD_TB_ABOVE"))
        t.tb_rank |= (std::min(std::max(number("GWAMD_TB_ABOVE", 0), 0), 6) + 1) << kTbAboveShift;
    for (const Choice& c : kDiag)
        if (is(c))
            t.diag |= c.bits;
    if (diag_env("GWAMD_CONSENSUS_LDS_BYTES"))
        t.diag |= int(uint32_t(std::min(std::max(number("GWAMD_CONSENSUS_LDS_BYTES", 0), 1), 65535)) << kDiagConsLdsShift);
    t.slots     = std::max(0, number("GWAMD_POA_SLOTS", 0));
    t.order_cus = std::max(0, number("GWAMD_LAUNCH_ORDER_CUS", 0));
    return t;
}

} // namespace poa
} // namespace gwamd
