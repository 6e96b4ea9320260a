// The banded POA kernel of a plan: one object per cells-per-lane value
// (poa_band_c<CPL>.o, each built from poa_band.hip; CPL = band width / 64 for
// the reference's band widths 128 .. 1,024) exports a resolver, listed here.
// The Makefile's BAND_CPLS is the same list: an object missing there is an
// unresolved symbol when the library loads.
#include "poa_common.hpp"

using namespace gwamd::poa;

#define GWAMD_BAND_CPLS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16)
#define GWAMD_BAND_DECL(N) extern "C" const void* gwamd_internal_poa_band_kernel_cpl##N(int, int, int);
GWAMD_BAND_CPLS(GWAMD_BAND_DECL)
#define GWAMD_BAND_ROW(N) {N, gwamd_internal_poa_band_kernel_cpl##N},
static const struct
{
    int cpl;
    const void* (*kernel)(int score_bits, int size_bits, int msa);
} kBandKernels[] = {GWAMD_BAND_CPLS(GWAMD_BAND_ROW)};

// (called by gwamd_internal_poa_kernel, poa_kernels.hip)
extern "C" KernelRef gwamd_internal_poa_band_kernel(const Dims* d, int score_bits, int size_bits, int msa)
{
    for (const auto& row : kBandKernels)
        if (row.cpl == d->lds_cpl)
            return {row.kernel(score_bits, size_bits, msa), kWave * (d->band_ad ? d->band_ad : 1),
                    size_t(d->lds_bytes)};
    return {nullptr, 0, 0};
}
