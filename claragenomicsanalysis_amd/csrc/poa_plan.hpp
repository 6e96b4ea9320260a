// The POA host plan (poa_plan.cpp): the kernel plan, the batch's capacity, its
// device layout and its window order, as pure functions of the batch
// capacities, the device's facts and the tuning switches.
#pragma once

#include "poa_common.hpp"
#include "poa_tuning.hpp"

#include <cstdint>
#include <vector>

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

// --- capacity, device layout and window order of a batch --------------------

// What the capacity needs to know of the device
struct PoaDeviceFacts
{
    int32_t cus           = 0;
    int32_t blocks_per_cu = 0; // resident workgroups per CU of the planned kernel (0: no answer, or the v1 kernel)
};

// The BatchSize numbers (cudapoa/batch.hpp) of the batch's alignment mode
struct RefSizes
{
    int64_t seq_len, consensus, seqs; // max_sequence_size, max_consensus_size, max_sequences_per_poa
    int64_t nodes, graph_dim;         // max_nodes_per_window, max_matrix_graph_dimension, or their _banded twins
    int64_t seq_dim;                  // max_matrix_sequence_dimension, banded: the band width + kBandPad
};

struct PoaCapacity
{
    int32_t max_poas = 0; // windows the batch holds
    int32_t slots    = 0; // scratch slots (persistent grid size for the LDS / banded kernels)
    int32_t resident = 0; // workgroups resident on the device at once (0: v1 kernel, or no occupancy answer)
    int64_t scorebuf_alloc = 0; // the reference's score budget (reserve_buf)
    int64_t window_bytes = 0, slot_bytes = 0; // this build's estimate per window and per slot
};

// Device bytes per window as accounted by the reference (allocate_block.hpp:292-338)
int64_t reference_device_bytes_per_poa(const RefSizes& rs, bool msa, int size_bytes);

// The reference's max_mem / (per window + score matrix), this build's own
// footprint (a slot per window, or only as many as the persistent grid has
// workgroups), GWAMD_POA_SLOTS, and the score budget.  `dims` is planned
// (plan_kernels).  Throws std::runtime_error where the reference does.
PoaCapacity plan_capacity(const PoaDeviceFacts& facts, const Dims& dims, const RefSizes& rs, int size_bytes,
                          int score_bytes, bool msa, int64_t max_mem, int tune_slots);

// The slab's arrays in slab order, F(Buffers member, bytes): the one list.
// The bytes are written over plan_layout's locals: P windows, Z slots, mn
// nodes, E edges, S reads, sz size bytes, d the Dims, msa.
#define GWAMD_POA_SLAB_ARRAYS(F)                                                                              \
    F(base, P * mn) F(in_cnt, P * mn * 2) F(out_cnt, P * mn * 2) F(aln_cnt, P * mn * 2)                      \
    F(node_cov, P * mn * 2) F(in_w, P * mn * E * 2) F(in_e, P * mn * E * sz) F(out_e, P * mn * E * sz)       \
    F(aln, P * mn * E * sz) F(sorted, P * mn * sz) F(pos, P * mn * sz) F(ag, Z * d.aln_cap * sz)             \
    F(ar, Z * d.aln_cap * sz) F(cscore, Z * mn * 4) F(cpred, Z * mn * 4 * sz) F(cons, P * d.max_consensus)   \
    F(cov, P * d.max_consensus * 2) F(cons_len, P * 4) F(status, P) F(msa_status, P) F(msa_len, P * 4)       \
    F(final_nodes, P * 4) F(cells, P * 8) F(phase, P * 8 * kPhases) F(order_stats, P * 4 * kOrderStats)      \
    F(edge_cov, msa ? P * mn * E * S * 2 : 0) F(edge_cov_cnt, msa ? P * mn * E * 2 : 0)                      \
    F(seq_begin, msa ? P * S * sz : 0) F(msa, msa ? P * S * d.max_consensus : 0)

// Where everything the batch allocates lies.  Slab offsets are named after
// their Buffers member; -1: the array is empty and its pointer stays null.
struct PoaLayout
{
#define GWAMD_F(name, bytes) int64_t name = -1;
    GWAMD_POA_SLAB_ARRAYS(GWAMD_F)
#undef GWAMD_F
    int64_t scores      = 0; // the score matrices, last and 256-B aligned
    int64_t slab_bytes  = 0;
    int64_t codes_bytes = 0; // Buffers::codes, an allocation of its own (LDS and banded kernels)
    int64_t seqs_bytes = 0, wts_bytes = 0, len_bytes = 0, off_bytes = 0; // the input arrays
    // the window buffer: WindowDesc[max_poas] | order int32[max_poas] | dequeue head int32, each 16-B aligned
    int64_t win_bytes = 0, order_off = 0, head_off = 0;
    int64_t device_bytes() const
    {
        return slab_bytes + codes_bytes + seqs_bytes + wts_bytes + len_bytes + off_bytes + win_bytes;
    }
};
PoaLayout plan_layout(const Dims& dims, int size_bytes, int score_bytes, bool msa, int32_t max_poas, int32_t slots);

// Queue order of the windows.  Workgroups i, i + C, i + 2C, ... (C = CUs)
// share a CU; windows are ranked by estimated DP cells (-sum * max of the read
// lengths, ties by window) and the first grid's worth is dealt to those rounds
// in snake order, so every CU gets a mix of heavy and light windows.  When a
// persistent kernel's batch holds more windows than slots, the rest follow
// heaviest first and are dequeued by whichever workgroup finishes first
// (longest processing time first).  Outputs stay indexed by window.
enum WindowOrder
{
    kNoOrder      = 0, // position i is window i (`order` untouched)
    kOrder        = 1,
    kOrderAndHead = 2, // ... and the workgroups dequeue past the first `slots` positions
};
WindowOrder plan_window_order(const WindowDesc* windows, const int32_t* seq_len, int n, int cus, int slots,
                              bool persistent_kernel, std::vector<int32_t>& order);

} // namespace poa
} // namespace gwamd
