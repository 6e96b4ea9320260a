// The POA kernel plan: which kernel a batch of given capacities runs and the
// layout of its LDS image and HBM side buffers, as a function of the
// capacities and the tuning switches alone; then how many windows and scratch
// slots the batch gets for its memory (plan_capacity), where every device
// array lies (plan_layout) and the order its windows are queued in
// (plan_window_order).  No HIP in here, so the plan can be examined (and
// sanitized) on the host: gwamd_internal_poa_plan, gwamd_internal_poa_capacity,
// gwamd_internal_poa_window_order.
#include "poa_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <iterator>
#include <stdexcept>
#include <string>
#include <utility>

namespace gwamd
{
namespace poa
{

// LDS-resident kernel (poa_window_kernel_lds): full alignment with 16-bit
// scores and node ids.  LDS image per window: read | ring of E rows (also
// the traceback tile and the add-alignment scratch) | row program |
// predecessor lists | shared words; the topological sort reuses everything
// below the shared words.  Span carries of multi-sweep reads live in HBM
// next to the traceback codes.
//
// 16-bit rows hold E[i][j] = H[i][j] - j * gap, not H.  The reference's width
// rule (cudapoa_limits.hpp:28-37) bounds H by upper = max_sequence_size * match
// and lower = max_sequence_size * max(gap, mismatch) + (graph rows -
// max_sequence_size) * gap; over the columns j <= max_sequence_size E then lies
// in [lower - max_sequence_size * max(gap, 0), upper - max_sequence_size *
// min(gap, 0)] (a read equal to its graph reaches j * (match - gap) at cell
// (j, j)).  That range can pass int16 where H does not, e.g. gap -20, match 40
// at 600 bases: 36,000.  Such a batch keeps the reference's 16-bit types and
// runs the global-memory kernel, which works in H (plan_kernels).
bool lds_e_domain_fits16(const Dims& dims, const Scores& sc)
{
    const int64_t ms    = dims.max_seq_len;
    const int64_t upper = ms * sc.match;
    const int64_t lower = ms * std::max(sc.gap, sc.mismatch) + (int64_t(dims.max_nodes) - ms) * sc.gap;
    return upper - ms * std::min(sc.gap, 0) <= INT16_MAX && lower - ms * std::max(sc.gap, 0) >= INT16_MIN;
}

void plan_lds_layout(Dims& dims, bool banded, int size_bits, int score_bits, const PoaTuning& tune)
{
    dims.lds_kernel = 0;
    if (tune.force_v1)
        return;
    // 16-bit node ids; 16-bit scores, or 32-bit ones (the reference's
    // use32bitScore batches: nw_forward_lds_w)
    if (banded || size_bits != 16 || (score_bits != 16 && score_bits != 32))
        return;
    const bool wide      = score_bits == 32;
    auto a16             = [](int64_t v) { return (v + 15) & ~int64_t(15); };
    int ring_rows        = 8;
    const int64_t read_b = lds_read_bytes(dims.max_seq_len);
    // forward pass shape: CPL columns per lane on NW waves; a sweep covers
    // NW*64*CPL read columns, longer reads take several sweeps
    // (GWAMD_POA_LDS_SHAPE="cpl,waves": any row of kLdsShapes of this
    // width).  32-bit scores: one sweep up to 4,096 columns (8 waves), 8,192
    // with 16 columns per lane
    int cpl = 8, nw = 1;
    const int ms = dims.max_seq_len;
    if (!wide && ms > 512)
        nw = 2;
    if (wide)
    {
        nw  = ms <= 512 ? 1 : (ms <= 1024 ? 2 : (ms <= 2048 ? 4 : 8));
        cpl = ms <= 4096 ? 8 : 16;
    }
    if (tune.lds_shape)
    {
        const auto* e = std::end(kLdsShapes);
        if (std::none_of(kLdsShapes, e, [&](const LdsShape& s) {
                return s.cpl == tune.lds_cpl && s.waves == tune.lds_waves && s.wide == wide;
            }))
            throw std::invalid_argument("GWAMD_POA_LDS_SHAPE: unsupported columns/waves pair");
        cpl = tune.lds_cpl, nw = tune.lds_waves;
    }
    const int ebytes     = wide ? 4 : 2;
    // the one-wave graph update's scratch always fits the ring region
    // (this is lds_add_wave0_bytes rounded up); the every-wave update's
    // larger one is not planned for: the kernel runs it where
    // lds_add_fits(max_seq_len, max_nodes, lds_rec_off - lds_ring_off)
    const int64_t add_b  = 5 * a16(dims.max_seq_len + 16) + 2 * (int64_t(dims.max_nodes) + dims.max_seq_len);
    const int64_t tile_b = int64_t(kTileRows) * kTileCols + kTbRankBytes;
    const int64_t rec_b  = a16(int64_t(dims.max_nodes + 2) * 4);
    const int64_t sh_b   = a16(wide ? kShBytesW(nw) : kShBytes(nw));
    auto ring_bytes      = [&](int rows) {
        return a16(std::max<int64_t>({int64_t(rows) * dims.score_stride * ebytes, tile_b, add_b}));
    };
    int64_t ring_b       = ring_bytes(ring_rows);
    int64_t fixed        = read_b + ring_b + rec_b + sh_b;
    int64_t target       = 40960 - 16; // 4 workgroups per CU incl. static LDS: one batch of
                                       // 1024 windows is resident on the 256 CUs at once
    if (wide)
    {
        // 32-bit rows are twice as wide: two windows per CU when their
        // images fit, else one; an 8-row ring when it fits, else 4 rows
        // (predecessors farther back go through the HBM spill rows)
        int64_t chosen = 0;
        for (int64_t budget : {int64_t(81920 - 16), int64_t(163840 - 64)})
        {
            for (int rows : {8, 4})
            {
                const int64_t rb = ring_bytes(rows);
                const int64_t fx = read_b + rb + rec_b + sh_b;
                if (fx + 2048 <= budget)
                {
                    ring_rows = rows, ring_b = rb, fixed = fx, chosen = budget;
                    break;
                }
            }
            if (chosen)
                break;
        }
        if (!chosen)
            return;
        target = chosen;
    }
    int64_t xl_cap       = std::max<int64_t>(1024, (target - fixed) / 2);
    xl_cap               = std::min<int64_t>(xl_cap, 65535);
    int64_t total        = fixed + a16(xl_cap * 2);
    total += a16(tune.lds_pad); // diagnostic: fewer windows per CU
    if (total > (wide ? 163840 - 64 : 65536))
        return;
    dims.lds_kernel    = 1;
    dims.tb_rank       = tune.tb_rank;
    dims.lds_ring_off  = int32_t(read_b);
    dims.lds_ring_rows = ring_rows;
    dims.lds_rec_off   = int32_t(read_b + ring_b);
    dims.lds_xl_off    = int32_t(read_b + ring_b + rec_b);
    dims.lds_xl_cap    = int32_t(xl_cap);
    dims.lds_sh_off    = int32_t(read_b + ring_b + rec_b + a16(xl_cap * 2));
    dims.lds_bytes     = int32_t(total);
    dims.lds_cpl       = cpl;
    dims.lds_waves     = nw;
    dims.code_stride   = int32_t(a16(int64_t(dims.max_seq_len) + 48));
    // HBM side buffer per window: traceback codes, span carries
    const int64_t code_b = int64_t(dims.score_rows) * dims.code_stride;
    const int64_t cr_b   = a16(int64_t(dims.max_nodes + 2) * ebytes);
    dims.aux_carry_off  = int32_t(code_b);
    dims.aux_stride     = code_b + cr_b;
}

// Banded kernel (poa_window_kernel_band, poa_band.hip): band widths 128 to
// 1,024 in steps of 128 (2 to 16 cells per lane), gap <= 0.  LDS image per window: staged
// read | work region (row-program flags, the 16-row ring of band rows, the
// traceback tile, the add-alignment scratch; the topological sort also
// reuses the read) | shared words.  Windows per CU: 4, 2 or 1, the most
// that leave room for the work region at this batch's maximum sizes.
void plan_band_kernel(Dims& dims, bool banded, int gap, int score_bits, const PoaTuning& tune)
{
    if (!banded || dims.lds_kernel || tune.force_v1)
        return;
    const int bw = dims.band_width;
    // every band width the reference accepts up to 1,024 (multiples of
    // 128, batch.hpp:85-94): CPL = bw / 64 cells per lane, one
    // object per CPL (poa_band_c<CPL>.o)
    if (bw % 128 != 0 || bw < 128 || bw > 1024 || gap > 0)
        return;
    auto a16          = [](int64_t v) { return (v + 15) & ~int64_t(15); };
    const int cpl     = bw / 64;
    const int sbytes  = score_bits / 8;
    // band row: position idx + cpl - 1, whole cpl-cell groups (66-67 of them)
    const int rowsz   = (bw + kBandPad + cpl + cpl - 1) / cpl * cpl;
    const int64_t ms  = dims.max_seq_len, mn = dims.max_nodes;
    const int64_t read_b  = a16(kReadGuard + ms + bw + 48);
    const int64_t sh_b    = 64;
    const int ring_rows   = band_ring_rows(cpl), tile_rows = band_tile_rows(cpl);
    const int64_t ring_b  = a16(int64_t(ring_rows) * rowsz * sbytes) + 4 * 256 * 4 + 1024 * 4; // + record staging
    const int64_t tile_b  = a16(int64_t(tile_rows) * bw + 64 * 16 + 512 + kTbRankBytes); // codes +
                                                                  // per-row decode info + walk tables
    const int64_t flags_b = 2 * a16(mn + 2); // row program: spill and far flags
    const int64_t add_b   = 7 * a16(ms + 16) + a16(2 * (mn + ms + 16)); // + the edge-slot bytes
    // anti-diagonal forward pass (poa_band_ad.hpp): a kAdRing-row ring and
    // one dummy word per lane.  Default: whenever the windows-per-CU
    // choice below leaves room for it (large windows, one or two per CU);
    // GWAMD_BAND_FWD=ad|row forces it on (planning for it) or off.
    const int64_t ad_b    = a16(int64_t(kAdRing) * rowsz * sbytes + kWave * sbytes) +
                         a16(mn / 8 + 64); // + the real-row bitmap
    // (band widths 128 / 256 only: its ring of kAdRing rows is too large beyond)
    const bool force_ad   = tune.band_fwd == 1 && cpl <= 4;
    const bool no_ad      = tune.band_fwd == 2;
    const int64_t min_w   = std::max({ring_b, tile_b, flags_b, force_ad ? ad_b : int64_t(0)});
    const int64_t want_w  = std::max(min_w, add_b);
    const int64_t kStatic = 256; // static __shared__ bytes of the kernel
    int64_t total         = 0;
    int chosen_per_cu     = 1;
    for (int per_cu : {4, 2, 1})
    {
        const int64_t budget = (163840 / per_cu - kStatic) & ~int64_t(15);
        if ((!force_ad && read_b + want_w + sh_b <= budget) || per_cu == 1)
        {
            total         = budget;
            chosen_per_cu = per_cu;
            break;
        }
    }
    const int64_t work = total - read_b - sh_b;
    if (work < min_w)
        return;
    dims.lds_kernel     = 3;
    // the pass runs kAdMaxWaves waves per window (GWAMD_BAND_AD_WAVES: fewer): one window per CU
    dims.band_ad        = (!no_ad && cpl <= 4 && chosen_per_cu == 1 && work >= ad_b) ? tune.band_ad_waves : 0;
    dims.tb_rank        = tune.tb_rank;
    dims.lds_cpl        = cpl;
    dims.lds_waves      = 1;
    dims.lds_bytes      = int32_t(total);
    dims.lds_ring_off   = int32_t(read_b);
    dims.lds_ring_rows  = ring_rows;
    dims.lds_work_bytes = int32_t(work);
    dims.lds_sh_off     = int32_t(read_b + work);
    dims.score_stride   = rowsz; // spill rows: band row at position idx + cpl - 1
    dims.code_stride    = bw;
    const int64_t rows   = dims.score_rows;
    int64_t o            = a16(rows * bw); // codes
    dims.aux_reca_off   = int32_t(o);
    o += a16(rows * 4);
    dims.aux_recb_off = int32_t(o);
    o += a16(rows * 4);
    dims.aux_col0_off = int32_t(o);
    o += a16(rows * 4);
    dims.aux_flag_off = int32_t(o);
    o += a16(rows);
    dims.aux_xl_off = int32_t(o);
    dims.aux_xl_cap = int32_t(2 * mn + 64);
    o += a16(int64_t(dims.aux_xl_cap) * 4);
    dims.aux_bx_off = int32_t(o);
    o += a16((rows / 256 + 2) * 4);
    dims.aux_recc_off = int32_t(o);
    o += a16(rows * 4);
    dims.aux_rece_off = int32_t(o);
    o += a16(rows * 4);
    dims.aux_stride = o;
}

void plan_kernels(Dims& dims, bool banded, const Scores& sc, int score_bits, int size_bits, const PoaTuning& tune)
{
    dims.lds_kernel = 0;
    if (banded || score_bits != 16 || lds_e_domain_fits16(dims, sc))
        plan_lds_layout(dims, banded, size_bits, score_bits, tune);
    plan_band_kernel(dims, banded, sc.gap, score_bits, tune);
    dims.diag = tune.diag;
}

namespace
{

inline int64_t align8(int64_t v) { return (v + 7) & ~int64_t(7); }
inline int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }

// Graph, inputs and outputs of one window: an estimate for the capacity, made
// before the layout existed and kept as it is because max_poas follows from it
// (it has a flat 32 B where the slab has the phase, cells, final_nodes and
// order_stats arrays).
int64_t window_bytes(const Dims& d, int sz, bool msa)
{
    const int64_t mn = d.max_nodes, E = kMaxEdges, S = d.max_seqs;
    int64_t b        = 0;
    b += align8(mn) + 4 * align8(mn * 2) + align8(mn * E * 2);   // base, counts, coverage, in_w
    b += 3 * align8(mn * E * sz) + 2 * align8(mn * sz);           // in_e, out_e, aln, sorted, pos
    b += align8(d.max_consensus) + align8(int64_t(d.max_consensus) * 2) + 32; // outputs
    b += int64_t(S) * d.max_seq_len * 2 + S * 12;                 // inputs
    if (msa)
        b += align8(mn * E * S * 2) + align8(mn * E * 2) + align8(S * sz) + align8(S * int64_t(d.max_consensus));
    return b;
}

// Forward-pass / traceback / consensus scratch of one slot.
int64_t slot_bytes(const Dims& d, int sz, int sbytes)
{
    const int64_t mn = d.max_nodes;
    int64_t b        = 0;
    b += 2 * align8(int64_t(d.aln_cap) * sz);                 // ag, ar
    b += int64_t(d.score_rows) * d.score_stride * sbytes;     // scores (LDS kernel: spill rows)
    if (d.lds_kernel)
        b += d.aux_stride; // traceback codes, row program, predecessor lists, carries
    b += align8(mn * 4) + align8(mn * 4 * sz);                // cscore, cpred
    return b;
}

// Non-score bytes of the reference slab for P windows
// (allocate_block.hpp:121-285, each buffer aligned to 8 B).
int64_t reference_fixed_slab(const RefSizes& rs, int64_t P, int sz, bool msa, bool cons)
{
    const int64_t S = rs.seqs, E = kMaxEdges, nodes = rs.nodes, gdim = rs.graph_dim;
    int64_t o       = 0;
    o += align8(P * rs.consensus);
    o += cons ? align8(P * rs.consensus * 2) : 0;
    o += msa ? align8(P * rs.consensus * S) : 0;
    o += 2 * align8(P * S * rs.seq_len);
    o += align8(P * S * sz) + align8(P * 32);
    o += msa ? align8(P * S * sz) : 0;
    o += 2 * align8(P * gdim * sz); // alignment graph / read
    o += align8(P * nodes) + align8(P * nodes * E * sz) + align8(P * nodes * 2);
    o += align8(P * nodes * E * sz) + align8(P * nodes * 2);
    o += align8(P * nodes * E * sz) + align8(P * nodes * 2);
    o += 2 * align8(P * nodes * E * 2);
    o += 2 * align8(P * nodes * sz) + align8(P * nodes * 2);
    o += cons ? align8(P * nodes * 4) + align8(P * nodes * sz) : 0;
    o += 2 * align8(P * nodes) + align8(P * nodes * sz) + align8(P * nodes * 2);
    o += msa ? align8(P * nodes * E * S * 2) + align8(P * nodes * E * 2) + align8(P * nodes * sz) : 0;
    return o;
}

} // namespace

// sizes of SizeT/ScoreT are the chosen types
int64_t reference_device_bytes_per_poa(const RefSizes& rs, bool msa, int size_bytes)
{
    const int64_t gdim = rs.graph_dim, nodes = rs.nodes;
    const int64_t E = kMaxEdges, A = kMaxAlignments, S = rs.seqs;
    int64_t b = 0;
    b += rs.consensus;                                            // consensus
    b += !msa ? rs.consensus * 2 : 0;                             // coverage
    b += msa ? rs.consensus * S : 0;                              // msa
    b += S * rs.seq_len * 2;                                      // sequences + weights
    b += S * size_bytes;                                          // sequence lengths
    b += 32;                                                      // WindowDetails
    b += msa ? S * size_bytes : 0;                                // sequence_begin_nodes_ids
    b += nodes;                                                   // nodes
    b += nodes * A * size_bytes + nodes * 2;                      // node_alignments (+count)
    b += nodes * E * size_bytes + nodes * 2;                      // incoming edges (+count)
    b += nodes * E * size_bytes + nodes * 2;                      // outgoing edges (+count)
    b += nodes * E * 2 * 2;                                       // in/out edge weights
    b += nodes * size_bytes * 2 + nodes * 2;                      // sorted, node map, local count
    b += !msa ? nodes * 4 + nodes * size_bytes : 0;               // consensus scores / predecessors
    b += nodes + nodes + nodes * size_bytes;                      // marks, check, nodes_to_visit
    b += nodes * 2;                                               // node coverage
    b += msa ? nodes * E * S * 2 + nodes * E * 2 + nodes * size_bytes : 0; // edge coverage, msa pos
    b += gdim * size_bytes * 2;                                   // alignment graph/read
    return b;
}

PoaCapacity plan_capacity(const PoaDeviceFacts& facts, const Dims& dims, const RefSizes& rs, int size_bytes,
                          int score_bytes, bool msa, int64_t max_mem, int tune_slots)
{
    // BatchBlock ctor (allocate_block.hpp:51-91)
    const int64_t per_poa = reference_device_bytes_per_poa(rs, msa, size_bytes);
    if (max_mem < per_poa)
    {
        throw std::runtime_error(std::string("Require at least ") + std::to_string(per_poa) +
                                 " bytes of device memory per CUDAPOA batch to process correctly.");
    }
    const int64_t ref_score_matrix = rs.seq_dim * rs.graph_dim * score_bytes;
    int64_t max_poas               = max_mem / (per_poa + ref_score_matrix);

    // this build's footprint: graph + inputs + outputs per window, and the
    // forward/traceback scratch per slot.  The LDS and banded kernels run
    // a persistent grid of as many workgroups as are resident at once, so
    // they need only that many slots however many windows the batch holds.
    PoaCapacity c;
    c.window_bytes   = window_bytes(dims, size_bytes, msa);
    c.slot_bytes     = slot_bytes(dims, size_bytes, score_bytes);
    int64_t own_cap  = max_mem / (c.window_bytes + c.slot_bytes); // a slot per window
    int64_t resident = 0;
    if (dims.lds_kernel)
    {
        resident = int64_t(facts.blocks_per_cu) * facts.cus;
        if (tune_slots > 0) // diagnostic: a smaller persistent grid
            resident = std::min<int64_t>(resident > 0 ? resident : INT32_MAX, tune_slots);
        if (resident > 0 && own_cap > resident)
            own_cap = std::max(own_cap, (max_mem - resident * c.slot_bytes) / c.window_bytes);
    }
    max_poas = std::min<int64_t>(max_poas, own_cap);
    if (max_poas < 1)
        throw std::runtime_error("Require more device memory per CUDAPOA batch to process correctly.");
    c.max_poas = int32_t(std::min<int64_t>(max_poas, INT32_MAX));
    c.slots    = resident > 0 ? int32_t(std::min<int64_t>(resident, c.max_poas)) : c.max_poas;
    c.resident = resident > 0 ? int32_t(resident) : 0;

    // score budget (allocate_block.hpp:196-201): what the reference's slab
    // leaves for the variable-width score matrices
    c.scorebuf_alloc =
        std::max<int64_t>(0, max_mem - reference_fixed_slab(rs, c.max_poas, size_bytes, msa, dims.want_consensus != 0));
    return c;
}

PoaLayout plan_layout(const Dims& d, int sz, int sbytes, bool msa, int32_t max_poas, int32_t slots)
{
    const int64_t P = max_poas, Z = slots, mn = d.max_nodes, E = kMaxEdges, S = d.max_seqs;
    PoaLayout l;
    int64_t off = 0;
#define GWAMD_F(name, bytes)                                                                                  \
    if (const int64_t b = align8(bytes))                                                                      \
        l.name = off, off += b;
    GWAMD_POA_SLAB_ARRAYS(GWAMD_F)
#undef GWAMD_F
    l.scores      = (off + 255) & ~int64_t(255);
    l.slab_bytes  = l.scores + Z * int64_t(d.score_rows) * d.score_stride * sbytes;
    l.codes_bytes = d.lds_kernel ? Z * d.aux_stride : 0;
    // inputs (allocate_block.hpp:84: max_poas * max_seqs * max_seq bytes)
    l.seqs_bytes = l.wts_bytes = P * S * d.max_seq_len + 64;
    l.len_bytes  = P * S * 4 + 8;
    l.off_bytes  = P * S * 8 + 8;
    // head_off + 4 <= P * 12 + 34 (two round-ups of at most 15), inside P * 12 + 64
    l.order_off = align16(P * int64_t(sizeof(WindowDesc)));
    l.head_off  = align16(l.order_off + P * 4);
    l.win_bytes = P * int64_t(sizeof(WindowDesc) + 4) + 64;
    return l;
}

WindowOrder plan_window_order(const WindowDesc* wd, const int32_t* ln, int n, int cus, int slots,
                              bool persistent_kernel, std::vector<int32_t>& order)
{
    const bool persistent = persistent_kernel && n > slots;
    if (!persistent && (cus <= 0 || n <= cus))
        return kNoOrder;
    std::vector<std::pair<int64_t, int32_t>> cost(static_cast<size_t>(n));
    for (int w = 0; w < n; w++)
    {
        int64_t sum = 0, mx = 0;
        for (int s = 0; s < wd[w].num_seqs; s++)
        {
            const int64_t l = ln[wd[w].first_seq + s];
            mx              = std::max(mx, l);
            if (s > 0)
                sum += l;
        }
        cost[size_t(w)] = {-sum * mx, w}; // heaviest first, ties by window
    }
    std::sort(cost.begin(), cost.end());
    order.resize(size_t(n));
    const int m = persistent ? slots : n; // positions placed statically
    for (int k = 0; k < m; k++)
    {
        if (cus <= 0)
        {
            order[size_t(k)] = cost[size_t(k)].second;
            continue;
        }
        const int t = k / cus, pos = k % cus;
        const int r = std::min(cus, m - t * cus); // workgroups in this round
        const int j = (t % 2 == 0) ? pos : r - 1 - pos;
        order[size_t(t * cus + j)] = cost[size_t(k)].second;
    }
    for (int k = m; k < n; k++)
        order[size_t(k)] = cost[size_t(k)].second;
    return persistent ? kOrderAndHead : kOrder;
}

} // namespace poa
} // namespace gwamd
