// Host side of the MI355X POA path: the reference's cudapoa::Batch API
// (cudapoa/include/.../batch.hpp:133-228) implemented over HIP, plus the plain
// C ABI declared in include/gwamd_cudapoa.h.
//
// Host semantics follow the reference's CudapoaBatch (cudapoa_batch.cuh:56-632)
// and BatchBlock (allocate_block.hpp:47-460): the same score/size type choice,
// the same window capacity (max_poas) and score-buffer budget accounting, the
// same per-entry status codes, and the same error behaviour (throws where the
// reference throws).  Device memory is laid out for the HIP kernels
// (poa_kernels.hip), not the reference's slab.
#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/cudapoa/utils.hpp>
#include <claraparabricks/genomeworks/cudapolish/windows.hpp>

#include "gwamd_cudapoa.h"
#include "gwamd_polish.h"
#include "host_common.hpp"
#include "mapper_reads.hpp"
#include "poa_batch_internal.hpp"
#include "polish_gather.hpp"
#include "poa_common.hpp"
#include "poa_plan.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <sstream>
#include <string>

extern "C" hipError_t gwamd_internal_poa_launch(const gwamd::poa::Buffers* b, const gwamd::poa::Dims* d,
                                       const gwamd::poa::Scores* sc, int score_bits, int size_bits, int banded,
                                       int msa, hipStream_t stream);
extern "C" int gwamd_internal_poa_blocks_per_cu(const gwamd::poa::Dims* d, int score_bits, int size_bits, int banded,
                                                int msa);
extern "C" gwamd::poa::KernelRef gwamd_internal_poa_kernel(const gwamd::poa::Dims* d, int score_bits, int size_bits,
                                                           int banded, int msa);

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapoa
{

using gwamd::host::PinnedBuf;
using gwamd::host::ScopedDevice;

namespace
{

// use32bitScore / use32bitSize (cudapoa_limits.hpp:28-53)
bool use32bit_score(const BatchSize& bs, int16_t gap, int16_t mismatch, int16_t match)
{
    int32_t upper = bs.max_sequence_size * match;
    int32_t lower = bs.max_sequence_size * std::max(gap, mismatch) +
                    (bs.max_matrix_graph_dimension - bs.max_sequence_size) * gap;
    return upper > INT16_MAX || (-lower) > (INT16_MAX + 1);
}

bool use32bit_size(const BatchSize& bs, bool banded)
{
    int32_t m = bs.max_consensus_size;
    m         = std::max(m, banded ? bs.max_matrix_graph_dimension_banded : bs.max_matrix_graph_dimension);
    m         = std::max(m, bs.max_matrix_sequence_dimension);
    return m > INT16_MAX;
}

inline int64_t align8(int64_t v) { return (v + 7) & ~int64_t(7); }

// The BatchSize numbers of the batch's alignment mode, for the plan (poa_plan.hpp)
gwamd::poa::RefSizes ref_sizes(const BatchSize& bs, bool banded)
{
    gwamd::poa::RefSizes rs{};
    rs.seq_len   = bs.max_sequence_size;
    rs.consensus = bs.max_consensus_size;
    rs.seqs      = bs.max_sequences_per_poa;
    rs.nodes     = banded ? bs.max_nodes_per_window_banded : bs.max_nodes_per_window;
    rs.graph_dim = banded ? bs.max_matrix_graph_dimension_banded : bs.max_matrix_graph_dimension;
    rs.seq_dim   = banded ? bs.alignment_band_width + gwamd::poa::kBandPad : bs.max_matrix_sequence_dimension;
    return rs;
}

// The batch constructor's planning steps: score and size widths, capacities,
// and the kernel plan (poa_plan.cpp).  Touches no device (gwamd_internal_poa_plan).
gwamd::poa::Dims plan_batch(const BatchSize& bs, bool banded, int8_t output_mask, int16_t gap, int16_t mismatch,
                            int16_t match, const gwamd::poa::PoaTuning& tune, int& score_bits, int& size_bits)
{
    score_bits = use32bit_score(bs, gap, mismatch, match) ? 32 : 16;
    // batch.cu:45-73: 16-bit score implies 16-bit size
    size_bits  = (score_bits == 32 && use32bit_size(bs, banded)) ? 32 : 16;
    gwamd::poa::Dims dims{};
    // this build's own per-window footprint
    dims.max_nodes     = banded ? bs.max_nodes_per_window_banded : bs.max_nodes_per_window;
    dims.max_seqs      = bs.max_sequences_per_poa;
    dims.max_seq_len   = bs.max_sequence_size;
    dims.max_consensus = bs.max_consensus_size;
    dims.band_width    = bs.alignment_band_width;
    dims.score_stride  = banded ? bs.alignment_band_width + gwamd::poa::kBandPad
                                : int32_t(align8(int64_t(bs.max_sequence_size) + 48));
    dims.score_rows    = dims.max_nodes + 2;
    dims.aln_cap       = dims.max_nodes + bs.max_sequence_size + 4;
    dims.want_consensus = (output_mask & OutputType::consensus) ? 1 : 0;
    // the reference's spoa_accurate build option (CMakeLists.txt:23-30) as a
    // process-wide default; gwamd_poa_set_spoa_accurate switches one batch
    if (const char* sa = std::getenv("GWAMD_SPOA_ACCURATE"))
        dims.spoa_accurate = std::atoi(sa) != 0 ? 1 : 0;
    gwamd::poa::plan_kernels(dims, banded, gwamd::poa::Scores{gap, mismatch, match}, score_bits, size_bits, tune);
    return dims;
}

} // namespace

class PoaBatch : public Batch
{
public:
    PoaBatch(int32_t device_id, hipStream_t stream, size_t max_mem, int8_t output_mask, const BatchSize& bs,
             int16_t gap, int16_t mismatch, int16_t match, bool banded)
        : device_id_(detail::check_non_negative(device_id, "Device ID has to be non-negative"))
        , stream_(stream)
        , output_mask_(output_mask)
        , bs_(bs)
        , gap_(gap)
        , mismatch_(mismatch)
        , match_(match)
        , banded_(banded)
    {
        detail::check_non_negative(bs.max_sequences_per_poa, "Maximum sequences per POA has to be non-negative");
        ScopedDevice dev(device_id_);
        dims_ = plan_batch(bs_, banded_, output_mask_, gap_, mismatch_, match_, tune_, score_bits_, size_bits_);
        const int sz     = size_bits_ / 8;
        const int sbytes = score_bits_ / 8;
        const bool msa   = (output_mask_ & OutputType::msa) != 0;
        // the device's facts, asked once: the plan (poa_plan.cpp) decides every number from them
        gwamd::poa::PoaDeviceFacts facts;
        GWAMD_HIP_CHECK(hipDeviceGetAttribute(&facts.cus, hipDeviceAttributeMultiprocessorCount, device_id_));
        if (dims_.lds_kernel)
            facts.blocks_per_cu = gwamd_internal_poa_blocks_per_cu(&dims_, score_bits_, size_bits_, banded_ ? 1 : 0,
                                                                   msa ? 1 : 0);
        order_cus_ = tune_.order_cus > 0 ? tune_.order_cus : facts.cus; // diagnostic: order for fewer CUs
        cap_ = gwamd::poa::plan_capacity(facts, dims_, ref_sizes(bs_, banded_), sz, sbytes, msa, int64_t(max_mem),
                                         tune_.slots);
        lay_ = gwamd::poa::plan_layout(dims_, sz, sbytes, msa, cap_.max_poas, cap_.slots);
        allocate();
        // pinned host staging for a full batch, as the reference's BatchBlock
        // allocates it up front (allocate_block.hpp:84-118), so filling a
        // batch never re-pins memory (capped; beyond the cap it grows)
        {
            const size_t cap_b = size_t(2) << 30;
            const size_t in_b  = std::min(cap_b, size_t(cap_.max_poas) * size_t(bs_.max_sequences_per_poa) *
                                                    size_t(bs_.max_sequence_size) + 16);
            h_seqs_.reserve(in_b, stream_);
            h_wts_.reserve(in_b, stream_);
            const size_t nseq = std::min(cap_b / 8, size_t(cap_.max_poas) * size_t(bs_.max_sequences_per_poa));
            h_len_.reserve(nseq * 4, stream_);
            h_off_.reserve(nseq * 8, stream_);
            h_win_.reserve(size_t(cap_.max_poas) * sizeof(gwamd::poa::WindowDesc), stream_);
        }
        bid_ = batches_++;
        reset();
    }

    StatusType add_poa_group(std::vector<StatusType>& per_seq_status, const Group& poa_group) override
    {
        int32_t max_len = 0;
        for (const auto& e : poa_group)
            max_len = std::max(max_len, e.length);
        if (!reserve_buf(max_len))
            return StatusType::exceeded_maximum_poas;
        per_seq_status.clear();
        StatusType st = add_poa();
        if (st != StatusType::success)
            return st;
        for (const auto& e : poa_group)
            per_seq_status.push_back(add_seq_to_poa(e.seq, e.weights, e.length));
        return StatusType::success;
    }

    // add_poa_group for sequences that are slices of reads resident on this
    // batch's device (gwamd_poa_add_poa_group_resident): the same bookkeeping
    // without the bytes, which upload() has the device write.  The slices are
    // checked by the caller; the read sets outlive the batch's use of them.
    StatusType add_poa_group_resident(std::vector<StatusType>& per_seq_status,
                                      const gwamd::mapper::DeviceReads* const* sets, const gwamd_read_slice* slices,
                                      int32_t n)
    {
        int32_t max_len = 0;
        for (int32_t i = 0; i < n; i++)
            max_len = std::max(max_len, int32_t(slices[i].end - slices[i].begin));
        if (!reserve_buf(max_len))
            return StatusType::exceeded_maximum_poas;
        per_seq_status.clear();
        StatusType st = add_poa();
        if (st != StatusType::success)
            return st;
        for (int32_t i = 0; i < n; i++)
        {
            const gwamd_read_slice& sl = slices[i];
            const int32_t len          = int32_t(sl.end - sl.begin);
            st                         = seq_status(len);
            per_seq_status.push_back(st);
            if (st != StatusType::success)
                continue;
            const gwamd::mapper::DeviceReads& set = *sets[sl.set];
            const int64_t at                      = set.offsets[sl.read] + int64_t(sl.begin);
            resident_.push_back(ResidentSeq{num_seqs_, sl.set, sl.read, sl.begin, sl.end, sl.flags});
            h_jobs_.reserve(resident_.size() * sizeof(gwamd::polish::SliceJob), stream_);
            h_jobs_.as<gwamd::polish::SliceJob>()[resident_.size() - 1] =
                gwamd::polish::SliceJob{set.bases() + at, set.has_qualities ? set.qualities() + at : nullptr,
                                        int64_t(num_bases_), uint32_t(len), sl.flags & 1u};
            h_jobs_.used_     = resident_.size() * sizeof(gwamd::polish::SliceJob);
            resident_max_len_ = std::max(resident_max_len_, len);
            book_seq(len);
        }
        return StatusType::success;
    }

    int32_t get_total_poas() const override { return poa_count_; }

    void generate_poa() override
    {
        if (poa_count_ == 0)
            return;
        upload();
        launch();
    }

    void upload()
    {
        ScopedDevice dev(device_id_);
        const size_t nb = num_bases_;
        if (resident_.empty())
        {
            GWAMD_HIP_CHECK(
                hipMemcpyAsync(d_seqs_.data(), h_seqs_.as<uint8_t>(), nb + 16, hipMemcpyHostToDevice, stream_));
            GWAMD_HIP_CHECK(
                hipMemcpyAsync(d_wts_.data(), h_wts_.as<int8_t>(), nb + 16, hipMemcpyHostToDevice, stream_));
        }
        else
            upload_mixed_inputs();
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_len_.data(), h_len_.as<int32_t>(), size_t(num_seqs_) * 4,
                                       hipMemcpyHostToDevice, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_off_.data(), h_off_.as<int64_t>(), size_t(num_seqs_) * 8,
                                       hipMemcpyHostToDevice, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_win_.data(), h_win_.as<gwamd::poa::WindowDesc>(),
                                       size_t(poa_count_) * sizeof(gwamd::poa::WindowDesc), hipMemcpyHostToDevice,
                                       stream_));
        // the windows' queue order (plan_window_order, poa_plan.cpp), staged
        // pinned so the copy stays asynchronous (generate_poa does not block)
        bufs_.order = nullptr;
        bufs_.head  = nullptr;
        const auto kind = gwamd::poa::plan_window_order(h_win_.as<gwamd::poa::WindowDesc>(), h_len_.as<int32_t>(),
                                                        poa_count_, order_cus_, cap_.slots, dims_.lds_kernel != 0,
                                                        order_);
        if (kind == gwamd::poa::kNoOrder)
            return;
        const size_t order_b = size_t(poa_count_) * 4;
        h_order_.reserve(order_b, stream_);
        std::memcpy(h_order_.as<int32_t>(), order_.data(), order_b);
        int32_t* d_order = reinterpret_cast<int32_t*>(d_win_.data() + lay_.order_off);
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_order, h_order_.as<int32_t>(), order_b, hipMemcpyHostToDevice, stream_));
        bufs_.order = d_order;
        if (kind == gwamd::poa::kOrderAndHead)
            bufs_.head = reinterpret_cast<int32_t*>(d_win_.data() + lay_.head_off);
    }

    // Test hook (gwamd_internal_poa_download_inputs): the packed bases and
    // weights as upload() left them on the device, num_bases + 16 bytes each
    size_t input_bytes() const { return num_bases_ + 16; }
    void download_inputs(uint8_t* seqs_out, int8_t* wts_out)
    {
        ScopedDevice dev(device_id_);
        GWAMD_HIP_CHECK(hipMemcpyAsync(seqs_out, d_seqs_.data(), input_bytes(), hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(wts_out, d_wts_.data(), input_bytes(), hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    int32_t device_id() const { return device_id_; }

    void launch()
    {
        if (poa_count_ == 0)
            return;
        ScopedDevice dev(device_id_);
        gwamd::poa::Buffers b = bufs_;
        b.num_windows         = poa_count_;
        b.num_slots           = cap_.slots;
        if (b.head) // the dequeue counter starts at 0 for every launch
            GWAMD_HIP_CHECK(hipMemsetAsync(b.head, 0, sizeof(int32_t), stream_));
        gwamd::poa::Scores sc{gap_, mismatch_, match_};
        const bool msa = (output_mask_ & OutputType::msa) != 0;
        if (ev_start_)
            GWAMD_HIP_CHECK(hipEventRecord(ev_start_, stream_));
        GWAMD_HIP_CHECK(gwamd_internal_poa_launch(&b, &dims_, &sc, score_bits_, size_bits_, banded_ ? 1 : 0, msa ? 1 : 0,
                                         stream_));
        if (ev_stop_)
            GWAMD_HIP_CHECK(hipEventRecord(ev_stop_, stream_));
        generated_ = true;
    }

    // instrumentation for the multi-batch driver (poa_batch_internal.hpp)
    void set_launch_events(hipEvent_t start, hipEvent_t stop)
    {
        ev_start_ = start;
        ev_stop_  = stop;
    }

    int64_t last_launch_cells()
    {
        if (poa_count_ == 0 || !generated_)
            return 0;
        std::vector<int64_t> cells(static_cast<size_t>(poa_count_));
        std::vector<int32_t> fn(static_cast<size_t>(poa_count_));
        get_stats(cells.data(), fn.data());
        int64_t s = 0;
        for (int64_t c : cells)
            s += c;
        return s;
    }

    void synchronize()
    {
        ScopedDevice dev(device_id_);
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

    // Copies per-window outputs of the last launch to host staging.
    void fetch(bool consensus, bool msa)
    {
        ScopedDevice dev(device_id_);
        const size_t n = size_t(poa_count_);
        h_status_.resize(n);
        h_msa_status_.resize(n);
        h_len_out_.resize(n);
        h_msa_len_.resize(n);
        if (consensus)
        {
            h_cons_.resize(n * dims_.max_consensus);
            h_cov_.resize(n * dims_.max_consensus);
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_cons_.data(), bufs_.cons, n * dims_.max_consensus, hipMemcpyDeviceToHost,
                                           stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_cov_.data(), bufs_.cov, n * dims_.max_consensus * 2,
                                           hipMemcpyDeviceToHost, stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_len_out_.data(), bufs_.cons_len, n * 4, hipMemcpyDeviceToHost, stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_status_.data(), bufs_.status, n, hipMemcpyDeviceToHost, stream_));
        }
        if (msa)
        {
            h_msa_.resize(n * size_t(dims_.max_seqs) * dims_.max_consensus);
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_msa_.data(), bufs_.msa, h_msa_.size(), hipMemcpyDeviceToHost, stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_msa_len_.data(), bufs_.msa_len, n * 4, hipMemcpyDeviceToHost, stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(h_msa_status_.data(), bufs_.msa_status, n, hipMemcpyDeviceToHost, stream_));
        }
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

    StatusType get_consensus(std::vector<std::string>& consensus, std::vector<std::vector<uint16_t>>& coverage,
                             std::vector<StatusType>& output_status) override
    {
        if (!(output_mask_ & OutputType::consensus))
            return StatusType::output_type_unavailable;
        fetch(true, false);
        for (int32_t w = 0; w < poa_count_; w++)
        {
            const StatusType st = StatusType(h_status_[w]);
            if (!generated_ || st != StatusType::success)
            {
                output_status.push_back(generated_ ? st : StatusType::generic_error);
                consensus.emplace_back();
                coverage.emplace_back();
                continue;
            }
            output_status.push_back(StatusType::success);
            const char* c = reinterpret_cast<const char*>(&h_cons_[size_t(w) * dims_.max_consensus]);
            consensus.emplace_back(c, size_t(h_len_out_[w]));
            const uint16_t* v = &h_cov_[size_t(w) * dims_.max_consensus];
            coverage.emplace_back(v, v + h_len_out_[w]);
        }
        return StatusType::success;
    }

    StatusType get_msa(std::vector<std::vector<std::string>>& msa, std::vector<StatusType>& output_status) override
    {
        if (!(output_mask_ & OutputType::msa))
            return StatusType::output_type_unavailable;
        fetch(false, true);
        for (int32_t w = 0; w < poa_count_; w++)
        {
            msa.emplace_back();
            const StatusType st = StatusType(h_msa_status_[w]);
            if (!generated_ || st != StatusType::success)
            {
                output_status.push_back(generated_ ? st : StatusType::generic_error);
                continue;
            }
            output_status.push_back(StatusType::success);
            const int nseq = h_win_.as<gwamd::poa::WindowDesc>()[w].num_seqs;
            for (int s = 0; s < nseq; s++)
            {
                const char* row = reinterpret_cast<const char*>(
                    &h_msa_[(size_t(w) * dims_.max_seqs + s) * dims_.max_consensus]);
                msa[w].emplace_back(row, size_t(h_msa_len_[w]));
            }
        }
        return StatusType::success;
    }

    void fetch_graphs()
    {
        ScopedDevice dev(device_id_);
        const size_t n  = size_t(poa_count_);
        const size_t mn = size_t(dims_.max_nodes);
        h_g_bases_.resize(n * mn);
        h_g_in_cnt_.resize(n * mn);
        h_g_in_w_.resize(n * mn * gwamd::poa::kMaxEdges);
        h_g_in_e_raw_.resize(n * mn * gwamd::poa::kMaxEdges * (size_bits_ / 8));
        h_final_nodes_.resize(n);
        h_status_.resize(n);
        h_msa_status_.resize(n);
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_g_bases_.data(), bufs_.base, n * mn, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_g_in_cnt_.data(), bufs_.in_cnt, n * mn * 2, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_g_in_w_.data(), bufs_.in_w, h_g_in_w_.size() * 2, hipMemcpyDeviceToHost,
                                       stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_g_in_e_raw_.data(), bufs_.in_e, h_g_in_e_raw_.size(), hipMemcpyDeviceToHost,
                                       stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_final_nodes_.data(), bufs_.final_nodes, n * 4, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_status_.data(), bufs_.status, n, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_msa_status_.data(), bufs_.msa_status, n, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
        h_g_in_e_.resize(h_g_in_w_.size());
        if (size_bits_ == 16)
        {
            const int16_t* s = reinterpret_cast<const int16_t*>(h_g_in_e_raw_.data());
            for (size_t i = 0; i < h_g_in_e_.size(); i++)
                h_g_in_e_[i] = s[i];
        }
        else
            std::memcpy(h_g_in_e_.data(), h_g_in_e_raw_.data(), h_g_in_e_raw_.size());
    }

    // Graph status: the consensus status when consensus is produced, else MSA's.
    StatusType graph_status(int32_t w) const
    {
        if (!generated_)
            return StatusType::generic_error;
        return StatusType((output_mask_ & OutputType::consensus) ? h_status_[w] : h_msa_status_[w]);
    }

    void get_graphs(std::vector<DirectedGraph>& graphs, std::vector<StatusType>& output_status) override
    {
        fetch_graphs();
        graphs.resize(poa_count_);
        const size_t mn = size_t(dims_.max_nodes);
        for (int32_t w = 0; w < poa_count_; w++)
        {
            StatusType st = graph_status(w);
            output_status.push_back(st);
            if (st != StatusType::success)
                continue;
            DirectedGraph& g = graphs[w];
            for (int32_t v = 0; v < h_final_nodes_[w]; v++)
            {
                g.set_node_label(v, std::string(1, char(h_g_bases_[w * mn + v])));
                const int ne = h_g_in_cnt_[w * mn + v];
                for (int e = 0; e < ne; e++)
                {
                    size_t idx = (w * mn + v) * gwamd::poa::kMaxEdges + e;
                    g.add_edge(h_g_in_e_[idx], v, h_g_in_w_[idx]);
                }
            }
        }
    }

    int32_t batch_id() const override { return bid_; }

    void reset() override
    {
        poa_count_          = 0;
        num_bases_          = 0;
        num_seqs_           = 0;
        next_scores_offset_ = 0;
        avail_scorebuf_     = cap_.scorebuf_alloc;
        generated_          = false;
        resident_.clear();
        host_runs_.clear();
        resident_max_len_ = 0;
        h_jobs_.used_     = 0;
    }

    // --- C ABI support ------------------------------------------------------
    int32_t score_bits() const { return score_bits_; }
    int32_t size_bits() const { return size_bits_; }
    const gwamd::poa::Dims& dims() const { return dims_; }
    const std::vector<uint8_t>& host_cons() const { return h_cons_; }
    const std::vector<uint16_t>& host_cov() const { return h_cov_; }
    const std::vector<int32_t>& host_cons_len() const { return h_len_out_; }
    const std::vector<uint8_t>& host_status() const { return h_status_; }
    const std::vector<uint8_t>& host_msa() const { return h_msa_; }
    const std::vector<int32_t>& host_msa_len() const { return h_msa_len_; }
    const std::vector<uint8_t>& host_msa_status() const { return h_msa_status_; }
    const std::vector<uint8_t>& host_g_bases() const { return h_g_bases_; }
    const std::vector<uint16_t>& host_g_in_cnt() const { return h_g_in_cnt_; }
    const std::vector<int32_t>& host_g_in_e() const { return h_g_in_e_; }
    const std::vector<uint16_t>& host_g_in_w() const { return h_g_in_w_; }
    const std::vector<int32_t>& host_final_nodes() const { return h_final_nodes_; }
    int32_t window_num_seqs(int32_t w) const { return h_win_.as<const gwamd::poa::WindowDesc>()[w].num_seqs; }
    int8_t output_mask() const { return output_mask_; }
    int64_t device_bytes() const { return lay_.device_bytes(); }
    int32_t kernel_kind() const
    {
        return dims_.lds_kernel == 3 ? (dims_.band_ad ? 4 : 3) : (dims_.lds_kernel ? 2 : 1);
    }
    int32_t max_poas() const { return cap_.max_poas; }
    int32_t max_sequence_size() const { return bs_.max_sequence_size; }
    int32_t slots() const { return cap_.slots; }
    int32_t resident_slots() const { return cap_.resident; }
    void set_spoa_accurate(bool on) { dims_.spoa_accurate = on ? 1 : 0; }
    bool spoa_accurate() const { return dims_.spoa_accurate != 0; }

    void get_phases(int64_t* out)
    {
        ScopedDevice dev(device_id_);
        if (poa_count_ == 0)
            return;
        GWAMD_HIP_CHECK(hipMemcpyAsync(out, bufs_.phase, size_t(poa_count_) * 8 * gwamd::poa::kPhases,
                                       hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

    // per-window row-order counters of the LDS kernel (poa_order.hpp; zeros from any other kernel)
    void get_order_stats(int32_t* out)
    {
        ScopedDevice dev(device_id_);
        if (poa_count_ == 0)
            return;
        GWAMD_HIP_CHECK(hipMemcpyAsync(out, bufs_.order_stats, size_t(poa_count_) * 4 * gwamd::poa::kOrderStats,
                                       hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

    void get_stats(int64_t* cells, int32_t* final_nodes)
    {
        ScopedDevice dev(device_id_);
        if (poa_count_ == 0)
            return;
        GWAMD_HIP_CHECK(hipMemcpyAsync(cells, bufs_.cells, size_t(poa_count_) * 8, hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(final_nodes, bufs_.final_nodes, size_t(poa_count_) * 4, hipMemcpyDeviceToHost,
                                       stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

private:
    // Allocates what the layout (plan_layout) lists and binds the kernels' pointers into it.
    void allocate()
    {
        const gwamd::host::Budget none;
        d_slab_.alloc(size_t(lay_.slab_bytes), none);
        d_codes_.alloc(size_t(lay_.codes_bytes), none);
        d_seqs_.alloc(size_t(lay_.seqs_bytes), none);
        d_wts_.alloc(size_t(lay_.wts_bytes), none);
        d_len_.alloc(size_t(lay_.len_bytes), none);
        d_off_.alloc(size_t(lay_.off_bytes), none);
        d_win_.alloc(size_t(lay_.win_bytes), none);
#define GWAMD_F(name, bytes)                                                                                  \
    if (lay_.name >= 0)                                                                                       \
        bufs_.name = reinterpret_cast<decltype(bufs_.name)>(d_slab_.data() + lay_.name);
        GWAMD_POA_SLAB_ARRAYS(GWAMD_F)
#undef GWAMD_F
        bufs_.scores  = d_slab_.data() + lay_.scores;
        bufs_.codes   = d_codes_.data();
        bufs_.seqs    = d_seqs_.data();
        bufs_.wts     = reinterpret_cast<const int8_t*>(d_wts_.data());
        bufs_.seq_len = reinterpret_cast<const int32_t*>(d_len_.data());
        bufs_.seq_off = reinterpret_cast<const int64_t*>(d_off_.data());
        bufs_.windows = reinterpret_cast<const gwamd::poa::WindowDesc*>(d_win_.data());
        // status defaults so that reading before generate is defined
        const size_t P = size_t(cap_.max_poas);
        GWAMD_HIP_CHECK(hipMemsetAsync(bufs_.status, int(StatusType::generic_error), P, stream_));
        GWAMD_HIP_CHECK(hipMemsetAsync(bufs_.msa_status, int(StatusType::generic_error), P, stream_));
        GWAMD_HIP_CHECK(hipMemsetAsync(bufs_.order_stats, 0, P * 4 * gwamd::poa::kOrderStats, stream_));
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }

    // cudapoa_batch.cuh:542-564
    bool reserve_buf(int32_t max_seq_length)
    {
        const int64_t gdim  = banded_ ? bs_.max_matrix_graph_dimension_banded : bs_.max_matrix_graph_dimension;
        const int64_t width = banded_ ? bs_.alignment_band_width + gwamd::poa::kBandPad
                                      : detail::align_up(max_seq_length + 1 + 4, 4);
        const int64_t need  = width * gdim * (score_bits_ / 8);
        if (need > avail_scorebuf_)
        {
            if (poa_count_ == 0)
            {
                std::cout << "Memory available " << std::fixed << std::setprecision(2)
                          << double(avail_scorebuf_) / 1024. / 1024. / 1024.;
                std::cout << "GB, Memory required " << double(need) / 1024. / 1024. / 1024.;
                std::cout << "GB (sequence length " << max_seq_length << ", graph length " << gdim << ")" << std::endl;
            }
            return false;
        }
        avail_scorebuf_ -= need;
        return true;
    }

    // cudapoa_batch.cuh:471-487
    StatusType add_poa()
    {
        if (poa_count_ == cap_.max_poas)
            return StatusType::exceeded_maximum_poas;
        h_win_.reserve(size_t(poa_count_ + 1) * sizeof(gwamd::poa::WindowDesc), stream_);
        gwamd::poa::WindowDesc& wd = h_win_.as<gwamd::poa::WindowDesc>()[poa_count_];
        wd.first_seq               = num_seqs_;
        wd.num_seqs                = 0;
        h_win_.used_               = size_t(poa_count_ + 1) * sizeof(gwamd::poa::WindowDesc);
        poa_count_++;
        generated_ = false;
        return StatusType::success;
    }

    // The checks of add_seq_to_poa (cudapoa_batch.cuh:490-503) on the window being filled
    StatusType seq_status(int32_t seq_len) const
    {
        if (seq_len > bs_.max_sequence_size)
            return StatusType::exceeded_maximum_sequence_size;
        if (h_win_.as<gwamd::poa::WindowDesc>()[poa_count_ - 1].num_seqs >= bs_.max_sequences_per_poa)
            return StatusType::exceeded_maximum_sequences_per_poa;
        return StatusType::success;
    }

    // ... and its counters (cudapoa_batch.cuh:505-539): the sequence takes
    // [num_bases_, num_bases_ + seq_len) of the packed arrays, wherever its bytes come from
    void book_seq(int32_t seq_len)
    {
        h_win_.as<gwamd::poa::WindowDesc>()[poa_count_ - 1].num_seqs++;
        h_len_.reserve(size_t(num_seqs_ + 1) * 4, stream_);
        h_off_.reserve(size_t(num_seqs_ + 1) * 8, stream_);
        h_len_.as<int32_t>()[num_seqs_] = seq_len;
        h_off_.as<int64_t>()[num_seqs_] = int64_t(num_bases_);
        num_bases_ += size_t(seq_len);
        num_seqs_++;
        h_len_.used_ = size_t(num_seqs_) * 4;
        h_off_.used_ = size_t(num_seqs_) * 8;
    }

    // cudapoa_batch.cuh:490-539
    StatusType add_seq_to_poa(const char* seq, const int8_t* weights, int32_t seq_len)
    {
        const StatusType st = seq_status(seq_len);
        if (st != StatusType::success)
            return st;
        if (weights != nullptr)
            for (int32_t i = 0; i < seq_len; i++)
                detail::check_non_negative(weights[i], "Base weights need to be non-negative");
        const size_t need = num_bases_ + size_t(seq_len) + 16;
        h_seqs_.reserve(need, stream_);
        h_wts_.reserve(need, stream_);
        if (seq_len > 0)
            std::memcpy(h_seqs_.as<uint8_t>() + num_bases_, seq, size_t(seq_len));
        if (weights == nullptr)
            std::memset(h_wts_.as<int8_t>() + num_bases_, 1, size_t(seq_len));
        else if (seq_len > 0)
            std::memcpy(h_wts_.as<int8_t>() + num_bases_, weights, size_t(seq_len));
        std::memset(h_seqs_.as<uint8_t>() + num_bases_ + seq_len, 0, 16);
        std::memset(h_wts_.as<int8_t>() + num_bases_ + seq_len, 0, 16);
        // the bytes the host holds, as runs: what upload() copies when the batch has resident sequences too
        if (!host_runs_.empty() && host_runs_.back().second == num_bases_)
            host_runs_.back().second += size_t(seq_len);
        else if (seq_len > 0)
            host_runs_.emplace_back(num_bases_, num_bases_ + size_t(seq_len));
        book_seq(seq_len);
        h_seqs_.used_ = h_wts_.used_ = num_bases_ + 16;
        return StatusType::success;
    }

    // upload() of the packed bases and weights of a batch with resident
    // sequences.  Every byte of [0, num_bases_) has one writer: the copy of
    // the host run it lies in, or the kernel for the resident sequence it
    // belongs to, which writes no byte outside its sequence
    // (polish_gather.hip); the 16 zero bytes after the last base are set here.
    // All on the batch's stream, so the POA kernels see them done.
    void upload_mixed_inputs()
    {
        const size_t nb = num_bases_;
        for (const auto& run : host_runs_)
        {
            const size_t bytes = run.second - run.first;
            GWAMD_HIP_CHECK(hipMemcpyAsync(d_seqs_.data() + run.first, h_seqs_.as<uint8_t>() + run.first, bytes,
                                           hipMemcpyHostToDevice, stream_));
            GWAMD_HIP_CHECK(hipMemcpyAsync(d_wts_.data() + run.first, h_wts_.as<int8_t>() + run.first, bytes,
                                           hipMemcpyHostToDevice, stream_));
        }
        GWAMD_HIP_CHECK(hipMemsetAsync(d_seqs_.data() + nb, 0, 16, stream_));
        GWAMD_HIP_CHECK(hipMemsetAsync(d_wts_.data() + nb, 0, 16, stream_));
        const size_t jobs_b = resident_.size() * sizeof(gwamd::polish::SliceJob);
        if (d_jobs_.size() < jobs_b)
        {
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream_)); // an earlier launch may still read the old array
            d_jobs_.alloc(std::max(jobs_b, 2 * d_jobs_.size()), gwamd::host::Budget());
        }
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_jobs_.data(), h_jobs_.as<uint8_t>(), jobs_b, hipMemcpyHostToDevice, stream_));
        gwamd::polish::gather_poa_slices(d_seqs_.data(), reinterpret_cast<int8_t*>(d_wts_.data()),
                                         reinterpret_cast<const gwamd::polish::SliceJob*>(d_jobs_.data()),
                                         int64_t(resident_.size()), resident_max_len_, stream_);
    }

    // A sequence added as a slice of a resident read (add_poa_group_resident)
    struct ResidentSeq
    {
        int32_t sequence; // its index in the batch
        int32_t set;
        uint32_t read, begin, end, flags;
    };

    int32_t device_id_;
    hipStream_t stream_;
    int8_t output_mask_;
    BatchSize bs_;
    int16_t gap_, mismatch_, match_;
    bool banded_;
    int32_t score_bits_ = 16, size_bits_ = 16;
    gwamd::poa::PoaCapacity cap_; // windows, slots, resident grid, score budget (plan_capacity)
    gwamd::poa::PoaLayout lay_;   // where every device array lies (plan_layout)
    int32_t order_cus_ = 0;       // CUs the window order is planned for
    int64_t avail_scorebuf_ = 0, next_scores_offset_ = 0;
    int32_t poa_count_  = 0;
    int32_t num_seqs_   = 0;
    size_t num_bases_   = 0;
    bool generated_     = false;
    int32_t bid_        = 0;
    hipEvent_t ev_start_ = nullptr, ev_stop_ = nullptr; // set_launch_events (multi-batch driver)
    const gwamd::poa::PoaTuning tune_ = gwamd::poa::read_poa_tuning(); // read once, here
    gwamd::poa::Dims dims_{};
    std::vector<int32_t> order_; // queue position -> window (plan_window_order)
    PinnedBuf h_order_;          // ... staged for the copy
    gwamd::poa::Buffers bufs_{};
    gwamd::host::DevBuf<uint8_t> d_seqs_, d_wts_, d_len_, d_off_, d_win_, d_slab_, d_codes_;
    PinnedBuf h_seqs_, h_wts_, h_len_, h_off_, h_win_;
    std::vector<ResidentSeq> resident_;                   // in sequence order
    std::vector<std::pair<size_t, size_t>> host_runs_;    // [first, last) of the packed bytes the host holds
    int32_t resident_max_len_ = 0;
    PinnedBuf h_jobs_;                                    // one SliceJob per resident sequence, staged for the copy
    gwamd::host::DevBuf<uint8_t> d_jobs_;
    std::vector<uint8_t> h_cons_, h_status_, h_msa_, h_msa_status_, h_g_bases_, h_g_in_e_raw_;
    std::vector<uint16_t> h_cov_, h_g_in_cnt_, h_g_in_w_;
    std::vector<int32_t> h_len_out_, h_msa_len_, h_g_in_e_, h_final_nodes_;
    static int32_t batches_; // batch id counter (cudapoa_batch.cuh:631-635)
};

int32_t PoaBatch::batches_ = 0;

StatusType Init()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return StatusType::generic_error;
    return StatusType::success;
}

// BatchBlock::estimate_max_poas (allocate_block.hpp:364-401)
int64_t estimate_max_poas(const BatchSize& batch_size, bool banded_alignment, bool msa_flag,
                          size_t free_device_memory, float memory_usage_quota, int32_t mismatch_score,
                          int32_t gap_score, int32_t match_score)
{
    const size_t mem_per_batch = size_t(memory_usage_quota * double(free_device_memory));
    int64_t sizeof_score       = 2;
    int64_t per_poa            = 0;
    const gwamd::poa::RefSizes rs = ref_sizes(batch_size, banded_alignment);
    if (use32bit_score(batch_size, int16_t(gap_score), int16_t(mismatch_score), int16_t(match_score)))
    {
        sizeof_score = 4;
        per_poa      = gwamd::poa::reference_device_bytes_per_poa(rs, msa_flag,
                                                             use32bit_size(batch_size, banded_alignment) ? 4 : 2);
    }
    else
        per_poa = gwamd::poa::reference_device_bytes_per_poa(rs, msa_flag, 2);
    return int64_t(mem_per_batch) / (per_poa + rs.seq_dim * rs.graph_dim * sizeof_score);
}

// get_multi_batch_sizes (utils.cu:24-138): groups are binned by their batch
// capacity (bins 1, 2, 4, ... 2^19 unless given), each non-empty bin becomes
// one BatchSize sized by its largest group (max read length x reads), and the
// following bins are merged into it while their group count fits its capacity.
void get_multi_batch_sizes_for_memory(std::vector<BatchSize>& list_of_batch_sizes,
                                      std::vector<std::vector<int32_t>>& list_of_groups_per_batch,
                                      const std::vector<Group>& poa_groups, size_t free_device_memory,
                                      bool banded_alignment, bool msa_flag, int32_t band_width,
                                      std::vector<int32_t>* bins_capacity, float gpu_memory_usage_quota,
                                      int32_t mismatch_score, int32_t gap_score, int32_t match_score)
{
    const int32_t num_groups = int32_t(poa_groups.size());
    std::vector<int64_t> max_poas(num_groups);
    std::vector<int32_t> max_lengths(num_groups);
    for (int32_t i = 0; i < num_groups; i++)
    {
        int32_t max_read_length = 0;
        for (const auto& e : poa_groups[i])
            max_read_length = std::max(max_read_length, e.length);
        max_poas[i] = estimate_max_poas(BatchSize(max_read_length, int32_t(poa_groups[i].size()), band_width),
                                        banded_alignment, msa_flag, free_device_memory, gpu_memory_usage_quota,
                                        mismatch_score, gap_score, match_score);
        max_lengths[i] = max_read_length;
    }
    std::vector<int32_t> default_bins(20, 1);
    for (size_t j = 1; j < default_bins.size(); j++)
        default_bins[j] = default_bins[j - 1] * 2;
    const std::vector<int32_t>& bins = bins_capacity ? *bins_capacity : default_bins;
    const int32_t num_bins           = int32_t(bins.size());
    std::vector<int32_t> freq(num_bins, 0), bin_len(num_bins, 0), bin_reads(num_bins, 0);
    std::vector<std::vector<int32_t>> bin_groups(num_bins);
    for (int32_t i = 0; i < num_groups; i++)
    {
        const int32_t current = max_lengths[i] * int32_t(poa_groups[i].size());
        for (int32_t j = 0; j < num_bins; j++)
        {
            if (max_poas[i] <= bins[j] || j == num_bins - 1)
            {
                freq[j]++;
                bin_groups[j].push_back(i);
                if (bin_len[j] * bin_reads[j] < current)
                {
                    bin_len[j]   = max_lengths[i];
                    bin_reads[j] = int32_t(poa_groups[i].size());
                }
                break;
            }
        }
    }
    for (int32_t j = 0; j < num_bins; j++)
    {
        if (freq[j] == 0)
            continue;
        list_of_batch_sizes.emplace_back(bin_len[j], bin_reads[j], band_width);
        list_of_groups_per_batch.push_back(bin_groups[j]);
        for (int32_t k = j + 1; k < num_bins; k++)
        {
            if (freq[k] == 0)
                continue;
            if (bins[j] >= freq[k])
            {
                auto& cur = list_of_groups_per_batch.back();
                cur.insert(cur.end(), bin_groups[k].begin(), bin_groups[k].end());
                freq[k] = 0;
            }
            else
                break;
        }
    }
}

void get_multi_batch_sizes(std::vector<BatchSize>& list_of_batch_sizes,
                           std::vector<std::vector<int32_t>>& list_of_groups_per_batch,
                           const std::vector<Group>& poa_groups, bool banded_alignment, bool msa_flag,
                           int32_t band_width, std::vector<int32_t>* bins_capacity, float gpu_memory_usage_quota,
                           int32_t mismatch_score, int32_t gap_score, int32_t match_score)
{
    size_t free_mem = 0, total = 0;
    if (hipMemGetInfo(&free_mem, &total) != hipSuccess)
        throw std::runtime_error("get_multi_batch_sizes: hipMemGetInfo failed");
    get_multi_batch_sizes_for_memory(list_of_batch_sizes, list_of_groups_per_batch, poa_groups, free_mem,
                                     banded_alignment, msa_flag, band_width, bins_capacity, gpu_memory_usage_quota,
                                     mismatch_score, gap_score, match_score);
}

std::unique_ptr<Batch> create_batch(int32_t device_id, hipStream_t stream, size_t max_mem, int8_t output_mask,
                                    const BatchSize& batch_size, int16_t gap_score, int16_t mismatch_score,
                                    int16_t match_score, bool cuda_banded_alignment)
{
    detail::check_non_negative(batch_size.max_sequences_per_poa, "Maximum sequences per POA has to be non-negative");
    return std::unique_ptr<Batch>(new PoaBatch(device_id, stream, max_mem, output_mask, batch_size, gap_score,
                                               mismatch_score, match_score, cuda_banded_alignment));
}

namespace detail
{
void set_launch_events(Batch* batch, hipEvent_t start, hipEvent_t stop)
{
    static_cast<PoaBatch*>(batch)->set_launch_events(start, stop);
}

int64_t last_launch_cells(Batch* batch) { return static_cast<PoaBatch*>(batch)->last_launch_cells(); }

int32_t max_sequence_size(const Batch* batch) { return static_cast<const PoaBatch*>(batch)->max_sequence_size(); }
} // namespace detail

} // namespace cudapoa
} // namespace genomeworks
} // namespace claraparabricks

// ---------------------------------------------------------------------------
// Groups as slices of resident reads: the one check of the slices, on the
// handles' host copies of the offsets and before any device call, behind the
// C entry (gwamd_poa_add_poa_group_resident) and the C++ free function
// (cudapolish::add_poa_group_resident, windows.hpp)
// ---------------------------------------------------------------------------
namespace
{

void check_resident_slices(const claraparabricks::genomeworks::cudapoa::PoaBatch& batch,
                           const std::vector<const gwamd::mapper::DeviceReads*>& sets, const gwamd_read_slice* slices,
                           int64_t n)
{
    if (n < 0)
        throw std::invalid_argument("the number of slices must not be negative");
    if (n > 0 && !slices)
        throw std::invalid_argument("slices is NULL");
    for (size_t s = 0; s < sets.size(); s++)
        if (!sets[s])
            throw std::invalid_argument("set " + std::to_string(s) + " is NULL");
    for (int64_t i = 0; i < n; i++)
    {
        const gwamd_read_slice& sl = slices[i];
        const std::string which    = "slice " + std::to_string(i);
        if (sl.set < 0 || size_t(sl.set) >= sets.size())
            throw std::invalid_argument(which + ": set index outside the sets");
        const gwamd::mapper::DeviceReads& set = *sets[size_t(sl.set)];
        if (int64_t(sl.read) >= set.num_reads())
            throw std::invalid_argument(which + ": read id beyond the reads");
        if (sl.begin > sl.end || int64_t(sl.end) > set.read_length(sl.read))
            throw std::invalid_argument(which + ": positions are not begin <= end <= read length");
        if (set.device_id != batch.device_id())
            throw std::invalid_argument(which + ": its reads are on device " + std::to_string(set.device_id) +
                                        ", the batch is on device " + std::to_string(batch.device_id()));
    }
}

claraparabricks::genomeworks::cudapoa::StatusType
add_resident_checked(claraparabricks::genomeworks::cudapoa::PoaBatch& batch,
                     std::vector<claraparabricks::genomeworks::cudapoa::StatusType>& per_seq_status,
                     const std::vector<const gwamd::mapper::DeviceReads*>& sets, const gwamd_read_slice* slices,
                     int32_t n)
{
    check_resident_slices(batch, sets, slices, n);
    return batch.add_poa_group_resident(per_seq_status, sets.data(), slices, n);
}

// Many groups in one call (gwamd_poa_add_poa_groups_resident): every slice is
// checked before the first group is added; then group after group as the single
// call adds it, up to the first that the batch has no room for.  Returns the
// number of groups consumed.  group_status and per_seq_status (one entry per
// slice) are written for those groups only.
int32_t add_resident_groups_checked(claraparabricks::genomeworks::cudapoa::PoaBatch& batch,
                                    const std::vector<const gwamd::mapper::DeviceReads*>& sets,
                                    const gwamd_read_slice* slices, const int32_t* group_counts, int32_t num_groups,
                                    int32_t* group_status, int32_t* per_seq_status)
{
    using claraparabricks::genomeworks::cudapoa::StatusType;
    if (num_groups < 0)
        throw std::invalid_argument("the number of groups must not be negative");
    if (num_groups > 0 && (!group_counts || !group_status))
        throw std::invalid_argument("group_counts or group_status is NULL");
    int64_t total = 0;
    for (int32_t g = 0; g < num_groups; g++)
    {
        if (group_counts[g] < 0)
            throw std::invalid_argument("group " + std::to_string(g) + ": negative number of slices");
        total += group_counts[g];
    }
    if (total > 0 && !per_seq_status)
        throw std::invalid_argument("per_seq_status is NULL");
    check_resident_slices(batch, sets, slices, total);
    std::vector<StatusType> st;
    int64_t at = 0;
    for (int32_t g = 0; g < num_groups; g++)
    {
        const int32_t n     = group_counts[g];
        const StatusType rc = batch.add_poa_group_resident(st, sets.data(), slices + at, n);
        if (rc == StatusType::exceeded_maximum_poas)
            return g;
        group_status[g] = int32_t(rc);
        for (size_t i = 0; i < size_t(n); i++)
            per_seq_status[size_t(at) + i] = int32_t(i < st.size() ? st[i] : rc);
        at += n;
    }
    return num_groups;
}

} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapolish
{

static_assert(sizeof(ReadSlice) == sizeof(gwamd_read_slice), "ReadSlice is gwamd_read_slice");

cudapoa::StatusType add_poa_group_resident(cudapoa::Batch& batch, std::vector<cudapoa::StatusType>& per_seq_status,
                                           const std::vector<const cudamapper::DeviceReads*>& sets,
                                           const std::vector<ReadSlice>& slices)
{
    auto* own = dynamic_cast<cudapoa::PoaBatch*>(&batch);
    if (!own)
        throw std::invalid_argument("add_poa_group_resident: the batch does not come from cudapoa::create_batch");
    std::vector<const gwamd::mapper::DeviceReads*> reads(sets.size());
    for (size_t s = 0; s < sets.size(); s++)
        reads[s] = sets[s] ? sets[s]->impl().reads.get() : nullptr;
    return add_resident_checked(*own, per_seq_status, reads,
                                reinterpret_cast<const gwamd_read_slice*>(slices.data()), int32_t(slices.size()));
}

int32_t add_poa_groups_resident(cudapoa::Batch& batch, std::vector<cudapoa::StatusType>& group_status,
                                std::vector<cudapoa::StatusType>& per_seq_status,
                                const std::vector<const cudamapper::DeviceReads*>& sets,
                                const std::vector<ReadSlice>& slices, const std::vector<int32_t>& group_counts)
{
    auto* own = dynamic_cast<cudapoa::PoaBatch*>(&batch);
    if (!own)
        throw std::invalid_argument("add_poa_groups_resident: the batch does not come from cudapoa::create_batch");
    if (group_counts.size() > size_t(INT32_MAX))
        throw std::invalid_argument("add_poa_groups_resident: too many groups for one call");
    std::vector<const gwamd::mapper::DeviceReads*> reads(sets.size());
    for (size_t s = 0; s < sets.size(); s++)
        reads[s] = sets[s] ? sets[s]->impl().reads.get() : nullptr;
    int64_t total = 0;
    for (int32_t c : group_counts)
        total += std::max(c, 0);
    if (total > int64_t(slices.size()))
        throw std::invalid_argument("add_poa_groups_resident: the groups count more slices than there are");
    std::vector<int32_t> groups(group_counts.size() + 1), seqs(size_t(total) + 1);
    const int32_t added =
        add_resident_groups_checked(*own, reads, reinterpret_cast<const gwamd_read_slice*>(slices.data()),
                                    group_counts.data(), int32_t(group_counts.size()), groups.data(), seqs.data());
    group_status.clear();
    per_seq_status.clear();
    for (int32_t g = 0, at = 0; g < added; g++)
    {
        group_status.push_back(cudapoa::StatusType(groups[size_t(g)]));
        for (int32_t i = 0; i < group_counts[size_t(g)]; i++, at++)
            per_seq_status.push_back(cudapoa::StatusType(seqs[size_t(at)]));
    }
    return added;
}

} // namespace cudapolish
} // namespace genomeworks
} // namespace claraparabricks

// ===========================================================================
// C ABI (include/gwamd_cudapoa.h)
// ===========================================================================
namespace cp = claraparabricks::genomeworks::cudapoa;

namespace
{

template <typename F>
int32_t guarded(F&& f)
{
    try
    {
        gwamd::host::last_error().clear();
        return f();
    }
    catch (const std::invalid_argument& e)
    {
        gwamd::host::last_error() = e.what();
        return GWAMD_E_INVALID_ARGUMENT;
    }
    catch (const std::runtime_error& e)
    {
        gwamd::host::last_error() = e.what();
        return std::string(e.what()).rfind("HIP error", 0) == 0 ? GWAMD_E_HIP : GWAMD_E_RUNTIME;
    }
    catch (const std::exception& e)
    {
        gwamd::host::last_error() = e.what();
        return GWAMD_E_RUNTIME;
    }
}

void to_c(const cp::BatchSize& b, gwamd_poa_batch_size* o)
{
    o->max_sequence_size                 = b.max_sequence_size;
    o->max_consensus_size                = b.max_consensus_size;
    o->max_nodes_per_window              = b.max_nodes_per_window;
    o->max_nodes_per_window_banded       = b.max_nodes_per_window_banded;
    o->max_matrix_graph_dimension        = b.max_matrix_graph_dimension;
    o->max_matrix_graph_dimension_banded = b.max_matrix_graph_dimension_banded;
    o->max_matrix_sequence_dimension     = b.max_matrix_sequence_dimension;
    o->alignment_band_width              = b.alignment_band_width;
    o->max_sequences_per_poa             = b.max_sequences_per_poa;
}

cp::BatchSize from_c(const gwamd_poa_batch_size* i)
{
    cp::BatchSize b;
    b.max_sequence_size                 = i->max_sequence_size;
    b.max_consensus_size                = i->max_consensus_size;
    b.max_nodes_per_window              = i->max_nodes_per_window;
    b.max_nodes_per_window_banded       = i->max_nodes_per_window_banded;
    b.max_matrix_graph_dimension        = i->max_matrix_graph_dimension;
    b.max_matrix_graph_dimension_banded = i->max_matrix_graph_dimension_banded;
    b.max_matrix_sequence_dimension     = i->max_matrix_sequence_dimension;
    b.alignment_band_width              = i->alignment_band_width;
    b.max_sequences_per_poa             = i->max_sequences_per_poa;
    return b;
}
} // namespace

struct gwamd_poa_batch
{
    std::unique_ptr<cp::PoaBatch> impl;
};

extern "C" {

const char* gwamd_last_error(void) { return gwamd::host::last_error().c_str(); }

int32_t gwamd_poa_batch_size_init(gwamd_poa_batch_size* out, int32_t max_seq_sz, int32_t max_seq_per_poa,
                                  int32_t band_width)
{
    return guarded([&] {
        to_c(cp::BatchSize(max_seq_sz, max_seq_per_poa, band_width), out);
        return 0;
    });
}

int32_t gwamd_poa_batch_size_init_full(gwamd_poa_batch_size* out, int32_t max_seq_sz, int32_t max_consensus_sz,
                                       int32_t max_nodes_per_w, int32_t max_nodes_per_w_banded, int32_t band_width,
                                       int32_t max_seq_per_poa)
{
    return guarded([&] {
        to_c(cp::BatchSize(max_seq_sz, max_consensus_sz, max_nodes_per_w, max_nodes_per_w_banded, band_width,
                           max_seq_per_poa),
             out);
        return 0;
    });
}

int32_t gwamd_poa_create_batch(gwamd_poa_batch** out, int32_t device_id, void* stream, size_t max_mem,
                               int8_t output_mask, const gwamd_poa_batch_size* batch_size, int16_t gap_score,
                               int16_t mismatch_score, int16_t match_score, int32_t cuda_banded_alignment)
{
    *out = nullptr;
    return guarded([&] {
        auto* h = new gwamd_poa_batch;
        try
        {
            h->impl.reset(new cp::PoaBatch(device_id, static_cast<hipStream_t>(stream), max_mem, output_mask,
                                           from_c(batch_size), gap_score, mismatch_score, match_score,
                                           cuda_banded_alignment != 0));
        }
        catch (...)
        {
            delete h;
            throw;
        }
        *out = h;
        return 0;
    });
}

void gwamd_poa_destroy_batch(gwamd_poa_batch* batch) { delete batch; }

int32_t gwamd_poa_add_poa_group(gwamd_poa_batch* batch, const char* const* seqs, const int8_t* const* weights,
                                const int32_t* lengths, int32_t n, int32_t* per_seq_status)
{
    return guarded([&] {
        cp::Group group;
        for (int32_t i = 0; i < n; i++)
            group.push_back(cp::Entry{seqs[i], weights ? weights[i] : nullptr, lengths[i]});
        std::vector<cp::StatusType> st;
        cp::StatusType rc = batch->impl->add_poa_group(st, group);
        for (size_t i = 0; i < st.size(); i++)
            per_seq_status[i] = int32_t(st[i]);
        for (size_t i = st.size(); i < size_t(n); i++)
            per_seq_status[i] = int32_t(rc);
        return int32_t(rc);
    });
}

int32_t gwamd_poa_add_poa_group_resident(gwamd_poa_batch* batch, const gwamd_device_reads* const* sets,
                                         int32_t num_sets, const gwamd_read_slice* slices, int32_t n,
                                         int32_t* per_seq_status)
{
    return guarded([&] {
        if (!batch)
            throw std::invalid_argument("batch is NULL");
        if (num_sets < 0)
            throw std::invalid_argument("num_sets must not be negative");
        if (num_sets > 0 && !sets)
            throw std::invalid_argument("sets is NULL");
        if (n > 0 && !per_seq_status)
            throw std::invalid_argument("per_seq_status is NULL");
        std::vector<const gwamd::mapper::DeviceReads*> reads(static_cast<size_t>(num_sets));
        for (int32_t s = 0; s < num_sets; s++)
            reads[size_t(s)] = sets[s] ? sets[s]->reads.get() : nullptr;
        std::vector<cp::StatusType> st;
        const cp::StatusType rc = add_resident_checked(*batch->impl, st, reads, slices, n);
        for (size_t i = 0; i < st.size(); i++)
            per_seq_status[i] = int32_t(st[i]);
        for (size_t i = st.size(); i < size_t(n); i++)
            per_seq_status[i] = int32_t(rc);
        return int32_t(rc);
    });
}

int32_t gwamd_poa_add_poa_groups_resident(gwamd_poa_batch* batch, const gwamd_device_reads* const* sets,
                                          int32_t num_sets, const gwamd_read_slice* slices,
                                          const int32_t* group_counts, int32_t num_groups, int32_t* group_status,
                                          int32_t* per_seq_status, int32_t* num_added)
{
    if (num_added)
        *num_added = 0;
    return guarded([&] {
        if (!batch)
            throw std::invalid_argument("batch is NULL");
        if (!num_added)
            throw std::invalid_argument("num_added is NULL");
        if (num_sets < 0)
            throw std::invalid_argument("num_sets must not be negative");
        if (num_sets > 0 && !sets)
            throw std::invalid_argument("sets is NULL");
        std::vector<const gwamd::mapper::DeviceReads*> reads(static_cast<size_t>(num_sets));
        for (int32_t s = 0; s < num_sets; s++)
            reads[size_t(s)] = sets[s] ? sets[s]->reads.get() : nullptr;
        *num_added = add_resident_groups_checked(*batch->impl, reads, slices, group_counts, num_groups, group_status,
                                                 per_seq_status);
        return int32_t(*num_added < num_groups ? cp::StatusType::exceeded_maximum_poas : cp::StatusType::success);
    });
}

int32_t gwamd_internal_poa_download_inputs(gwamd_poa_batch* batch, uint8_t* seqs_out, int8_t* wts_out)
{
    return guarded([&] {
        if (!batch || !seqs_out != !wts_out)
            throw std::invalid_argument("batch is NULL, or one of seqs_out and wts_out");
        if (seqs_out) // both NULL: the count alone
            batch->impl->download_inputs(seqs_out, wts_out);
        return int32_t(batch->impl->input_bytes());
    });
}

int32_t gwamd_poa_get_total_poas(const gwamd_poa_batch* batch) { return batch->impl->get_total_poas(); }

int32_t gwamd_poa_generate_poa(gwamd_poa_batch* batch)
{
    return guarded([&] {
        batch->impl->generate_poa();
        return 0;
    });
}

int32_t gwamd_poa_upload(gwamd_poa_batch* batch)
{
    return guarded([&] {
        batch->impl->upload();
        return 0;
    });
}

int32_t gwamd_poa_launch(gwamd_poa_batch* batch)
{
    return guarded([&] {
        batch->impl->launch();
        return 0;
    });
}

int32_t gwamd_poa_synchronize(gwamd_poa_batch* batch)
{
    return guarded([&] {
        batch->impl->synchronize();
        return 0;
    });
}

int32_t gwamd_poa_get_consensus(gwamd_poa_batch* batch, int32_t* status, int32_t* lengths, const char** cons_base,
                                const uint16_t** cov_base, int32_t* stride)
{
    return guarded([&] {
        std::vector<std::string> cons;
        std::vector<std::vector<uint16_t>> cov;
        std::vector<cp::StatusType> st;
        cp::StatusType rc = batch->impl->get_consensus(cons, cov, st);
        if (rc != cp::StatusType::success)
            return int32_t(rc);
        for (size_t i = 0; i < st.size(); i++)
        {
            status[i]  = int32_t(st[i]);
            lengths[i] = int32_t(cons[i].size());
        }
        *cons_base = reinterpret_cast<const char*>(batch->impl->host_cons().data());
        *cov_base  = batch->impl->host_cov().data();
        *stride    = batch->impl->dims().max_consensus;
        return int32_t(rc);
    });
}

int32_t gwamd_poa_get_msa(gwamd_poa_batch* batch, int32_t* status, int32_t* num_rows, const char** msa_base,
                          int32_t* row_stride, int32_t* max_seqs)
{
    return guarded([&] {
        std::vector<std::vector<std::string>> msa;
        std::vector<cp::StatusType> st;
        cp::StatusType rc = batch->impl->get_msa(msa, st);
        if (rc != cp::StatusType::success)
            return int32_t(rc);
        for (size_t i = 0; i < st.size(); i++)
        {
            status[i]   = int32_t(st[i]);
            num_rows[i] = int32_t(msa[i].size());
        }
        *msa_base   = reinterpret_cast<const char*>(batch->impl->host_msa().data());
        *row_stride = batch->impl->dims().max_consensus;
        *max_seqs   = batch->impl->dims().max_seqs;
        return int32_t(rc);
    });
}

int32_t gwamd_poa_get_graphs(gwamd_poa_batch* batch, int32_t* status, int32_t* num_nodes, const uint8_t** bases,
                             const uint16_t** in_count, const int32_t** in_edges, const uint16_t** in_weights,
                             int32_t* max_nodes)
{
    return guarded([&] {
        batch->impl->fetch_graphs();
        const int32_t n = batch->impl->get_total_poas();
        for (int32_t w = 0; w < n; w++)
        {
            status[w]    = int32_t(batch->impl->graph_status(w));
            num_nodes[w] = batch->impl->host_final_nodes()[w];
        }
        *bases      = batch->impl->host_g_bases().data();
        *in_count   = batch->impl->host_g_in_cnt().data();
        *in_edges   = batch->impl->host_g_in_e().data();
        *in_weights = batch->impl->host_g_in_w().data();
        *max_nodes  = batch->impl->dims().max_nodes;
        return 0;
    });
}

int32_t gwamd_poa_batch_id(const gwamd_poa_batch* batch) { return batch->impl->batch_id(); }

void gwamd_poa_reset(gwamd_poa_batch* batch) { batch->impl->reset(); }

int32_t gwamd_poa_get_stats(gwamd_poa_batch* batch, int64_t* cells, int32_t* final_nodes)
{
    return guarded([&] {
        batch->impl->get_stats(cells, final_nodes);
        return 0;
    });
}

int32_t gwamd_poa_get_phase_ticks(gwamd_poa_batch* batch, int64_t* ticks)
{
    return guarded([&] {
        batch->impl->get_phases(ticks);
        return int32_t(gwamd::poa::kPhases);
    });
}

// Row-order counters of the last run, kOrderStats int32 per window
// (OrderStat, poa_common.hpp); returns the words per window (out == NULL:
// only that).
int32_t gwamd_internal_poa_order_stats(gwamd_poa_batch* batch, int32_t* out)
{
    return guarded([&] {
        if (out)
            batch->impl->get_order_stats(out);
        return int32_t(gwamd::poa::kOrderStats);
    });
}

int32_t gwamd_poa_get_types(const gwamd_poa_batch* batch, int32_t* score_bits, int32_t* size_bits)
{
    *score_bits = batch->impl->score_bits();
    *size_bits  = batch->impl->size_bits();
    return batch->impl->kernel_kind();
}

int32_t gwamd_poa_env_tuning(int32_t* tb_rank, int32_t* band_fwd, int32_t* force_v1, int32_t* diag)
{
    if (!tb_rank || !band_fwd || !force_v1 || !diag)
    {
        gwamd::host::last_error() = "gwamd_poa_env_tuning: NULL output";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    const gwamd::poa::PoaTuning t = gwamd::poa::read_poa_tuning();
    *tb_rank                      = t.tb_rank;
    *band_fwd                     = t.band_fwd;
    *force_v1                     = t.force_v1 ? 1 : 0;
    *diag                         = t.diag;
    return 0;
}

int32_t gwamd_poa_set_spoa_accurate(gwamd_poa_batch* batch, int32_t on)
{
    const int32_t was = batch->impl->spoa_accurate() ? 1 : 0;
    batch->impl->set_spoa_accurate(on != 0);
    return was;
}

int32_t gwamd_poa_get_capacity(const gwamd_poa_batch* batch, int64_t* device_bytes, int32_t* max_poas)
{
    *device_bytes = batch->impl->device_bytes();
    *max_poas     = batch->impl->max_poas();
    return 0;
}

int32_t gwamd_poa_get_grid(const gwamd_poa_batch* batch, int32_t* slots, int32_t* resident)
{
    *slots    = batch->impl->slots();
    *resident = batch->impl->resident_slots();
    return 0;
}

// Test hooks (tests/test_poa_add_waves.py): the fit rule of the LDS kernel's
// every-wave graph update (lds_add_bytes / lds_add_fits, poa_common.hpp), and
// what the host's plan makes of it for a full-alignment batch of these
// capacities without a device: returns the rule applied to the planned ring
// region, as the kernel applies it (-1 when no LDS kernel is planned), and the
// plan's ring region bytes, waves and LDS bytes.
long long gwamd_internal_poa_lds_add_bytes(int32_t max_seq_len, int32_t max_nodes)
{
    return gwamd::poa::lds_add_bytes(max_seq_len, max_nodes);
}

int32_t gwamd_internal_poa_lds_add_fits(int32_t max_seq_len, int32_t max_nodes, int32_t ring_bytes)
{
    return gwamd::poa::lds_add_fits(max_seq_len, max_nodes, ring_bytes) ? 1 : 0;
}

int32_t gwamd_internal_poa_lds_add_plan(int32_t max_seq_len, int32_t max_nodes, int32_t score_bits,
                                        int32_t* ring_bytes, int32_t* waves, int32_t* lds_bytes)
{
    gwamd::poa::Dims d{};
    d.max_nodes    = max_nodes;
    d.max_seq_len  = max_seq_len;
    d.score_stride = int32_t((int64_t(max_seq_len) + 48 + 7) & ~int64_t(7));
    d.score_rows   = max_nodes + 2;
    try
    {
        gwamd::poa::plan_lds_layout(d, false, 16, score_bits, gwamd::poa::read_poa_tuning());
    }
    catch (const std::exception& e)
    {
        gwamd::host::last_error() = e.what();
        return -2;
    }
    if (!d.lds_kernel)
        return -1;
    if (ring_bytes)
        *ring_bytes = d.lds_rec_off - d.lds_ring_off;
    if (waves)
        *waves = d.lds_waves;
    if (lds_bytes)
        *lds_bytes = d.lds_bytes;
    return gwamd::poa::lds_add_fits(d.max_seq_len, d.max_nodes, d.lds_rec_off - d.lds_ring_off) ? 1 : 0;
}

// Test hook (tests/test_poa_plan.py): the plan the batch constructor makes for
// these capacities (plan_batch), without a device.  Writes the values of
// gwamd_internal_poa_plan_fields() in that order (score_bits, size_bits, every
// field of the planned Dims, then kernel: 1 when the kernel table has a kernel
// for this plan) and returns their count; negative when planning throws
// (gwamd_last_error says why) or `cap` is too small.
// The BatchSize of the plan hooks: the three-argument one with the node
// capacities replaced (no band width <= sequence size rule, as for the tests' batches)
static cp::BatchSize hook_batch_size(int32_t max_sequence_size, int32_t max_sequences_per_poa, int32_t band_width,
                                     int32_t max_nodes_per_window, int32_t max_nodes_per_window_banded)
{
    cp::BatchSize bs(max_sequence_size, max_sequences_per_poa, band_width);
    bs.max_nodes_per_window              = cp::detail::align_up(max_nodes_per_window, 4);
    bs.max_nodes_per_window_banded       = cp::detail::align_up(max_nodes_per_window_banded, 4);
    bs.max_matrix_graph_dimension        = bs.max_nodes_per_window;
    bs.max_matrix_graph_dimension_banded = bs.max_nodes_per_window_banded;
    return bs;
}

#define GWAMD_PLAN_FIELDS(F)                                                                                  \
    F(max_nodes) F(max_seqs) F(max_seq_len) F(max_consensus) F(score_stride) F(score_rows) F(aln_cap)        \
    F(band_width) F(want_consensus) F(spoa_accurate) F(lds_kernel) F(lds_bytes) F(lds_ring_off)              \
    F(lds_ring_rows) F(lds_sh_off) F(lds_rec_off) F(lds_xl_off) F(lds_xl_cap) F(lds_cpl) F(lds_waves)        \
    F(code_stride) F(aux_stride) F(aux_carry_off) F(lds_work_bytes) F(aux_reca_off) F(aux_recb_off)          \
    F(aux_col0_off) F(aux_flag_off) F(aux_xl_off) F(aux_xl_cap) F(aux_bx_off) F(aux_recc_off)                \
    F(aux_rece_off) F(band_ad) F(tb_rank) F(diag)

const char* gwamd_internal_poa_plan_fields(void)
{
#define GWAMD_F(f) "," #f
    return "score_bits,size_bits" GWAMD_PLAN_FIELDS(GWAMD_F) ",kernel";
#undef GWAMD_F
}

int32_t gwamd_internal_poa_plan(int32_t max_sequence_size, int32_t max_sequences_per_poa, int32_t band_width,
                                int32_t max_nodes_per_window, int32_t max_nodes_per_window_banded, int32_t banded,
                                int32_t msa, int32_t gap, int32_t mismatch, int32_t match, int64_t* out, int32_t cap)
{
    return guarded([&]() -> int32_t {
        const cp::BatchSize bs = hook_batch_size(max_sequence_size, max_sequences_per_poa, band_width,
                                                 max_nodes_per_window, max_nodes_per_window_banded);
        int score_bits = 0, size_bits = 0;
        const gwamd::poa::Dims d =
            cp::plan_batch(bs, banded != 0, msa ? cp::OutputType::msa : cp::OutputType::consensus, int16_t(gap),
                           int16_t(mismatch), int16_t(match), gwamd::poa::read_poa_tuning(), score_bits, size_bits);
#define GWAMD_F(f) , int64_t(d.f)
        const bool found  = gwamd_internal_poa_kernel(&d, score_bits, size_bits, banded, msa).fn != nullptr;
        const int64_t v[] = {score_bits, size_bits GWAMD_PLAN_FIELDS(GWAMD_F), found ? 1 : 0};
#undef GWAMD_F
        const int32_t n = int32_t(sizeof(v) / sizeof(v[0]));
        if (!out || cap < n)
            return -1;
        std::copy(v, v + n, out);
        return n;
    });
}
#undef GWAMD_PLAN_FIELDS

// Test hooks (tests/test_poa_capacity.py), without a device.  The capacity and
// layout the batch constructor plans for these capacities (the arguments of
// gwamd_internal_poa_plan), `max_mem` bytes and a device of `cus` CUs holding
// `blocks_per_cu` workgroups of the planned kernel each: the values of
// gwamd_internal_poa_capacity_fields() in that order (PoaCapacity, the slab
// offset of every Buffers array or -1, the rest of PoaLayout, device_bytes);
// returns their count, negative as gwamd_internal_poa_plan does.
#define GWAMD_SLAB_NAME(name, bytes) #name ","
#define GWAMD_SLAB_VALUE(name, bytes) lay.name,
const char* gwamd_internal_poa_capacity_fields(void)
{
    return "max_poas,slots,resident,scorebuf_alloc,window_bytes,slot_bytes," GWAMD_POA_SLAB_ARRAYS(GWAMD_SLAB_NAME)
           "scores,slab_bytes,codes_bytes,seqs_bytes,wts_bytes,len_bytes,off_bytes,win_bytes,order_off,head_off,"
           "device_bytes";
}

int32_t gwamd_internal_poa_capacity(int32_t max_sequence_size, int32_t max_sequences_per_poa, int32_t band_width,
                                    int32_t max_nodes_per_window, int32_t max_nodes_per_window_banded,
                                    int32_t banded, int32_t msa, int32_t gap, int32_t mismatch, int32_t match,
                                    int64_t max_mem, int32_t cus, int32_t blocks_per_cu, int64_t* out, int32_t cap)
{
    return guarded([&]() -> int32_t {
        const cp::BatchSize bs = hook_batch_size(max_sequence_size, max_sequences_per_poa, band_width,
                                                 max_nodes_per_window, max_nodes_per_window_banded);
        const gwamd::poa::PoaTuning tune = gwamd::poa::read_poa_tuning();
        int score_bits = 0, size_bits = 0;
        const gwamd::poa::Dims d =
            cp::plan_batch(bs, banded != 0, msa ? cp::OutputType::msa : cp::OutputType::consensus, int16_t(gap),
                           int16_t(mismatch), int16_t(match), tune, score_bits, size_bits);
        const gwamd::poa::PoaCapacity c =
            gwamd::poa::plan_capacity({cus, blocks_per_cu}, d, cp::ref_sizes(bs, banded != 0), size_bits / 8,
                                      score_bits / 8, msa != 0, max_mem, tune.slots);
        const gwamd::poa::PoaLayout lay =
            gwamd::poa::plan_layout(d, size_bits / 8, score_bits / 8, msa != 0, c.max_poas, c.slots);
        const int64_t v[] = {c.max_poas, c.slots, c.resident, c.scorebuf_alloc, c.window_bytes, c.slot_bytes,
                             GWAMD_POA_SLAB_ARRAYS(GWAMD_SLAB_VALUE) lay.scores, lay.slab_bytes, lay.codes_bytes,
                             lay.seqs_bytes, lay.wts_bytes, lay.len_bytes, lay.off_bytes, lay.win_bytes,
                             lay.order_off, lay.head_off, lay.device_bytes()};
        const int32_t n = int32_t(sizeof(v) / sizeof(v[0]));
        if (!out || cap < n)
            return -1;
        std::copy(v, v + n, out);
        return n;
    });
}
#undef GWAMD_SLAB_NAME
#undef GWAMD_SLAB_VALUE

// The queue order of `n` windows (plan_window_order): `windows` holds a
// (first read, read count) pair per window, `seq_len` the read lengths.
// Writes the order when there is one (n entries) and returns the WindowOrder kind.
int32_t gwamd_internal_poa_window_order(const int32_t* windows, const int32_t* seq_len, int32_t n, int32_t cus,
                                        int32_t slots, int32_t persistent, int32_t* order)
{
    return guarded([&]() -> int32_t {
        static_assert(sizeof(gwamd::poa::WindowDesc) == 2 * sizeof(int32_t), "WindowDesc is two int32");
        std::vector<int32_t> o;
        const auto kind = gwamd::poa::plan_window_order(reinterpret_cast<const gwamd::poa::WindowDesc*>(windows),
                                                        seq_len, n, cus, slots, persistent != 0, o);
        std::copy(o.begin(), o.end(), order);
        return int32_t(kind);
    });
}

static size_t query_free_memory(uint64_t given)
{
    if (given != 0)
        return size_t(given);
    size_t free_mem = 0, total = 0;
    if (hipMemGetInfo(&free_mem, &total) != hipSuccess)
        throw std::runtime_error("hipMemGetInfo failed");
    return free_mem;
}

int64_t gwamd_poa_estimate_max_poas(int32_t max_seq_sz, int32_t max_seq_per_poa, int32_t band_width, int32_t banded,
                                    int32_t msa, uint64_t free_device_memory, float quota, int32_t mismatch,
                                    int32_t gap, int32_t match)
{
    int64_t r = 0;
    const int32_t rc = guarded([&]() -> int32_t {
        r = cp::estimate_max_poas(cp::BatchSize(max_seq_sz, max_seq_per_poa, band_width), banded != 0, msa != 0,
                                  query_free_memory(free_device_memory), quota, mismatch, gap, match);
        return 0;
    });
    return rc != 0 ? int64_t(rc) : r;
}

int32_t gwamd_poa_get_multi_batch_sizes(const int32_t* group_max_len, const int32_t* group_num_reads,
                                        int32_t num_groups, uint64_t free_device_memory, int32_t banded,
                                        int32_t msa, int32_t band_width, const int32_t* bins, int32_t num_bins,
                                        float quota, int32_t mismatch, int32_t gap, int32_t match,
                                        int32_t* num_batches, int32_t* batch_max_seq, int32_t* batch_num_reads,
                                        int32_t* group_batch, int32_t* group_rank)
{
    return guarded([&]() -> int32_t {
        // groups as Entry lists: only the longest read and the read count matter
        std::vector<cp::Group> groups(size_t(std::max(num_groups, 0)));
        for (int32_t i = 0; i < num_groups; i++)
        {
            groups[i].resize(size_t(std::max(group_num_reads[i], 1)));
            for (auto& e : groups[i])
                e = cp::Entry{nullptr, nullptr, 0};
            groups[i][0].length = group_max_len[i];
        }
        std::vector<int32_t> bin_vec;
        if (bins && num_bins > 0)
            bin_vec.assign(bins, bins + num_bins);
        std::vector<cp::BatchSize> sizes;
        std::vector<std::vector<int32_t>> per_batch;
        cp::get_multi_batch_sizes_for_memory(sizes, per_batch, groups, query_free_memory(free_device_memory),
                                         banded != 0, msa != 0, band_width, bin_vec.empty() ? nullptr : &bin_vec,
                                         quota, mismatch, gap, match);
        *num_batches = int32_t(sizes.size());
        for (size_t b = 0; b < sizes.size(); b++)
        {
            batch_max_seq[b]   = sizes[b].max_sequence_size;
            batch_num_reads[b] = sizes[b].max_sequences_per_poa;
            for (size_t r = 0; r < per_batch[b].size(); r++)
            {
                group_batch[per_batch[b][r]] = int32_t(b);
                group_rank[per_batch[b][r]]  = int32_t(r);
            }
        }
        return 0;
    });
}

} // extern "C"
