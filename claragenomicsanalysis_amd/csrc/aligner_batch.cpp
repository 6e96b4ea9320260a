// Host side of the MI355X global aligner: the reference's C++ API
// (create_aligner / Aligner / Alignment, cudaaligner/src/aligner.cpp,
// aligner_global.cpp, alignment_impl.cpp) and the C ABI of
// include/gwamd_cudaaligner.h.  Device work is in aligner_kernels.hip.
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>
#include <claraparabricks/genomeworks/cudaaligner/cudaaligner.hpp>

#include "aligner_common.hpp"
#include "aligner_plan.hpp"
#include "aligner_resident.hpp"
#include "allocator_handle.hpp"
#include "gwamd_cudaaligner.h"
#include "host_common.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

extern "C" gwamd::aln::KernelRef gwamd_internal_aligner_kernel(const gwamd::aln::KernelKey* k);
extern "C" hipError_t gwamd_internal_aligner_occupancy(const gwamd::aln::KernelKey* k, int lds_bytes,
                                                       int* blocks_per_cu);
extern "C" hipError_t gwamd_internal_aligner_launch(const gwamd::aln::Args* a, const gwamd::aln::KernelKey* k,
                                                    int grid, hipStream_t stream);

namespace
{
// What plan_slots asks of the current device for this layout.
gwamd::aln::DeviceFacts device_facts(const gwamd::aln::AlignerPlan& plan, int device_id)
{
    gwamd::aln::DeviceFacts f;
    GWAMD_HIP_CHECK(gwamd_internal_aligner_occupancy(&plan.occupancy_key, plan.args.lds_bytes, &f.per_cu));
    if (plan.uk_wide)
    {
        const gwamd::aln::KernelKey wide{plan.algo, 0, 1, 1024};
        GWAMD_HIP_CHECK(gwamd_internal_aligner_occupancy(&wide, plan.uk_wide_lds, &f.wide_per_cu));
    }
    GWAMD_HIP_CHECK(hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, device_id));
    if (plan.algo == gwamd::aln::kAlgoBanded || plan.algo == gwamd::aln::kAlgoUkkonen)
    {
        // (only the banded aligners' workspace cap looks at the free memory)
        size_t free_b = 0, total_b = 0;
        GWAMD_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        f.free_bytes = int64_t(free_b);
    }
    return f;
}
} // namespace

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

using gwamd::host::PinnedBuf;
using gwamd::host::ScopedDevice;

StatusType Init() { return StatusType::success; }

std::ostream& operator<<(std::ostream& os, const FormattedAlignment& f)
{
    // alignment.cpp:24-35
    const std::size_t line = (f.linebreak_after == 0) ? f.query.size() : f.linebreak_after;
    for (std::size_t i = 0; i < f.query.size(); i += line)
        os << f.query.substr(i, line) << '\n' << f.pairing.substr(i, line) << '\n' << f.target.substr(i, line) << '\n';
    os << std::endl;
    return os;
}

namespace
{

int32_t throw_on_negative(int32_t v, const char* msg)
{
    if (v < 0)
        throw std::invalid_argument(msg);
    return v;
}

// genomeutils::reverse_complement (genomeutils.hpp:137-150)
void reverse_complement(const char* src, int32_t n, char* dst)
{
    for (int32_t p = 0; p < n; p++)
    {
        const char c = src[n - 1 - p];
        dst[p]       = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
    }
}

char cigar_state(AlignmentState s)
{
    switch (s)
    {
    case AlignmentState::match:
    case AlignmentState::mismatch: return 'M';
    case AlignmentState::insertion: return 'I';
    case AlignmentState::deletion: return 'D';
    default: throw std::runtime_error("Unrecognized alignment state.");
    }
}

} // namespace

// AlignmentImpl (alignment_impl.cpp:24-112)
class AlignmentImpl : public Alignment
{
public:
    AlignmentImpl(const char* query, int32_t query_length, const char* target, int32_t target_length)
        : query_(query, query + throw_on_negative(query_length, "query_length has to be non-negative."))
        , target_(target, target + throw_on_negative(target_length, "target_length has to be non-negative."))
    {
    }
    const std::string& get_query_sequence() const override { return query_; }
    const std::string& get_target_sequence() const override { return target_; }
    AlignmentType get_alignment_type() const override { return type_; }
    StatusType get_status() const override { return status_; }
    const std::vector<AlignmentState>& get_alignment() const override { return alignment_; }
    void set_alignment_type(AlignmentType t) { type_ = t; }
    void set_status(StatusType s) { status_ = s; }
    void set_alignment(std::vector<AlignmentState>&& a) { alignment_ = std::move(a); }
    // the result storage, refilled in place by sync_alignments (an aligner
    // that aligns its batch again reuses the vectors' capacity)
    std::vector<AlignmentState>& alignment_storage() { return alignment_; }

    std::string convert_to_cigar() const override
    {
        if (alignment_.empty())
            return std::string();
        std::string cigar;
        char last   = cigar_state(alignment_[0]);
        int32_t cnt = 0;
        for (AlignmentState x : alignment_)
        {
            const char c = cigar_state(x);
            if (c == last)
                cnt++;
            else
            {
                cigar += std::to_string(cnt) + last;
                cnt  = 1;
                last = c;
            }
        }
        cigar += std::to_string(cnt) + last;
        return cigar;
    }

    FormattedAlignment format_alignment(int32_t maximal_line_length) const override
    {
        int64_t t = 0, q = 0;
        FormattedAlignment r;
        r.linebreak_after = (maximal_line_length < 0) ? 0 : maximal_line_length;
        for (AlignmentState x : alignment_)
        {
            switch (x)
            {
            case AlignmentState::match:
                r.target += target_[t++];
                r.query += query_[q++];
                r.pairing += '|';
                break;
            case AlignmentState::mismatch:
                r.target += target_[t++];
                r.query += query_[q++];
                r.pairing += 'x';
                break;
            case AlignmentState::deletion:
                r.target += '-';
                r.query += query_[q++];
                r.pairing += ' ';
                break;
            case AlignmentState::insertion:
                r.target += target_[t++];
                r.query += '-';
                r.pairing += ' ';
                break;
            default: throw std::runtime_error("Unknown alignment state");
            }
        }
        return r;
    }

private:
    std::string query_, target_;
    StatusType status_ = StatusType::uninitialized;
    AlignmentType type_ = AlignmentType::unset;
    std::vector<AlignmentState> alignment_;
};

// AlignerGlobal (aligner_global.cpp) with the HIP kernels of aligner_kernels.hip.
class AlignerGlobalHip : public Aligner
{
public:
    // budget: the pool of the caller's DefaultDeviceAllocator (null or a
    // negative capacity: all available memory, allocator.hpp:282-305), shared
    // by every aligner made from copies of that allocator.  The reference
    // serves every device buffer of the aligner from that pool; here the
    // fixed buffers (sequences, paths, lengths) come first and the workspace
    // gets as many persistent-grid slots as what is left of the pool holds;
    // less than the fixed buffers plus one slot throws, as the reference's
    // pool does when an allocation does not fit.  The bytes stay reserved
    // until the aligner is destroyed.
    AlignerGlobalHip(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments, int algorithm,
                     hipStream_t stream, int32_t device_id, std::shared_ptr<DeviceBudget> budget = nullptr)
        : max_q_(throw_on_negative(max_query_length, "max_query_length must be non-negative."))
        , max_t_(throw_on_negative(max_target_length, "max_target_length must be non-negative."))
        , max_n_(throw_on_negative(max_alignments, "max_alignments must be non-negative."))
        , algo_(algorithm)
        , stream_(stream)
        , device_id_(device_id)
        , tuning_(gwamd::aln::read_aligner_tuning())
    {
        if (max_alignments < 1)
            throw std::runtime_error("Max alignments must be at least 1.");
        plan_       = gwamd::aln::plan_layout(algo_, max_q_, max_t_, max_n_, tuning_);
        stride_     = plan_.args.stride;
        max_result_ = plan_.args.max_path_length;
        ScopedDevice dev(device_id_);
        slot_plan_          = gwamd::aln::plan_slots(plan_, device_facts(plan_, device_id_), max_n_, tuning_);
        slots_              = slot_plan_.slots;
        const int64_t fixed = plan_.fixed_bytes;
        if (budget && budget->capacity() >= 0)
        {
            const int64_t sb  = std::max<int64_t>(1, plan_.slot_bytes);
            const int64_t got = reserved_.reserve(budget, fixed + sb, fixed + int64_t(slots_) * sb);
            if (got < 0)
                throw std::runtime_error("The aligner needs " + std::to_string(fixed + sb) +
                                         " device bytes, more than its allocator has left (" +
                                         std::to_string(budget->capacity() - budget->used()) + " of " +
                                         std::to_string(budget->capacity()) + ").");
            slots_ = int32_t(std::min<int64_t>(slots_, (got - fixed) / sb));
            // keep exactly what this aligner uses
            reserved_.trim(fixed + int64_t(slots_) * sb);
        }
        device_bytes_ = fixed + int64_t(slots_) * plan_.slot_bytes;
        // (at least 16 bytes each; the workspace is not cleared: every slot
        // entry is written before it is read)
        auto zeroed = [&](auto& buf, size_t n) {
            buf.alloc(std::max(n, 16 / sizeof(*buf.data())), nullptr);
            GWAMD_HIP_CHECK(hipMemsetAsync(buf.data(), 0, buf.size() * sizeof(*buf.data()), stream_));
        };
        zeroed(d_seqs_, size_t(2) * stride_ * max_n_ + 16);
        zeroed(d_lens_, size_t(2) * max_n_);
        zeroed(d_paths_, size_t(max_result_) * max_n_ + 16);
        zeroed(d_plen_, size_t(max_n_));
        zeroed(d_stats_, 4);
        if (algo_ == GWAMD_ALIGNER_MYERS_BANDED)
            d_spec_ed_.alloc(size_t(max_n_) * gwamd::aln::kMaxSpecSweeps, nullptr);
        d_ws_.alloc(std::max<size_t>(size_t(slots_) * size_t(plan_.slot_bytes), 16), nullptr);
        h_seqs_.reserve(size_t(2) * stride_ * max_n_ + 16, stream_);
        h_lens_.reserve(size_t(2) * max_n_ * 4, stream_);
        h_paths_.reserve(size_t(max_result_) * max_n_ + 16, stream_);
        h_plen_.reserve(size_t(max_n_) * 4, stream_);
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
        pipe_ = std::make_unique<Pipeline>(); // (here, not as a member: on this aligner's device, after the checks)
    }

    ~AlignerGlobalHip() override
    {
        // the side streams may still run this aligner's work
        (void)hipSetDevice(device_id_);
        for (hipStream_t st : {hipStream_t(pipe_->stream2), hipStream_t(pipe_->s_in), hipStream_t(pipe_->s_out)})
            (void)hipStreamSynchronize(st);
    }

    StatusType add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                             bool rc_query, bool rc_target) override
    {
        if (device_added_) // a batch is all host-added or all device-added
            return StatusType::generic_error;
        const int32_t n     = int32_t(alignments_.size());
        const StatusType ok = can_add(n, query_length, target_length);
        if (ok != StatusType::success)
            return ok;
        char* qd = h_seqs_.as<char>() + size_t(2 * n) * stride_;
        char* td = h_seqs_.as<char>() + size_t(2 * n + 1) * stride_;
        if (rc_query)
            reverse_complement(query, query_length, qd);
        else if (query_length > 0)
            std::memcpy(qd, query, size_t(query_length));
        if (rc_target)
            reverse_complement(target, target_length, td);
        else if (target_length > 0)
            std::memcpy(td, target, size_t(target_length));
        h_lens_.as<int32_t>()[2 * n]     = query_length;
        h_lens_.as<int32_t>()[2 * n + 1] = target_length;
        max_diff_ = std::max(max_diff_, std::abs(query_length - target_length));
        auto a = std::make_shared<AlignmentImpl>(qd, query_length, td, target_length);
        a->set_alignment_type(AlignmentType::global_alignment);
        alignments_.push_back(a);
        return StatusType::success;
    }

    // The overlap regions of `count` overlaps added from reads resident on this
    // aligner's device (not part of the Aligner interface: aligner_resident.hpp).
    // Lengths and statuses are checked on the host as add_alignment checks
    // them, all before anything is added; the sequences are written into the
    // device buffer by gather_overlap_regions_kernel on the aligner's stream,
    // so the Alignment objects carry no sequence copies and the uploads skip
    // the sequence buffer for this batch.  The caller has checked the overlaps
    // against the reads (gwamd::mapper::check_overlaps).
    StatusType add_device_overlaps(const gwamd::mapper::DeviceReads& query, const gwamd::mapper::DeviceReads& target,
                                   const gwamd::mapper::OverlapRecord* overlaps, int32_t count)
    {
        if (count < 0 || (!alignments_.empty() && !device_added_))
            return StatusType::generic_error;
        if (query.device_id != device_id_ || target.device_id != device_id_)
            return StatusType::generic_error;
        const int32_t n = int32_t(alignments_.size());
        for (int32_t k = 0; k < count; k++)
        {
            const gwamd::mapper::OverlapRecord& o = overlaps[k];
            const StatusType ok = can_add(n + k, int32_t(o.query_end - o.query_start),
                                          int32_t(o.target_end - o.target_start));
            if (ok != StatusType::success)
                return ok;
        }
        if (count == 0)
            return StatusType::success;
        ScopedDevice dev(device_id_);
        // the records of every device-added range of the batch stay until reset(): the gather reads them in stream order
        d_records_.emplace_back(size_t(count), nullptr);
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_records_.back().data(), overlaps,
                                       size_t(count) * sizeof(gwamd::mapper::OverlapRecord), hipMemcpyHostToDevice,
                                       stream_));
        gwamd::mapper::gather_overlap_regions(d_seqs_.data() + size_t(2 * n) * stride_, d_lens_.data() + 2 * n,
                                              d_records_.back().data(), count, stride_, query, target, stream_);
        // (the pageable source is staged before hipMemcpyAsync returns only for small copies: wait for it)
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
        for (int32_t k = 0; k < count; k++)
        {
            const int32_t ql = int32_t(overlaps[k].query_end - overlaps[k].query_start);
            const int32_t tl = int32_t(overlaps[k].target_end - overlaps[k].target_start);
            h_lens_.as<int32_t>()[2 * (n + k)]     = ql;
            h_lens_.as<int32_t>()[2 * (n + k) + 1] = tl;
            max_diff_ = std::max(max_diff_, std::abs(ql - tl));
            auto a = std::make_shared<AlignmentImpl>("", 0, "", 0);
            a->set_alignment_type(AlignmentType::global_alignment);
            alignments_.push_back(a);
        }
        device_added_ = true;
        return StatusType::success;
    }

    // aligner_global.cpp:131-159 (H2D, kernel, D2H on the aligner's stream).
    // Batches of many grids' worth of pairs run as a pipeline of stages: the
    // pairs are cut into K consecutive chunks; all uploads go back to back on
    // a copy-in stream, chunk k's kernel runs on half of the workspace slots
    // (k % 2, one compute stream per half) once its upload is in, and its
    // download follows on a copy-out stream, so copies overlap the kernels
    // and sync_alignments fills each chunk's results on the host while later
    // chunks are still aligning.  Results are the same pair by pair; the
    // aligner's stream waits for every stage.
    StatusType align_all() override
    {
        if (alignments_.empty())
            return StatusType::success;
        ScopedDevice dev(device_id_);
        const int32_t n = int32_t(alignments_.size());
        stages_         = gwamd::aln::pipeline_stages(slots_, n, tuning_);
        if (stages_ <= 1)
        {
            stages_ = 1;
            chunk0_[0] = 0, chunk0_[1] = n;
            upload();
            launch(); // records pipe_->ev_k[0] / pipe_->ev_k[1] around the kernel
            if (!keep_on_device_)
                download();
            GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_d[0], stream_));
            return StatusType::success;
        }
        GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_fork, stream_));
        for (hipStream_t st : {hipStream_t(pipe_->s_in), hipStream_t(pipe_->stream2), hipStream_t(pipe_->s_out)})
            GWAMD_HIP_CHECK(hipStreamWaitEvent(st, pipe_->ev_fork, 0));
        const int32_t half_slots = slots_ / 2;
        for (int k = 0; k < stages_; k++)
        {
            const int32_t i0 = int32_t(int64_t(n) * k / stages_);
            const int32_t c  = int32_t(int64_t(n) * (k + 1) / stages_) - i0;
            chunk0_[k]       = i0;
            chunk0_[k + 1]   = i0 + c;
            GWAMD_HIP_CHECK(hipMemcpyAsync(d_lens_.data() + 2 * size_t(i0), h_lens_.as<int32_t>() + 2 * size_t(i0),
                                           2 * size_t(c) * 4, hipMemcpyHostToDevice, pipe_->s_in));
            if (!device_added_) // (device-added: already gathered on stream_, before ev_fork)
                GWAMD_HIP_CHECK(hipMemcpyAsync(d_seqs_.data() + 2 * size_t(i0) * stride_,
                                               h_seqs_.as<char>() + 2 * size_t(i0) * stride_,
                                               2 * size_t(c) * stride_, hipMemcpyHostToDevice, pipe_->s_in));
            GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_h[k], pipe_->s_in));
        }
        for (int k = 0; k < stages_; k++)
        {
            hipStream_t st   = (k & 1) ? pipe_->stream2 : stream_;
            const int32_t i0 = chunk0_[k], c = chunk0_[k + 1] - chunk0_[k];
            GWAMD_HIP_CHECK(hipStreamWaitEvent(st, pipe_->ev_h[k], 0));
            GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_k[2 * k], st));
            launch_range(i0, c, (k & 1) * half_slots, (k & 1) ? slots_ - half_slots : half_slots, st);
            GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_k[2 * k + 1], st));
            GWAMD_HIP_CHECK(hipStreamWaitEvent(pipe_->s_out, pipe_->ev_k[2 * k + 1], 0));
            if (!keep_on_device_)
            {
                GWAMD_HIP_CHECK(hipMemcpyAsync(h_paths_.as<int8_t>() + size_t(i0) * max_result_,
                                               d_paths_.data() + size_t(i0) * max_result_, size_t(c) * max_result_,
                                               hipMemcpyDeviceToHost, pipe_->s_out));
                GWAMD_HIP_CHECK(hipMemcpyAsync(h_plen_.as<int32_t>() + i0, d_plen_.data() + i0, size_t(c) * 4,
                                               hipMemcpyDeviceToHost, pipe_->s_out));
            }
            GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_d[k], pipe_->s_out));
        }
        GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_join, pipe_->s_out)); // after every kernel and download
        GWAMD_HIP_CHECK(hipStreamWaitEvent(stream_, pipe_->ev_join, 0));
        return StatusType::success;
    }

    // Kernel time of the last align_all(): the union of its launches'
    // intervals (HIP events on their streams), ms.
    double last_kernel_ms()
    {
        ScopedDevice dev(device_id_);
        if (stages_ == 0)
            return 0.0;
        std::vector<std::pair<double, double>> iv;
        for (int k = 0; k < stages_; k++)
        {
            GWAMD_HIP_CHECK(hipEventSynchronize(pipe_->ev_k[2 * k + 1]));
            float a = 0.f, b = 0.f;
            GWAMD_HIP_CHECK(hipEventElapsedTime(&a, pipe_->ev_k[0], pipe_->ev_k[2 * k]));
            GWAMD_HIP_CHECK(hipEventElapsedTime(&b, pipe_->ev_k[0], pipe_->ev_k[2 * k + 1]));
            iv.emplace_back(double(a), double(b));
        }
        std::sort(iv.begin(), iv.end());
        double total = 0.0, lo = iv[0].first, hi = iv[0].second;
        for (size_t k = 1; k < iv.size(); k++)
        {
            if (iv[k].first > hi)
            {
                total += hi - lo;
                lo = iv[k].first;
            }
            hi = std::max(hi, iv[k].second);
        }
        return total + (hi - lo);
    }

    StatusType sync_alignments() override
    {
        // aligner_global.cpp:161-189: paths come out end -> start
        ScopedDevice dev(device_id_);
        const int32_t n = int32_t(alignments_.size());
        auto fill       = [&](int32_t i0, int32_t i1) {
            for (int32_t i = i0; i < i1; i++)
            {
                const int32_t len = h_plen_.as<int32_t>()[i];
                const int8_t* p   = h_paths_.as<int8_t>() + size_t(i) * max_result_;
                auto* a           = static_cast<AlignmentImpl*>(alignments_[size_t(i)].get());
                std::vector<AlignmentState>& st = a->alignment_storage();
                st.resize(size_t(std::max(len, 0)));
                for (int32_t k = 0; k < len; k++)
                    st[size_t(len - 1 - k)] = static_cast<AlignmentState>(p[k]);
                a->set_status(StatusType::success);
            }
        };
        // the alignments are independent: large batches are filled by a few
        // host threads (each alignment object is touched by one thread)
        auto fill_range = [&](int32_t b0, int32_t b1) {
            const int32_t m   = b1 - b0;
            const int32_t nth = m < 4096 ? 1 : int32_t(std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
            if (nth <= 1)
            {
                fill(b0, b1);
                return;
            }
            std::vector<std::thread> th;
            const int32_t per = (m + nth - 1) / nth;
            for (int32_t t = 0; t < nth; t++)
                th.emplace_back(fill, b0 + std::min(m, t * per), b0 + std::min(m, (t + 1) * per));
            for (auto& t : th)
                t.join();
        };
        if (stages_ > 1 && chunk0_[stages_] == n)
        {
            // each stage's paths reach the host while later stages are still
            // aligning: fill them as they arrive
            for (int k = 0; k < stages_; k++)
            {
                GWAMD_HIP_CHECK(hipEventSynchronize(pipe_->ev_d[k]));
                fill_range(chunk0_[k], chunk0_[k + 1]);
            }
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
        }
        else
        {
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
            fill_range(0, n);
        }
        return StatusType::success;
    }

    const std::vector<std::shared_ptr<Alignment>>& get_alignments() const override { return alignments_; }
    void reset() override
    {
        alignments_.clear();
        max_diff_ = 0;
        stages_   = 0; // no launch of this batch yet
        if (device_added_)
        {
            // a gather of the batch may still read its records
            ScopedDevice dev(device_id_);
            (void)hipStreamSynchronize(stream_);
            d_records_.clear();
            device_added_ = false;
        }
    }

    // bench / C ABI helpers: the split path (upload, launch, download) runs
    // one stage on stream_, so sync_alignments waits for stream_ before it
    // fills and last_kernel_ms times that launch (the state of an
    // earlier pipelined align_all() must not survive into a split launch)
    void upload()
    {
        ScopedDevice dev(device_id_);
        const size_t n = alignments_.size();
        stages_        = 1;
        chunk0_[0]     = 0;
        chunk0_[1]     = int32_t(n);
        GWAMD_HIP_CHECK(hipMemcpyAsync(d_lens_.data(), h_lens_.as<int32_t>(), 2 * n * 4, hipMemcpyHostToDevice, stream_));
        if (!device_added_)
            GWAMD_HIP_CHECK(hipMemcpyAsync(d_seqs_.data(), h_seqs_.as<char>(), 2 * n * size_t(stride_),
                                           hipMemcpyHostToDevice, stream_));
    }
    void launch()
    {
        ScopedDevice dev(device_id_);
        stages_    = 1;
        chunk0_[0] = 0;
        chunk0_[1] = int32_t(alignments_.size());
        GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_k[0], stream_));
        launch_range(0, int32_t(alignments_.size()), 0, slots_, stream_);
        GWAMD_HIP_CHECK(hipEventRecord(pipe_->ev_k[1], stream_));
    }
    // Pairs [i0, i0 + count) on workspace slots [slot0, slot0 + nslots).
    void launch_range(int32_t i0, int32_t count, int32_t slot0, int32_t nslots, hipStream_t s)
    {
        ScopedDevice dev(device_id_);
        int32_t mq = 0; // the longest query of these pairs, where the launch plan asks
        if (gwamd::aln::launch_needs_max_query(plan_))
            for (int32_t k = i0; k < i0 + count; k++)
                mq = std::max(mq, h_lens_.as<int32_t>()[2 * size_t(k)]);
        const gwamd::aln::LaunchPlan l = gwamd::aln::plan_launch(plan_, slot_plan_, count, nslots, mq, max_diff_);
        gwamd::aln::Args a = args();
        a.seqs     = d_seqs_.data() + 2 * size_t(i0) * stride_;
        a.lens     = d_lens_.data() + 2 * size_t(i0);
        a.paths    = d_paths_.data() + size_t(i0) * max_result_;
        a.path_len = d_plen_.data() + i0;
        a.n        = count;
        // run-ahead distances of this stage's pairs: stages on the two compute
        // streams must not share [0, count * sweeps)
        if (a.spec_ed)
            a.spec_ed = a.spec_ed + size_t(i0) * gwamd::aln::kMaxSpecSweeps;
        a.ws           = d_ws_.data() + size_t(slot0) * size_t(plan_.slot_bytes);
        a.uk_threads   = l.uk_threads;
        a.lds_bytes    = l.lds_bytes;
        a.lds_tile_off = l.lds_tile_off;
        a.tile_bytes   = l.tile_bytes;
        a.band_waves   = l.band_waves;
        a.spec_sweeps  = l.spec_sweeps;
        // band doubling run ahead: two launches, spec_phase 1 then 2
        for (int k = 0; k < (l.spec_sweeps > 0 ? 2 : 1); k++)
        {
            a.spec_phase = l.spec_sweeps > 0 ? k + 1 : 0;
            GWAMD_HIP_CHECK(gwamd_internal_aligner_launch(&a, &l.key, l.grid[k], s));
        }
    }
    void download()
    {
        ScopedDevice dev(device_id_);
        const size_t n = alignments_.size();
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_paths_.as<int8_t>(), d_paths_.data(), n * size_t(max_result_),
                                       hipMemcpyDeviceToHost, stream_));
        GWAMD_HIP_CHECK(hipMemcpyAsync(h_plen_.as<int32_t>(), d_plen_.data(), n * 4, hipMemcpyDeviceToHost, stream_));
    }
    void synchronize()
    {
        ScopedDevice dev(device_id_);
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    // the internal view of the device path buffer (aligner_resident.hpp)
    gwamd::aln::DevicePaths device_paths() const
    {
        return {d_paths_.data(), int64_t(d_paths_.size()), d_plen_.data(), max_result_, stream_};
    }
    void keep_paths_on_device(bool keep) { keep_on_device_ = keep; }
    const int8_t* host_paths() const { return h_paths_.as<int8_t>(); }
    const int32_t* host_path_lengths() const { return h_plen_.as<int32_t>(); }
    int32_t max_result_length() const { return max_result_; }
    int32_t grid() const { return slots_; }
    void path_stats(int64_t* out)
    {
        ScopedDevice dev(device_id_);
        unsigned long long v[3] = {0, 0, 0};
        GWAMD_HIP_CHECK(hipStreamSynchronize(stream_));
        GWAMD_HIP_CHECK(hipMemcpy(v, d_stats_.data(), sizeof(v), hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; i++)
            out[i] = int64_t(v[i]);
    }
    int64_t device_bytes() const { return device_bytes_; }

private:
    int32_t ukkonen_max_difference() const { return gwamd::aln::ukkonen_max_difference(max_t_); }

    // whether a pair of these lengths can be the n-th of the batch
    StatusType can_add(int32_t n, int32_t query_length, int32_t target_length) const
    {
        // AlignerGlobalUkkonen::add_alignment (aligner_global_ukkonen.cpp:47-57)
        if (algo_ == GWAMD_ALIGNER_UKKONEN && std::abs(query_length - target_length) > ukkonen_max_difference())
            return StatusType::exceeded_max_alignment_difference;
        // aligner_global.cpp:60-118
        if (query_length < 0 || target_length < 0)
            return StatusType::generic_error;
        if (n >= max_n_)
            return StatusType::exceeded_max_alignments;
        if (query_length > max_q_)
            return StatusType::exceeded_max_length;
        if (target_length > max_t_)
            return StatusType::exceeded_max_length;
        return StatusType::success;
    }

    // the planned layout with this aligner's arrays, for the whole batch
    gwamd::aln::Args args() const
    {
        gwamd::aln::Args a = plan_.args;
        a.seqs             = d_seqs_.data();
        a.lens             = d_lens_.data();
        a.paths            = d_paths_.data();
        a.path_len         = d_plen_.data();
        a.ws               = d_ws_.data();
        a.spec_ed          = d_spec_ed_.data();
        a.stats            = d_stats_.data();
        a.n                = int32_t(alignments_.size());
        return a;
    }

    struct UntimedEvent : gwamd::host::OwnedEvent
    {
        UntimedEvent() : OwnedEvent(hipEventDisableTiming) {}
    };
    // pipelined align_all(): the second compute stream, the copy-in and
    // copy-out streams, fork / join events, per stage the upload-done and
    // download-done events and the kernel's start / stop events
    struct Pipeline
    {
        gwamd::host::OwnedStream stream2, s_in, s_out;
        gwamd::host::OwnedEvent ev_fork, ev_join;
        UntimedEvent ev_d[gwamd::aln::kMaxStages], ev_h[gwamd::aln::kMaxStages];
        gwamd::host::OwnedEvent ev_k[2 * gwamd::aln::kMaxStages];
    };

    int32_t max_q_, max_t_, max_n_;
    int algo_;
    hipStream_t stream_;
    int32_t device_id_;
    const gwamd::aln::AlignerTuning tuning_; // the switches as they were at construction
    gwamd::aln::AlignerPlan plan_;
    gwamd::aln::SlotPlan slot_plan_;
    int32_t slots_ = 1; // slot_plan_.slots, or as many as the allocator's pool had room for
    int32_t stride_ = 0, max_result_ = 0;
    int32_t max_diff_ = 0; // largest |query - target| of the batch
    bool device_added_ = false; // the batch's sequences were gathered on the device: no upload of h_seqs_
    bool keep_on_device_ = false; // align_all() leaves the paths on the device (keep_paths_on_device)
    // stages of the last align_all() (0: none yet) and their first pairs
    int stages_                                 = 0;
    int32_t chunk0_[gwamd::aln::kMaxStages + 1] = {};
    int64_t device_bytes_                       = 0;
    gwamd::host::PoolReservation reserved_; // of the allocator pool; before the arrays, so released after them
    gwamd::host::DevBuf<char> d_seqs_;
    gwamd::host::DevBuf<int32_t> d_lens_;
    gwamd::host::DevBuf<int8_t> d_paths_;
    gwamd::host::DevBuf<int32_t> d_plen_;
    gwamd::host::DevBuf<uint8_t> d_ws_;
    gwamd::host::DevBuf<unsigned long long> d_stats_;
    gwamd::host::DevBuf<int32_t> d_spec_ed_; // banded Myers: distances of the sweeps run ahead
    std::vector<gwamd::host::DevBuf<gwamd::mapper::OverlapRecord>> d_records_; // of the device-added ranges
    std::unique_ptr<Pipeline> pipe_;
    PinnedBuf h_seqs_, h_lens_, h_paths_, h_plen_;
    std::vector<std::shared_ptr<Alignment>> alignments_;
};

std::unique_ptr<Aligner> create_aligner(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                        AlignmentType type, DefaultDeviceAllocator allocator, hipStream_t stream,
                                        int32_t device_id)
{
    // aligner.cpp:30-38
    if (type == AlignmentType::global_alignment)
        return std::make_unique<AlignerGlobalHip>(max_query_length, max_target_length, max_alignments,
                                                  GWAMD_ALIGNER_HIRSCHBERG_MYERS, stream, device_id,
                                                  allocator.budget());
    throw std::runtime_error("Aligner for specified type not implemented yet.");
}

std::unique_ptr<Aligner> create_global_aligner(int32_t max_query_length, int32_t max_target_length,
                                               int32_t max_alignments, GlobalAlgorithm algorithm, hipStream_t stream,
                                               int32_t device_id)
{
    const int algo = int(algorithm);
    if (algo < GWAMD_ALIGNER_HIRSCHBERG_MYERS || algo > GWAMD_ALIGNER_UKKONEN)
        throw std::invalid_argument("unknown aligner algorithm");
    return std::make_unique<AlignerGlobalHip>(max_query_length, max_target_length, max_alignments, algo, stream,
                                              device_id);
}

std::unique_ptr<Aligner> create_aligner(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                        AlignmentType type, hipStream_t stream, int32_t device_id,
                                        int64_t max_device_memory_allocator_caching_size)
{
    // aligner.cpp:40-63
    if (max_device_memory_allocator_caching_size < -1)
        throw std::invalid_argument("max_device_memory_allocator_caching_size has to be either -1 (=all available "
                                    "GPU memory) or greater or equal than 0.");
    return create_aligner(max_query_length, max_target_length, max_alignments, type,
                          DefaultDeviceAllocator(max_device_memory_allocator_caching_size), stream, device_id);
}

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks

namespace gwamd
{
namespace aln
{
claraparabricks::genomeworks::cudaaligner::StatusType
add_device_overlaps(claraparabricks::genomeworks::cudaaligner::Aligner& aligner, const gwamd::mapper::DeviceReads& query,
                    const gwamd::mapper::DeviceReads& target, const gwamd::mapper::OverlapRecord* overlaps,
                    int32_t count)
{
    auto* impl = dynamic_cast<claraparabricks::genomeworks::cudaaligner::AlignerGlobalHip*>(&aligner);
    if (!impl)
        throw std::invalid_argument("add_device_overlaps: not an aligner of create_aligner");
    return impl->add_device_overlaps(query, target, overlaps, count);
}

DevicePaths device_paths(claraparabricks::genomeworks::cudaaligner::Aligner& aligner)
{
    auto* impl = dynamic_cast<claraparabricks::genomeworks::cudaaligner::AlignerGlobalHip*>(&aligner);
    if (!impl)
        throw std::invalid_argument("device_paths: not an aligner of create_aligner");
    return impl->device_paths();
}

void keep_paths_on_device(claraparabricks::genomeworks::cudaaligner::Aligner& aligner, bool keep)
{
    auto* impl = dynamic_cast<claraparabricks::genomeworks::cudaaligner::AlignerGlobalHip*>(&aligner);
    if (!impl)
        throw std::invalid_argument("keep_paths_on_device: not an aligner of create_aligner");
    impl->keep_paths_on_device(keep);
}
} // namespace aln
} // namespace gwamd

// ===========================================================================
// C ABI (include/gwamd_cudaaligner.h)
// ===========================================================================
namespace ca = claraparabricks::genomeworks::cudaaligner;

namespace
{
template <typename F>
int32_t guarded_aln(F&& f)
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
} // namespace

struct gwamd_aligner
{
    std::unique_ptr<ca::AlignerGlobalHip> impl;
};

extern "C" {

int32_t gwamd_aligner_create(gwamd_aligner** out, int32_t max_query_length, int32_t max_target_length,
                             int32_t max_alignments, int32_t alignment_type, int32_t algorithm, void* stream,
                             int32_t device_id, int64_t max_caching)
{
    return guarded_aln([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (max_caching < -1)
            throw std::invalid_argument("max_device_memory_allocator_caching_size has to be either -1 (=all "
                                        "available GPU memory) or greater or equal than 0.");
        if (alignment_type != ca::AlignmentType::global_alignment)
            throw std::runtime_error("Aligner for specified type not implemented yet.");
        if (algorithm < GWAMD_ALIGNER_HIRSCHBERG_MYERS || algorithm > GWAMD_ALIGNER_UKKONEN)
            throw std::invalid_argument("unknown aligner algorithm");
        auto h  = std::make_unique<gwamd_aligner>();
        h->impl = std::make_unique<ca::AlignerGlobalHip>(
            max_query_length, max_target_length, max_alignments, algorithm, static_cast<hipStream_t>(stream),
            device_id, max_caching >= 0 ? std::make_shared<claraparabricks::genomeworks::DeviceBudget>(max_caching)
                                        : nullptr);
        *out    = h.release();
        return int32_t(0);
    });
}

void gwamd_aligner_destroy(gwamd_aligner* a) { delete a; }

int32_t gwamd_device_allocator_create(gwamd_device_allocator** out, int64_t max_caching_size)
{
    return guarded_aln([&] {
        if (!out)
            throw std::invalid_argument("out is NULL");
        if (max_caching_size < -1)
            throw std::invalid_argument("max_caching_size has to be either -1 (=all available GPU memory) or "
                                        "greater or equal than 0.");
        auto h   = std::make_unique<gwamd_device_allocator>();
        h->alloc = claraparabricks::genomeworks::create_default_device_allocator(max_caching_size);
        *out     = h.release();
        return int32_t(0);
    });
}

void gwamd_device_allocator_destroy(gwamd_device_allocator* a) { delete a; }

int64_t gwamd_device_allocator_capacity(const gwamd_device_allocator* a)
{
    return a ? a->alloc.max_cached_bytes() : -1;
}

int64_t gwamd_device_allocator_used(const gwamd_device_allocator* a)
{
    return a && a->alloc.budget() ? a->alloc.budget()->used() : 0;
}

int64_t gwamd_device_allocator_default_size(void)
{
    return claraparabricks::genomeworks::create_default_device_allocator().max_cached_bytes();
}

int32_t gwamd_aligner_create_with_allocator(gwamd_aligner** out, int32_t max_query_length, int32_t max_target_length,
                                            int32_t max_alignments, int32_t alignment_type, int32_t algorithm,
                                            void* stream, int32_t device_id, gwamd_device_allocator* allocator)
{
    return guarded_aln([&] {
        if (!out || !allocator)
            throw std::invalid_argument("out or allocator is NULL");
        if (alignment_type != ca::AlignmentType::global_alignment)
            throw std::runtime_error("Aligner for specified type not implemented yet.");
        if (algorithm < GWAMD_ALIGNER_HIRSCHBERG_MYERS || algorithm > GWAMD_ALIGNER_UKKONEN)
            throw std::invalid_argument("unknown aligner algorithm");
        auto h  = std::make_unique<gwamd_aligner>();
        h->impl = std::make_unique<ca::AlignerGlobalHip>(max_query_length, max_target_length, max_alignments,
                                                         algorithm, static_cast<hipStream_t>(stream), device_id,
                                                         allocator->alloc.budget());
        *out    = h.release();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_add_alignment(gwamd_aligner* a, const char* q, int32_t qlen, const char* t, int32_t tlen,
                                    int32_t rc_q, int32_t rc_t)
{
    return guarded_aln([&] { return int32_t(a->impl->add_alignment(q, qlen, t, tlen, rc_q != 0, rc_t != 0)); });
}

int32_t gwamd_aligner_align_all(gwamd_aligner* a)
{
    return guarded_aln([&] { return int32_t(a->impl->align_all()); });
}

int32_t gwamd_aligner_sync_alignments(gwamd_aligner* a)
{
    return guarded_aln([&] { return int32_t(a->impl->sync_alignments()); });
}

int32_t gwamd_aligner_num_alignments(const gwamd_aligner* a) { return int32_t(a->impl->get_alignments().size()); }

int32_t gwamd_aligner_get_alignment(gwamd_aligner* a, int32_t i, int8_t* states, int32_t cap, int32_t* status)
{
    return guarded_aln([&] {
        const auto& al = a->impl->get_alignments();
        if (i < 0 || i >= int32_t(al.size()))
            throw std::invalid_argument("alignment index out of range");
        const auto& st = al[size_t(i)]->get_alignment();
        if (status)
            *status = int32_t(al[size_t(i)]->get_status());
        if (states && int32_t(st.size()) <= cap)
            for (size_t k = 0; k < st.size(); k++)
                states[k] = int8_t(st[k]);
        return int32_t(st.size());
    });
}

int32_t gwamd_aligner_get_sequences(gwamd_aligner* a, int32_t i, const char** q, int32_t* qlen, const char** t,
                                    int32_t* tlen)
{
    return guarded_aln([&] {
        const auto& al = a->impl->get_alignments();
        if (i < 0 || i >= int32_t(al.size()))
            throw std::invalid_argument("alignment index out of range");
        const std::string& qs = al[size_t(i)]->get_query_sequence();
        const std::string& ts = al[size_t(i)]->get_target_sequence();
        *q                    = qs.data();
        *qlen                 = int32_t(qs.size());
        *t                    = ts.data();
        *tlen                 = int32_t(ts.size());
        return int32_t(0);
    });
}

int32_t gwamd_aligner_get_cigar(gwamd_aligner* a, int32_t i, char* buf, int32_t cap)
{
    return guarded_aln([&] {
        const auto& al = a->impl->get_alignments();
        if (i < 0 || i >= int32_t(al.size()))
            throw std::invalid_argument("alignment index out of range");
        const std::string c = al[size_t(i)]->convert_to_cigar();
        if (buf && int32_t(c.size()) < cap)
            std::memcpy(buf, c.c_str(), c.size() + 1);
        return int32_t(c.size());
    });
}

void gwamd_aligner_reset(gwamd_aligner* a) { a->impl->reset(); }

int32_t gwamd_alignment_format(const char* query, int32_t query_length, const char* target, int32_t target_length,
                               const int8_t* states, int32_t num_states, int32_t maximal_line_length,
                               char* query_out, char* pairing_out, char* target_out, int32_t cap,
                               int32_t* linebreak_after)
{
    return guarded_aln([&] {
        ca::AlignmentImpl al(query, query_length, target, target_length);
        std::vector<ca::AlignmentState> st(size_t(std::max(num_states, 0)));
        for (int32_t k = 0; k < num_states; k++)
            st[size_t(k)] = static_cast<ca::AlignmentState>(states[k]);
        al.set_alignment(std::move(st));
        const ca::FormattedAlignment f = al.format_alignment(maximal_line_length);
        if (linebreak_after)
            *linebreak_after = f.linebreak_after;
        const int32_t n = int32_t(f.query.size());
        if (n < cap)
        {
            for (auto pr : {std::make_pair(query_out, &f.query), std::make_pair(pairing_out, &f.pairing),
                            std::make_pair(target_out, &f.target)})
                if (pr.first)
                    std::memcpy(pr.first, pr.second->c_str(), pr.second->size() + 1);
        }
        return n;
    });
}

int32_t gwamd_alignment_cigar(const int8_t* states, int32_t num_states, char* buf, int32_t cap)
{
    return guarded_aln([&] {
        ca::AlignmentImpl al("", 0, "", 0);
        std::vector<ca::AlignmentState> st(size_t(std::max(num_states, 0)));
        for (int32_t k = 0; k < num_states; k++)
            st[size_t(k)] = static_cast<ca::AlignmentState>(states[k]);
        al.set_alignment(std::move(st));
        const std::string c = al.convert_to_cigar();
        if (buf && int32_t(c.size()) < cap)
            std::memcpy(buf, c.c_str(), c.size() + 1);
        return int32_t(c.size());
    });
}

int32_t gwamd_aligner_upload(gwamd_aligner* a)
{
    return guarded_aln([&] {
        a->impl->upload();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_launch(gwamd_aligner* a)
{
    return guarded_aln([&] {
        a->impl->launch();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_download(gwamd_aligner* a)
{
    return guarded_aln([&] {
        a->impl->download();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_synchronize(gwamd_aligner* a)
{
    return guarded_aln([&] {
        a->impl->synchronize();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_get_paths(gwamd_aligner* a, const int8_t** paths, const int32_t** lengths, int32_t* stride)
{
    *paths   = a->impl->host_paths();
    *lengths = a->impl->host_path_lengths();
    *stride  = a->impl->max_result_length();
    return 0;
}

int32_t gwamd_aligner_get_config(const gwamd_aligner* a, int32_t* grid, int64_t* device_bytes)
{
    *grid         = a->impl->grid();
    *device_bytes = a->impl->device_bytes();
    return 0;
}

int32_t gwamd_aligner_last_kernel_ms(gwamd_aligner* a, double* ms)
{
    if (!a || !ms)
    {
        gwamd::host::last_error() = "gwamd_aligner_last_kernel_ms: null argument";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    return guarded_aln([&] {
        *ms = a->impl->last_kernel_ms();
        return int32_t(0);
    });
}

int32_t gwamd_aligner_get_stats(gwamd_aligner* a, int64_t* hbm_state_sweeps, int64_t* ukkonen_wide_pairs,
                                int64_t* ukkonen_max_rows_per_thread)
{
    if (!a || !hbm_state_sweeps || !ukkonen_wide_pairs || !ukkonen_max_rows_per_thread)
    {
        gwamd::host::last_error() = "gwamd_aligner_get_stats: null argument";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    return guarded_aln([&] {
        int64_t v[3];
        a->impl->path_stats(v);
        *hbm_state_sweeps            = v[0];
        *ukkonen_wide_pairs          = v[1];
        *ukkonen_max_rows_per_thread = v[2];
        return int32_t(0);
    });
}

int32_t gwamd_aligner_pair_fits(int32_t algorithm, int32_t max_query_length, int32_t max_target_length)
{
    if (algorithm < GWAMD_ALIGNER_HIRSCHBERG_MYERS || algorithm > GWAMD_ALIGNER_UKKONEN || max_query_length < 0 ||
        max_target_length < 0)
    {
        gwamd::host::last_error() = "gwamd_aligner_pair_fits: bad algorithm or negative length";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    return gwamd::aln::aligner_pair_fits(algorithm, max_query_length, max_target_length) ? 1 : 0;
}

int32_t gwamd_aligner_max_lengths(int32_t algorithm, int32_t* max_query, int32_t* max_target)
{
    if (max_query == nullptr || max_target == nullptr || algorithm < GWAMD_ALIGNER_HIRSCHBERG_MYERS ||
        algorithm > GWAMD_ALIGNER_UKKONEN)
    {
        gwamd::host::last_error() = "gwamd_aligner_max_lengths: bad algorithm or NULL output";
        return GWAMD_E_INVALID_ARGUMENT;
    }
    const gwamd::aln::AlignerLimits lim = gwamd::aln::aligner_limits(algorithm);
    *max_query                          = lim.max_query;
    *max_target                         = lim.max_target;
    return 0;
}

// Test hook (tests/test_aligner_plan.py): the plan an aligner of these
// capacities makes on a device of these facts, and one launch of it, without a
// device.  cus == 0 asks the current device for the facts, as the constructor
// does.  count, nslots and max_query_in_range below 1 stand for max_alignments,
// the planned slots and max_query_length.  Writes the values of
// gwamd_internal_aligner_plan_fields() in that order (the layout, the slots,
// the pipeline stages of max_alignments pairs, the launch, then kernel: 1 when
// the kernel table has the launch's kernel and the occupancy query's) and
// returns their count; negative when planning throws (gwamd_last_error says
// why) or `cap` is too small.
#define GWAMD_ARGS_FIELDS(F)                                                                                  \
    F(stride) F(max_path_length) F(max_query_length) F(max_matrix_elems) F(ws_slot_bytes) F(ws_front_off)     \
    F(front_cap) F(ws_leaf_off) F(leaf_cols) F(ws_split_off) F(ws_pat_off) F(ws_hbuf_off) F(ws_tcod_off)      \
    F(long_mode) F(stripe_blocks) F(lds_target_off) F(lds_pat_off) F(lds_scratch_off) F(lds_stack_off)       \
    F(lds_bytes) F(pat_words) F(scratch_bytes) F(lds_seq2_off) F(lds_tile_off) F(tile_bytes) F(ukkonen_p)     \
    F(uk_threads) F(lds_edge_off) F(band_waves) F(spec_phase) F(spec_sweeps)

const char* gwamd_internal_aligner_plan_fields(void)
{
#define GWAMD_F(f) #f ","
    return GWAMD_ARGS_FIELDS(GWAMD_F) "slot_bytes,fixed_bytes,uk_wide_lds,uk_wide,band_waves_forced,occ_long_mode,"
                                      "occ_band_waves,slots,resident,stages,launch_long_mode,launch_band_waves,"
                                      "launch_uk_threads,launch_lds_bytes,launch_lds_tile_off,launch_tile_bytes,"
                                      "launch_spec_sweeps,launch_grid0,launch_grid1,kernel";
#undef GWAMD_F
}

int32_t gwamd_internal_aligner_plan(int32_t algo, int32_t max_q, int32_t max_t, int32_t max_n, int32_t cus,
                                    int32_t per_cu, int32_t wide_per_cu, int64_t free_bytes, int32_t count,
                                    int32_t nslots, int32_t max_query_in_range, int32_t max_diff, int64_t* out,
                                    int32_t cap)
{
    return guarded_aln([&]() -> int32_t {
        namespace ga = gwamd::aln;
        if (algo < GWAMD_ALIGNER_HIRSCHBERG_MYERS || algo > GWAMD_ALIGNER_UKKONEN || max_q < 0 || max_t < 0 ||
            max_n < 1)
            throw std::invalid_argument("gwamd_internal_aligner_plan: bad algorithm or capacity");
        const ga::AlignerTuning tuning = ga::read_aligner_tuning();
        const ga::AlignerPlan p        = ga::plan_layout(algo, max_q, max_t, max_n, tuning);
        ga::DeviceFacts facts{cus, per_cu, wide_per_cu, free_bytes};
        if (cus == 0)
        {
            int dev = 0;
            GWAMD_HIP_CHECK(hipGetDevice(&dev));
            facts = device_facts(p, dev);
        }
        const ga::SlotPlan sp = ga::plan_slots(p, facts, max_n, tuning);
        const int stages      = ga::pipeline_stages(sp.slots, max_n, tuning);
        const ga::LaunchPlan l =
            ga::plan_launch(p, sp, count < 1 ? max_n : count, nslots < 1 ? sp.slots : nslots,
                            max_query_in_range < 1 ? max_q : max_query_in_range, max_diff);
        const bool found = gwamd_internal_aligner_kernel(&l.key).fn != nullptr &&
                           gwamd_internal_aligner_kernel(&p.occupancy_key).fn != nullptr;
#define GWAMD_F(f) int64_t(p.args.f),
        const int64_t v[] = {GWAMD_ARGS_FIELDS(GWAMD_F) p.slot_bytes, p.fixed_bytes, p.uk_wide_lds, p.uk_wide,
                             p.band_waves_forced, p.occupancy_key.long_mode, p.occupancy_key.band_waves, sp.slots,
                             sp.resident, stages, l.key.long_mode, l.band_waves, l.uk_threads, l.lds_bytes,
                             l.lds_tile_off, l.tile_bytes, l.spec_sweeps, l.grid[0], l.grid[1], found ? 1 : 0};
#undef GWAMD_F
        const int32_t n = int32_t(sizeof(v) / sizeof(v[0]));
        if (!out || cap < n)
            return -1;
        std::copy(v, v + n, out);
        return n;
    });
}
#undef GWAMD_ARGS_FIELDS

} // extern "C"
