// Test hooks of the POA device code: five single-workgroup kernels, each
// running one routine of poa_wave.hpp / poa_order.hpp / poa_rowprog.hpp on one
// graph given as the reference's fixed-slot arrays, behind C entry points for
// the tests and scripts/.  Not product code, and its own translation unit.
//
// Every hook has one shape: check the arguments (-2 before anything is sized
// or allocated from them), put the graph on the device (HookGraph), run one
// block (run_block), copy back.  A HIP error or any other exception is -1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_common.hpp"
#include "poa_wave.hpp"
#include "poa_order.hpp"
#include "poa_rowprog.hpp"

namespace
{
using namespace gwamd::poa;
using gwamd::host::DevBuf;

const gwamd::host::Budget kNoPool; // the hooks' device arrays are charged to no pool
constexpr int kLdsMax = 163840;    // LDS bytes of a workgroup

bool bad_threads(int threads, int most)
{
    return threads < 64 || threads > most || threads % 64;
}

// count entries of src as a device array of D (the C ABI's int32 ids narrowed to SizeT)
template <typename D, typename S>
DevBuf<D> to_device(const S* src, size_t count)
{
    DevBuf<D> d(count, kNoPool);
    std::vector<D> h(count);
    for (size_t i = 0; i < count; i++)
        h[i] = D(src[i]);
    GWAMD_HIP_CHECK(hipMemcpy(d.data(), h.data(), count * sizeof(D), hipMemcpyHostToDevice));
    return d;
}

// count entries of a device array into dst, widened
template <typename D, typename S>
void to_host(const S* dev, D* dst, size_t count)
{
    std::vector<S> h(count);
    GWAMD_HIP_CHECK(hipMemcpy(h.data(), dev, count * sizeof(S), hipMemcpyDeviceToHost));
    std::copy(h.begin(), h.end(), dst);
}

template <typename T>
DevBuf<T> device_filled(size_t count, int byte)
{
    DevBuf<T> d(count, kNoPool);
    GWAMD_HIP_CHECK(hipMemset(d.data(), byte, count * sizeof(T)));
    return d;
}

// One graph of n nodes as the hooks receive it: kMaxEdges / kMaxAlignments
// slots per node, node ids as int32.  A null array is not part of the graph.
struct HostGraph
{
    const uint8_t* base = nullptr;
    const uint16_t *in_cnt = nullptr, *out_cnt = nullptr, *aln_cnt = nullptr, *cov = nullptr, *in_w = nullptr;
    const int32_t *in_e = nullptr, *out_e = nullptr, *aln = nullptr, *sorted = nullptr, *pos = nullptr;
};

// The device copy of a HostGraph, owned, and the WinGraph bound to it.  sorted
// and pos always exist (uninitialised when not given): they are outputs too.
template <typename SizeT>
class HookGraph
{
public:
    HookGraph(int n, const HostGraph& h) : n_(size_t(n))
    {
        const size_t ne = n_ * kMaxEdges, na = n_ * kMaxAlignments;
        g.base      = put(base_, h.base, n_);
        g.in_cnt    = put(in_cnt_, h.in_cnt, n_);
        g.out_cnt   = put(out_cnt_, h.out_cnt, n_);
        g.aln_cnt   = put(aln_cnt_, h.aln_cnt, n_);
        g.cov       = put(cov_, h.cov, n_);
        g.in_w      = put(in_w_, h.in_w, ne);
        g.in_e      = put(in_e_, h.in_e, ne);
        g.out_e     = put(out_e_, h.out_e, ne);
        g.aln       = put(aln_, h.aln, na);
        g.sorted    = put(sorted_, h.sorted, n_, true);
        g.pos       = put(pos_, h.pos, n_, true);
        g.max_nodes = n;
    }
    // a per-node SizeT array of the device (g.sorted, g.pos or the caller's own):
    // set from narrowed host values, set bytewise, read back as int32
    void store(SizeT* dev, const std::vector<SizeT>& v) const
    {
        GWAMD_HIP_CHECK(hipMemcpy(dev, v.data(), n_ * sizeof(SizeT), hipMemcpyHostToDevice));
    }
    void fill(SizeT* dev, int byte) const { GWAMD_HIP_CHECK(hipMemset(dev, byte, n_ * sizeof(SizeT))); }
    void fetch(const SizeT* dev, int32_t* dst) const { to_host(dev, dst, n_); }

    WinGraph<SizeT> g{};

private:
    template <typename D, typename S>
    static D* put(DevBuf<D>& buf, const S* src, size_t count, bool always = false)
    {
        if (src)
            buf = to_device<D>(src, count);
        else if (always)
            buf.alloc(count, kNoPool);
        return buf.data();
    }
    size_t n_;
    DevBuf<uint8_t> base_;
    DevBuf<uint16_t> in_cnt_, out_cnt_, aln_cnt_, cov_, in_w_;
    DevBuf<SizeT> in_e_, out_e_, aln_, sorted_, pos_;
};

// one block of `threads` with lds_bytes of dynamic LDS, not waited for
template <typename... P, typename... A>
void enqueue_block(void (*kernel)(P...), int threads, size_t lds_bytes, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), lds_bytes, 0, args...);
}

// the same with the kernel's LDS limit raised first, checked and waited for
template <typename... P, typename... A>
void run_block(void (*kernel)(P...), int threads, size_t lds_bytes, A... args)
{
    GWAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes)));
    enqueue_block(kernel, threads, lds_bytes, args...);
    GWAMD_HIP_CHECK(hipGetLastError());
    GWAMD_HIP_CHECK(hipDeviceSynchronize());
}

// mean milliseconds of `reps` calls of once(), between two events on the null stream
template <typename F>
double mean_ms(int reps, F&& once)
{
    const gwamd::host::OwnedEvent e0, e1;
    GWAMD_HIP_CHECK(hipEventRecord(e0, 0));
    for (int k = 0; k < reps; k++)
        once();
    GWAMD_HIP_CHECK(hipEventRecord(e1, 0));
    float t = 0.f;
    GWAMD_HIP_CHECK(hipEventSynchronize(e1));
    GWAMD_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    return double(t) / reps;
}

// f() with every exception as the hooks' -1: a HIP call, a device allocation
// or an event that failed (host_common.hpp), or the host's own memory
template <typename F>
int guarded(F&& f) noexcept
try
{
    return f();
}
catch (...)
{
    return -1;
}
// the same around f(SizeT()), SizeT the node-id type of size_bits
template <typename F>
int guarded(int size_bits, F&& f) noexcept
{
    return guarded([&] { return size_bits == 16 ? f(int16_t()) : f(int32_t()); });
}

// the level-keyed Kahn sort (topsort_levels) of one graph by one workgroup,
// for the known-answer and random-DAG tests against the FIFO sort
template <typename SizeT>
__global__ void __launch_bounds__(1024) topsort_levels_test_kernel(WinGraph<SizeT> g, int n, int n_prev, int scratch,
                                                                   SizeT* hint, int n_hint, int* ok, uint64_t* prof)
{
    extern __shared__ __align__(16) uint8_t lds[];
#ifdef GWAMD_TOPSORT_PROFILE
    uint64_t p[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool r = topsort_levels<SizeT>(g, n, n_prev, (GWAMD_LDS uint8_t*)(lds), scratch, int(threadIdx.x),
                                         int(blockDim.x), hint, n_hint, p);
    if (threadIdx.x == 0 && prof)
        for (int k = 0; k < 10; k++)
            prof[k] += p[k];
#else
    const bool r = topsort_levels<SizeT>(g, n, n_prev, (GWAMD_LDS uint8_t*)(lds), scratch, int(threadIdx.x),
                                         int(blockDim.x), hint, n_hint);
    (void)prof;
#endif
    if (threadIdx.x == 0)
        *ok = r ? 1 : 0;
}

// order_splice_core on one order and one path by one workgroup.
// LDS: curr | key | cnt | stage (u16), kind (u8), one control word.
__global__ void __launch_bounds__(1024) order_splice_test_kernel(int16_t* sorted, int16_t* pos, int V, int L,
                                                                 const uint16_t* curr_g, const uint8_t* kind_g,
                                                                 int* out)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const int Lp             = (L + 8) & ~7;
    GWAMD_LDS uint8_t* a     = (GWAMD_LDS uint8_t*)(lds);
    GWAMD_LDS uint16_t* curr = (GWAMD_LDS uint16_t*)(a);
    GWAMD_LDS uint16_t* key  = curr + Lp;
    GWAMD_LDS uint16_t* cnt  = key + Lp;
    GWAMD_LDS uint16_t* stg  = cnt + ((V + 1 + L + 8) & ~7);
    GWAMD_LDS int* ctl       = (GWAMD_LDS int*)(stg + ((V + 8) & ~7));
    GWAMD_LDS uint8_t* kind  = (GWAMD_LDS uint8_t*)(ctl + 4);
    for (int i = int(threadIdx.x); i < L; i += int(blockDim.x))
    {
        curr[i] = curr_g[i];
        kind[i] = kind_g[i];
    }
    __syncthreads();
    const int r = order_splice_core<int16_t>(glb_of(sorted), glb_of(pos), V, L, curr, kind, key, cnt, stg, ctl,
                                             int(threadIdx.x), int(blockDim.x));
    if (threadIdx.x == 0)
        *out = r;
}

// The row program of one graph and order built by one wave
// (build_row_program_wave0) and then by every wave of the workgroup
// (build_row_program_args), each into cleared LDS, both copied out: records
// [V + 2] u32, then lists and sink words [xl_cap + kSinkWords] u16.
template <typename SizeT>
__global__ void __launch_bounds__(512) row_program_test_kernel(WinGraph<SizeT> g, int V, int xl_cap, int ring_rows,
                                                               uint32_t* rec_out, uint16_t* xl_out)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const int nrec   = V + 2, nxl = xl_cap + kSinkWords;
    uint32_t* rec    = reinterpret_cast<uint32_t*>(lds);
    uint16_t* xl     = reinterpret_cast<uint16_t*>(lds + ((4 * nrec + 15) & ~15));
    GWAMD_LDS uint8_t* flags = (GWAMD_LDS uint8_t*)(lds) + ((4 * nrec + 15) & ~15) + ((2 * nxl + 15) & ~15);
    GWAMD_LDS uint16_t* sinks = (GWAMD_LDS uint16_t*)(xl) + xl_cap;
    const int tid = int(threadIdx.x), nthr = int(blockDim.x);
    for (int which = 0; which < 2; which++)
    {
        for (int i = tid; i < nrec; i += nthr)
            rec[i] = 0;
        for (int i = tid; i < nxl; i += nthr)
            xl[i] = 0;
        __syncthreads();
        if (which == 0)
        {
            if (tid < kWave)
                build_row_program_wave0<SizeT>(g, V, rec, xl, xl_cap, ring_rows, tid, flags, sinks);
        }
        else
            build_row_program_args<SizeT>(g, V, rec, xl, xl_cap, ring_rows, tid, nthr, flags, sinks);
        __syncthreads();
        for (int i = tid; i < nrec; i += nthr)
            rec_out[which * nrec + i] = rec[i];
        for (int i = tid; i < nxl; i += nthr)
            xl_out[which * nxl + i] = xl[i];
        __syncthreads();
    }
}

// the racon DFS sort (topsort_racon_lds) of one graph by one wave, with the
// group heads in HBM (heads != nullptr: racon_dfs_csr) or the round-5 step
// (heads == nullptr)
template <typename SizeT>
__global__ void __launch_bounds__(64) topsort_racon_test_kernel(WinGraph<SizeT> g, int n, int scratch, int32_t* heads,
                                                               SizeT* mpos, int* out)
{
    extern __shared__ __align__(16) uint8_t lds[];
    // a static word first, as in the kernels: the dynamic scratch then does
    // not start at LDS address 0 (a null scratch pointer means "no scratch")
    __shared__ int keep[4];
    if (threadIdx.x < 4)
        keep[threadIdx.x] = n;
    __syncthreads();
    int cols     = 0;
    const bool r = topsort_racon_lds<SizeT>(g, n, (GWAMD_LDS uint8_t*)(lds), scratch, int(threadIdx.x), mpos, &cols,
                                            heads);
    if (threadIdx.x == 0)
    {
        out[0] = r && keep[3] == n ? 1 : 0;
        out[1] = cols;
    }
}

// the consensus of one graph by one wave, as finish_window runs it
// (consensus_window: the LDS path when the graph fits `scratch` bytes, else
// consensus_raw on lane 0)
template <typename SizeT>
__global__ void __launch_bounds__(64) consensus_test_kernel(WinGraph<SizeT> g, int n, int scratch, int force_hbm,
                                                           int32_t* cscore, SizeT* cpred, uint8_t* cons,
                                                           uint16_t* cov, int max_cons, int* out)
{
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ int sh[2];
    int len = 0, st = kSuccess;
    const int path = consensus_window<SizeT>(g, n, cscore, cpred, cons, cov, max_cons, (GWAMD_LDS uint8_t*)(lds),
                                             scratch, force_hbm != 0, int(threadIdx.x), sh[0], sh[1], len, st);
    if (threadIdx.x == 0)
    {
        if (len < max_cons)
            cons[len] = 0;
        out[0] = st;
        out[1] = len;
        out[2] = path;
    }
}

} // namespace

// Test hook (tests/test_poa_consensus.py): the consensus of one graph given as
// the reference's fixed-slot arrays (kMaxEdges / kMaxAlignments slots per
// node), by one wave with `scratch` bytes of LDS offered to the wave-wide path
// (consensus_lds); force_hbm keeps consensus_raw.  cons_out / cov_out hold
// max_cons entries and receive the consensus in host order.  Returns 1 when
// the LDS path ran, 0 for the HBM path, negative on a HIP error or bad
// arguments.
extern "C" int gwamd_internal_consensus(int size_bits, int n, const uint8_t* base, const int32_t* sorted,
                                        const int32_t* pos, const uint16_t* in_cnt, const int32_t* in_e,
                                        const uint16_t* in_w, const uint16_t* out_cnt, const int32_t* out_e,
                                        const uint16_t* aln_cnt, const int32_t* aln, const uint16_t* cov, int max_cons,
                                        int force_hbm, int scratch, int* status, int* len, uint8_t* cons_out,
                                        uint16_t* cov_out)
{
    return guarded(size_bits, [&](auto id) {
        using SizeT = decltype(id);
        if (n <= 0 || n > 32767 || max_cons <= 0 || scratch < 0 || scratch > kLdsMax - 64)
            return -2;
        const size_t mc = size_t(max_cons);
        const HookGraph<SizeT> G(n, {base, in_cnt, out_cnt, aln_cnt, cov, in_w, in_e, out_e, aln, sorted, pos});
        const DevBuf<uint8_t> d_cons  = device_filled<uint8_t>(mc + 1, 0);
        const DevBuf<uint16_t> d_ccov = device_filled<uint16_t>(mc + 1, 0);
        const DevBuf<SizeT> d_cpred(n, kNoPool);
        const DevBuf<int32_t> d_cscore(n, kNoPool);
        const DevBuf<int> d_out(3, kNoPool);
        // (at least one LDS word, so the kernel's dynamic array exists)
        run_block(&consensus_test_kernel<SizeT>, 64, std::max(scratch, 16), G.g, n, scratch, force_hbm,
                  d_cscore.data(), d_cpred.data(), d_cons.data(), d_ccov.data(), max_cons, d_out.data());
        int out[3] = {0, 0, 0};
        to_host(d_out.data(), out, 3);
        to_host(d_cons.data(), cons_out, mc);
        to_host(d_ccov.data(), cov_out, mc);
        *status = out[0];
        *len    = out[1];
        return out[2];
    });
}

// The fit rule of the wave-wide consensus: LDS bytes of the compact graph of
// n nodes and m in-edges, and whether it runs with `scratch` bytes offered.
extern "C" long long gwamd_internal_consensus_lds_bytes(int n, int m)
{
    return consensus_lds_bytes(n, m);
}
extern "C" int gwamd_internal_consensus_lds_fits(int n, int m, int scratch)
{
    return consensus_lds_fits(n, m, scratch) ? 1 : 0;
}

// Test hook (tests/test_poa_topsort.py, scripts/racon_bench.py): the racon
// DFS sort (cudapoa_topsort.cuh:94-189) of one graph given as fixed-slot
// in-edge and aligned-node arrays (kMaxEdges / kMaxAlignments slots), by one
// wave with `scratch` bytes of LDS; v1 selects the round-5 DFS step.  Writes
// the order, the MSA column of every node and the column count.  Returns 1
// when the LDS sort ran, 0 when it declined (the kernels then run the HBM
// sort), negative on a HIP error or bad arguments.  reps > 0: that many more
// sorts, *ms = the mean time per sort.
extern "C" int gwamd_internal_topsort_racon(int size_bits, int n, const uint16_t* in_cnt, const int32_t* in_e,
                                            const uint16_t* aln_cnt, const int32_t* aln, int scratch, int v1,
                                            int32_t* sorted, int32_t* mpos, int* ncols, int reps, double* ms)
{
    return guarded(size_bits, [&](auto id) {
        using SizeT = decltype(id);
        if (n <= 0 || n > 65535 || scratch < 0 || scratch > kLdsMax - 64)
            return -2;
        HostGraph h;
        h.in_cnt = in_cnt, h.in_e = in_e, h.aln_cnt = aln_cnt, h.aln = aln;
        const HookGraph<SizeT> G(n, h);
        G.fill(G.g.sorted, 0xff);
        const DevBuf<SizeT> d_mpos = device_filled<SizeT>(n, 0xff);
        const DevBuf<int32_t> d_heads(n, kNoPool);
        const DevBuf<int> d_out(2, kNoPool);
        int32_t* hp       = v1 ? nullptr : d_heads.data();
        const auto kernel = &topsort_racon_test_kernel<SizeT>;
        run_block(kernel, 64, scratch, G.g, n, scratch, hp, d_mpos.data(), d_out.data());
        int out[2] = {0, 0};
        to_host(d_out.data(), out, 2);
        if (reps > 0)
        {
            const double t = mean_ms(
                reps, [&] { enqueue_block(kernel, 64, scratch, G.g, n, scratch, hp, d_mpos.data(), d_out.data()); });
            if (ms)
                *ms = t;
        }
        G.fetch(G.g.sorted, sorted);
        if (mpos)
            G.fetch(d_mpos.data(), mpos);
        if (ncols)
            *ncols = out[1];
        return out[0];
    });
}

// Test hook (tests/test_poa_order_splice.py): the LDS kernel's row program of
// one graph (fixed-slot in-edge lists, base bytes, degrees) under the order
// `sorted` (a topological order of the n nodes), built by one wave and by
// every wave of a workgroup of `threads` threads.  rec_out: 2 x (n + 2) words,
// xl_out: 2 x (xl_cap + kSinkWords) entries (the one-wave build first).
// Returns 0, -1 on a HIP error, -2 on bad arguments.
extern "C" int gwamd_internal_row_program(int n, const uint8_t* base, const uint16_t* in_cnt, const uint16_t* out_cnt,
                                          const int32_t* in_e, const int32_t* sorted, int xl_cap, int ring_rows,
                                          int threads, uint32_t* rec_out, uint16_t* xl_out)
{
    return guarded([&] {
        if (n <= 0 || n > 8192 || xl_cap < 64 || xl_cap % 8 || bad_threads(threads, 512) || ring_rows < 1)
            return -2;
        std::vector<int32_t> po(n, -1);
        for (int q = 0; q < n; q++)
        {
            if (sorted[q] < 0 || sorted[q] >= n || po[sorted[q]] >= 0)
                return -2;
            po[sorted[q]] = q;
        }
        const int nrec = n + 2, nxl = xl_cap + kSinkWords;
        const int nblk = (n + kRowProgBlk - 1) / kRowProgBlk;
        const size_t lds_b = size_t((4 * nrec + 15) & ~15) + size_t((2 * nxl + 15) & ~15) +
                             size_t((n + 2 + 15) & ~15) + 4 * size_t(nblk) + 16;
        if (lds_b > size_t(kLdsMax))
            return -2;
        HostGraph h;
        h.base = base, h.in_cnt = in_cnt, h.out_cnt = out_cnt, h.in_e = in_e, h.sorted = sorted, h.pos = po.data();
        const HookGraph<int16_t> G(n, h);
        const DevBuf<uint32_t> d_rec(2 * nrec, kNoPool);
        const DevBuf<uint16_t> d_xl(2 * nxl, kNoPool);
        run_block(&row_program_test_kernel<int16_t>, threads, lds_b, G.g, n, xl_cap, ring_rows, d_rec.data(),
                  d_xl.data());
        to_host(d_rec.data(), rec_out, 2 * nrec);
        to_host(d_xl.data(), xl_out, 2 * nxl);
        return 0;
    });
}

// Test hook (tests/test_poa_order_splice.py): order_splice_core on the order
// sorted[0..V) (a permutation of 0..V-1) and the path curr / kind [L] by one
// workgroup of `threads` threads; n: the node count with the path's new
// nodes; sorted and pos come back with n entries.  Returns 0 spliced, 1 / 2
// declined (order check / no old node; nothing written), -1 on a HIP error,
// -2 on bad arguments.
extern "C" int gwamd_internal_order_splice(int V, int n, int L, int32_t* sorted, int32_t* pos, const int32_t* curr,
                                           const uint8_t* kind, int threads)
{
    return guarded([&] {
        if (V <= 0 || n < V || n > 32767 || L <= 0 || L > 32767 || bad_threads(threads, 1024))
            return -2;
        std::vector<int16_t> so(n, int16_t(-1)), po(n, int16_t(-1));
        for (int q = 0; q < V; q++)
        {
            if (sorted[q] < 0 || sorted[q] >= V || po[sorted[q]] >= 0)
                return -2;
            so[q]         = int16_t(sorted[q]);
            po[sorted[q]] = int16_t(q);
        }
        for (int i = 0; i < L; i++)
        {
            const bool isnew = (kind[i] & 3) >= 2;
            if (curr[i] < 0 || curr[i] >= n || (isnew != (curr[i] >= V)))
                return -2;
        }
        const size_t lds_b = 2 * (2 * size_t((L + 8) & ~7) + size_t((V + 1 + L + 8) & ~7) + size_t((V + 8) & ~7)) +
                             16 + size_t(L) + 16;
        if (lds_b > 65536)
            return -2;
        const DevBuf<int16_t> d_so = to_device<int16_t>(so.data(), n), d_po = to_device<int16_t>(po.data(), n);
        const DevBuf<uint16_t> d_cu = to_device<uint16_t>(curr, L);
        const DevBuf<uint8_t> d_ki  = to_device<uint8_t>(kind, L);
        const DevBuf<int> d_out(1, kNoPool);
        run_block(&order_splice_test_kernel, threads, lds_b, d_so.data(), d_po.data(), V, L, d_cu.data(),
                  d_ki.data(), d_out.data());
        int out = -1;
        to_host(d_out.data(), &out, 1);
        to_host(d_so.data(), sorted, n);
        to_host(d_po.data(), pos, n);
        return out;
    });
}

// Test hook (tests/test_poa_topsort.py): topsort_levels of one graph given as
// the reference's fixed-slot edge arrays (kMaxEdges slots per node), with the
// previous read's order of the first n_prev nodes (order_prev: a permutation
// of 0..n_prev-1, may be null when n_prev is 0) and critical-predecessor
// hints for the first n_hint nodes (hint may be null when n_hint is 0; it
// receives the final c(v)).  Returns 1 when the level sort produced sorted[],
// 0 when it declined (the kernels then run the FIFO sort), negative on a HIP
// error or bad arguments.
// Timing mode of the same hook (scripts/topsort_bench.py): after the checked
// run, `reps` more sorts; *ms gets the mean time per sort (HIP events around
// launches of one workgroup, copies of the previous order included) and
// prof[10] the section cycles, anchors and iterations of GWAMD_TOPSORT_PROFILE
// builds.
extern "C" int gwamd_internal_topsort_levels_timed(int size_bits, int n, int n_prev, int n_hint,
                                                   const uint16_t* in_cnt, const int32_t* in_e,
                                                   const uint16_t* out_cnt, const int32_t* out_e, int32_t* hint,
                                                   const int32_t* order_prev, int threads, int scratch,
                                                   int32_t* sorted, int reps, double* ms, uint64_t* prof)
{
    return guarded(size_bits, [&](auto id) {
        using SizeT = decltype(id);
        if (n <= 0 || bad_threads(threads, 1024) || scratch < 0 || scratch > kLdsMax || (n_hint > 0 && !hint) ||
            n_prev < 0 || n_prev > n || (n_prev > 0 && !order_prev))
            return -2;
        // the previous order: a permutation of the first n_prev nodes
        std::vector<SizeT> so(n, SizeT(0));
        std::vector<char> seen(n_prev, 0);
        for (int q = 0; q < n_prev; q++)
        {
            const int v = order_prev[q];
            if (v < 0 || v >= n_prev || seen[v])
                return -2;
            seen[v] = 1;
            so[q]   = SizeT(v);
        }
        HostGraph h;
        h.in_cnt = in_cnt, h.in_e = in_e, h.out_cnt = out_cnt, h.out_e = out_e;
        const HookGraph<SizeT> G(n, h);
        G.store(G.g.sorted, so);
        const DevBuf<SizeT> d_hint = hint ? to_device<SizeT>(hint, n) : device_filled<SizeT>(n, 0);
        const DevBuf<int> d_ok(1, kNoPool);
        const auto kernel = &topsort_levels_test_kernel<SizeT>;
        run_block(kernel, threads, scratch, G.g, n, n_prev, scratch, d_hint.data(), n_hint, d_ok.data(), nullptr);
        int ok = 0;
        to_host(d_ok.data(), &ok, 1);
        if (reps > 0)
        {
            // the same sort `reps` times (the graph, previous order and hints are
            // inputs only; the outputs are rewritten identically)
            const DevBuf<uint64_t> d_prof = device_filled<uint64_t>(10, 0);
            const double t = mean_ms(reps, [&] {
                G.store(G.g.sorted, so);
                enqueue_block(kernel, threads, scratch, G.g, n, n_prev, scratch, d_hint.data(), n_hint, d_ok.data(),
                              d_prof.data());
            });
            if (ms)
                *ms = t;
            if (prof)
                to_host(d_prof.data(), prof, 10);
        }
        G.fetch(G.g.sorted, sorted);
        if (hint)
            G.fetch(d_hint.data(), hint);
        return ok;
    });
}

extern "C" int gwamd_internal_topsort_levels(int size_bits, int n, int n_prev, int n_hint, const uint16_t* in_cnt,
                                             const int32_t* in_e, const uint16_t* out_cnt, const int32_t* out_e,
                                             int32_t* hint, const int32_t* order_prev, int threads, int scratch,
                                             int32_t* sorted)
{
    return gwamd_internal_topsort_levels_timed(size_bits, n, n_prev, n_hint, in_cnt, in_e, out_cnt, out_e, hint,
                                               order_prev, threads, scratch, sorted, 0, nullptr, nullptr);
}
