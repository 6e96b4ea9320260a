// MI355X (gfx950) POA kernels: one POA window per 64-lane workgroup.
//
// Per window and per read s >= 1 (reference generatePOAKernel,
// cudapoa_kernels.cuh:66-359):
//   1. the read is staged in LDS;
//   2. the DP over the graph rows in topological order runs wave-parallel:
//      each lane owns 8 consecutive columns (one 16-B group of the score row),
//      the diagonal/vertical maxima over all predecessors are formed in
//      registers, and the horizontal gap closure is an exact max-prefix scan
//      across the wave (H[j] - j*gap is a running maximum), replacing the
//      reference's __any_sync fix-point loop (cudapoa_nw.cuh:265-310);
//   3. traceback, addAlignmentToGraph and the Kahn topological sort run on
//      lane 0 with the reference's tie order;
// then the heaviest-bundle consensus (or the racon sort + MSA) is generated in
// the same launch (reference runs them as separate kernels).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "poa_wave.hpp"
#include "poa_order.hpp"
#include "poa_rowprog.hpp" // the LDS kernel's row program (build_row_program)

namespace gwamd
{
namespace poa
{

// ---------------------------------------------------------------------------
template <typename ScoreT, typename SizeT, bool BANDED, bool MSA>
__global__ void __launch_bounds__(kWave) poa_window_kernel(Buffers b, Dims d, Scores sc)
{
    extern __shared__ __align__(16) uint8_t lds_read[];
    __shared__ int sh_alen;
    __shared__ int sh_status;
    __shared__ int sh_len;

    const int w = b.order ? b.order[blockIdx.x] : int(blockIdx.x);
    if (w >= b.num_windows)
        return;
    const int lane = threadIdx.x;

    const WinGraph<SizeT> g     = bind_window<SizeT>(b, d.max_nodes, size_t(w));
    const SlotScratch<SizeT> sl = bind_slot<SizeT>(b, d, size_t(w)); // one slot per window here
    const WinMsa<SizeT> msa     = bind_window_msa<SizeT, MSA>(b, d, size_t(w));
    ScoreT* S       = static_cast<ScoreT*>(b.scores) + size_t(w) * d.score_rows * size_t(d.score_stride);
    SizeT *ag = sl.ag, *ar = sl.ar, *cpred = sl.cpred, *seq_begin = msa.seq_begin;
    int32_t* cscore = sl.cscore;
    uint16_t *ecov = msa.ecov, *ecovc = msa.ecov_cnt;

    PhaseTimer ph;
    const WindowDesc wd = b.windows[w];
    const int nseq      = wd.num_seqs;
    int status          = kSuccess;
    int64_t cells       = 0;
    int node_count      = 0;

    if (nseq > 0)
    {
        const int len0 = b.seq_len[wd.first_seq];
        const uint8_t* seq0 = b.seqs + b.seq_off[wd.first_seq];
        const int8_t* w0    = b.wts + b.seq_off[wd.first_seq];
        build_backbone<SizeT, MSA>(g, seq0, w0, len0, lane, ecov, ecovc, seq_begin, d.max_seqs);
        node_count = len0;
        ph.lap<kPhBackbone>();
        for (int s = 1; s < nseq; s++)
        {
            if (node_count >= d.max_nodes) // cudapoa_kernels.cuh:222-227
            {
                status = kNodeCountExceeded;
                break;
            }
            const int L             = b.seq_len[wd.first_seq + s];
            const int64_t off       = b.seq_off[wd.first_seq + s];
            const uint8_t* read_g   = b.seqs + off;
            const int8_t* wts_g     = b.wts + off;
            // stage read in LDS (padded with zeros to a 16-B multiple)
            const int padded = (L + 16 + 15) & ~15;
            for (int j = lane; j < padded; j += kWave)
                lds_read[j] = j < L ? read_g[j] : 0;
            __syncthreads();
            const int V = node_count;
            int alen;
            if (BANDED)
            {
                Band B;
                B.bw         = d.band_width;
                B.stride     = d.band_width + kBandPad;
                B.max_column = L + 1;
                B.gradient   = float(L + 1) / float(V + 1);
                cells += int64_t(V + 1) * (d.band_width + kBandPad);
                nw_forward_banded<ScoreT, SizeT>(g, V, lds_read, L, S, B, sc, lane);
                __syncthreads();
                ph.lap<kPhForward>();
                if (lane == 0)
                    sh_alen = traceback_banded<ScoreT, SizeT>(g, V, lds_read, L, S, B, sc, ag, ar, d.aln_cap);
            }
            else
            {
                cells += int64_t(V + 1) * (L + 1);
                nw_forward_full<ScoreT, SizeT>(g, V, lds_read, L, S, d.score_stride, sc, lane);
                __syncthreads();
                ph.lap<kPhForward>();
                if (lane == 0)
                    sh_alen = traceback_full<ScoreT, SizeT>(g, V, lds_read, L, S, d.score_stride, sc, ag, ar,
                                                            d.aln_cap);
            }
            __syncthreads();
            ph.lap<kPhTraceback>();
            alen = sh_alen;
            if (alen == -1)
            {
                status = kLoopCountExceeded;
                break;
            }
            if (lane == 0)
            {
                int nc     = node_count;
                uint8_t rc = add_alignment<SizeT, MSA>(g, nc, ag, ar, alen, read_g, wts_g, s, ecov, ecovc, seq_begin,
                                                       d.max_seqs);
                ph.lap<kPhAdd>();
                rc = uniform(rc); // wave-uniform: the sort below runs scalar control flow
                nc = uniform(nc);
                if (rc == kSuccess)
                {
                    if (d.spoa_accurate) // cudapoa_kernels.cuh:324-337
                    {
                        if (!topsort_racon<SizeT>(g, nc, cscore, cpred, 4 * d.max_nodes))
                            rc = kGenericError;
                    }
                    else
                        topsort_kahn<SizeT>(g, nc, cscore);
                }
                ph.lap<kPhTopsort>();
                sh_status = rc;
                sh_len    = nc;
            }
            __syncthreads();
            status     = uniform(sh_status); // LDS values: tell the compiler they are wave-uniform
            node_count = uniform(sh_len);
            if (status != kSuccess)
                break;
        }
    }

    finish_window<SizeT, MSA>(b, d, w, lane, g, status, nseq, node_count, cscore, cpred, ecov, ecovc, seq_begin,
                              sh_len, sh_status);
    ph.lap<kPhOutput>();
    if (lane == 0)
    {
        if (b.phase)
            ph.store(b.phase + size_t(w) * kPhases);
        b.final_nodes[w] = node_count;
        b.cells[w]       = cells;
    }
}


// ===========================================================================
// LDS-resident kernel (full alignment, 16-bit scores and node ids).
//
// Differences from poa_window_kernel, same results:
//  * scores are kept in the E domain, E[i][j] = H[i][j] - j*gap, so the
//    horizontal gap closure is a plain prefix maximum and row 0 is all zeros;
//  * only the last kRing rows live in LDS (a ring); a row is also written to
//    HBM ("spilled") only if a later row reads it from farther back than the
//    ring (measured predecessor distances are <= 10 rows);
//  * instead of the score matrix the forward pass writes one traceback code
//    per cell (direction + predecessor slot, chosen with the reference's tie
//    order, cudapoa_nw.cuh:361-443), and the traceback walks those codes from
//    128x128 tiles staged in LDS;
//  * the per-read row program (base, predecessor rows, sink/spill flags) is
//    built in LDS once per read, so the row loop touches HBM only for the
//    code stores (poa_rowprog.hpp).
// ===========================================================================

// ---------------------------------------------------------------------------
// Packed 16-bit forward pass.  E values are int16, two cells per 32-bit
// register, so the diagonal/vertical/max work runs on v_pk_* instructions.
// The reference's rule for 16-bit scores (cudapoa_limits.hpp:28-37) bounds H,
// not E = H - j*gap: a read equal to its graph has E(j, j) = j * (match - gap).
// The host plans this pass only when the E range over the batch's columns
// fits int16 (lds_e_domain_fits16, poa_plan.cpp); a 16-bit batch past that
// bound runs the global-memory kernel.  Cells beyond the read may wrap; they
// only feed cells further right, never a cell <= L.
typedef short pk_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short pk_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pk_s16x2, a),
                                                                  __builtin_bit_cast(pk_s16x2, b)));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk_u16x2, a) + __builtin_bit_cast(pk_u16x2, b));
}
// min/mad against 0/1 constants are rewritten by the compiler into per-half
// compare + select sequences; the callers pass the constants through
// opaque_u32() so the packed forms survive.
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk_u16x2, a) - __builtin_bit_cast(pk_u16x2, b));
}
__device__ __forceinline__ uint32_t pk_min_u(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(pk_u16x2, a),
                                                                  __builtin_bit_cast(pk_u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_mad(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pk_u16x2, a) * __builtin_bit_cast(pk_u16x2, b) +
                                            __builtin_bit_cast(pk_u16x2, c));
}
__device__ __forceinline__ uint32_t opaque_u32(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ uint32_t pk_bcast(int v) { return (uint32_t(uint16_t(v)) * 0x10001u); }
// (lo, max(hi, lo)): one v_pk_max_i16 with op_sel_hi selecting src1's low half
__device__ __forceinline__ uint32_t pk_max_lo_into_hi(uint32_t a)
{
    const pk_s16x2 v = __builtin_bit_cast(pk_s16x2, a);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(v, __builtin_shufflevector(v, v, 0, 0)));
}
// max(a, (c.hi, c.hi)): the carry of the previous register pair, via op_sel
__device__ __forceinline__ uint32_t pk_max_hi_carry(uint32_t a, uint32_t c)
{
    const pk_s16x2 v = __builtin_bit_cast(pk_s16x2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pk_s16x2, a),
                                                                  __builtin_shufflevector(v, v, 1, 1)));
}

// Global loads on the rare far-predecessor paths are waited for inside their
// branch: a value still in flight where the paths join makes the compiler wait
// for vmcnt(0) on the common path too, i.e. for every code/spill store the
// wave has issued (HBM store latency on each row).
__device__ __forceinline__ void settle_vm1(uint32_t& v) { asm volatile("" : "+v"(v)); }
template <int NR>
__device__ __forceinline__ void settle_vm(uint32_t (&P)[NR], uint32_t& prev)
{
#pragma unroll
    for (int i = 0; i < NR; i++)
        settle_vm1(P[i]);
    settle_vm1(prev);
}

// loads the packed E values of predecessor row p (NR registers) and E_p[jb]
template <int NR>
__device__ __forceinline__ void load_pred_pk(const int16_t* ring, int ring_stride, int ring_mask, const int16_t* spill,
                                             int stride, int r, int p, int jb, uint32_t (&P)[NR], uint32_t& prev)
{
    const int16_t* lrow = ring + (p & ring_mask) * ring_stride + jb + kColShift;
#pragma unroll
    for (int q = 0; q < NR / 4; q++)
    {
        const uint4 v = *reinterpret_cast<const uint4*>(lrow + 1 + 8 * q);
        P[4 * q] = v.x, P[4 * q + 1] = v.y, P[4 * q + 2] = v.z, P[4 * q + 3] = v.w;
    }
    prev = uint32_t(uint16_t(lrow[0]));
    if (p == 0)
    {
#pragma unroll
        for (int i = 0; i < NR; i++)
            P[i] = 0;
        prev = 0;
    }
    else if (r - p > ring_mask)
    {
        const int16_t* grow = spill + size_t(p) * stride + jb + kColShift;
#pragma unroll
        for (int q = 0; q < NR / 4; q++)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(grow + 1 + 8 * q);
            P[4 * q] = v.x, P[4 * q + 1] = v.y, P[4 * q + 2] = v.z, P[4 * q + 3] = v.w;
        }
        prev = uint32_t(uint16_t(grow[0]));
        settle_vm<NR>(P, prev);
    }
}

// diagonal sources E_p[j-1] for the lane's cells: element 2i-1 and 2i
template <int NR>
__device__ __forceinline__ void diag_src(const uint32_t (&P)[NR], uint32_t prev, uint32_t (&Dg)[NR])
{
    Dg[0] = __builtin_amdgcn_alignbyte(P[0], prev << 16, 2);
#pragma unroll
    for (int i = 1; i < NR; i++)
        Dg[i] = __builtin_amdgcn_alignbyte(P[i], P[i - 1], 2);
}

// Diagnostic build only (-DGWAMD_FWD_PROFILE): shader-clock cycles of the
// forward pass sections, stored in place of the backbone/add/topsort/output
// phase slots.  With -DGWAMD_FWD_PROFILE_COUNTS as well the slots hold event
// counts instead (rows by kind, poll misses), and no clock is read.  The
// 16-bit scores take nw_forward_lds_v2 as in the default build
// (GWAMD_POA_FWD=v1: the round-3 pass); its sections are listed in
// scripts/gpu_fwdprof.sh.
#ifdef GWAMD_FWD_PROFILE
struct FwdProf
{
    uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t m    = 0;
#ifdef GWAMD_FWD_PROFILE_COUNTS
    __device__ void start() {}
    template <int I>
    __device__ void lap()
    {
    }
    template <int I>
    __device__ void count()
    {
        t[I] += 1;
    }
#elif defined(GWAMD_FWD_PROFILE_ONLY)
    // one section of nw_forward_lds_v2 timed (slot GWAMD_FWD_PROFILE_ONLY,
    // between its marks and its laps) and the whole row loop (slot 7): two
    // clock reads per timed section instead of one per lap
    uint64_t m0 = 0;
    __device__ void start() { m0 = __builtin_amdgcn_s_memtime(); }
    __device__ void stop() { t[7] += __builtin_amdgcn_s_memtime() - m0; }
    template <int I>
    __device__ void mark()
    {
        if (I == GWAMD_FWD_PROFILE_ONLY)
            m = __builtin_amdgcn_s_memtime();
    }
    template <int I>
    __device__ void lap()
    {
        if (I == GWAMD_FWD_PROFILE_ONLY)
            t[I] += __builtin_amdgcn_s_memtime() - m;
    }
    template <int I>
    __device__ void count()
    {
    }
#else
    __device__ void start() { m = __builtin_amdgcn_s_memtime(); }
    template <int I>
    __device__ void lap()
    {
        const uint64_t x = __builtin_amdgcn_s_memtime();
        t[I] += x - m;
        m = x;
    }
    template <int I>
    __device__ void count()
    {
    }
#endif
#ifndef GWAMD_FWD_PROFILE_ONLY
    __device__ void stop() {}
    template <int I>
    __device__ void mark()
    {
    }
#endif
};
#define GWAMD_FP_START(fp) fp.start()
#define GWAMD_FP_STOP(fp) fp.stop()
#define GWAMD_FP_MARK(fp, I) fp.template mark<I>()
#define GWAMD_FP_LAP(fp, I) fp.template lap<I>()
#define GWAMD_FP_COUNT(fp, I) fp.template count<I>()
#else
struct FwdProf
{
};
#define GWAMD_FP_START(fp)
#define GWAMD_FP_STOP(fp)
#define GWAMD_FP_MARK(fp, I)
#define GWAMD_FP_LAP(fp, I)
#define GWAMD_FP_COUNT(fp, I)
#endif

// Lane-parallel predecessor rows of row rr: lane k < n holds the row of
// predecessor slot k.  A source row gets the virtual row 0 as its single
// predecessor (n = 1, row 0), which gives the same column-0 value (gap) and
// the same scores as the reference's source-node case.
template <typename SizeT>
__device__ __forceinline__ int row_preds(const RowProg& P, WinGraph<SizeT> g, int rr, uint32_t rec, int lane,
                                         int& n)
{
    g = as_global(g);
    n      = int((rec >> 8) & 63);
    int pv = 0;
    if (n == int(kRecEscape))
    {
        const int node = uniform(int(g.sorted[rr - 1]));
        n              = uniform(int(g.in_cnt[node]));
        uint32_t t     = lane < n ? uint32_t(pred_row(g, node, lane)) : 0u;
        settle_vm1(t);
        pv = int(t);
    }
    else if (n >= 2)
        pv = lane < n ? int(P.xl[(rec >> 16) + lane]) : 0;
    else if (n == 1)
        pv = rr - int(rec >> 16);
    if (n == 0)
        n = 1;
    return pv;
}

// Forward pass of one read, split over NW waves of the workgroup: wave q owns
// the span of 64*CPL columns starting at cb = q*64*CPL (CPL cells per lane),
// and one sweep covers the read.  The waves are decoupled, not in lockstep:
// wave q needs from wave q-1 only the carry of each row (E_r[cb], the maximum
// over every column left of its span), which wave q-1 posts into a tagged
// LDS channel as soon as its row scan is done; wave q computes its own cells
// of the row before it waits for that word.  (This pass and nw_forward_lds_w:
// one word per row.  nw_forward_lds_v2 hands the carries over in blocks of
// kHandBlock rows, untagged, behind a head / tail pair in the same region, and
// keeps them in a register instead of `bnd`: poa_handover.hpp.)  The column-0 value of a row is
// the maximum of its predecessors' column-0 values, which lane 0 of wave 0
// loads anyway as the diagonal source of column 1.  The diagonal source of a
// span's first column for predecessor row p is the carry the wave received
// for row p (kept per wave in `bnd`, and in the spill row for far rows).
// The predecessor row r-1 (the common case in Kahn order) comes from
// registers; row r+1's predecessor list and row r+2's record are loaded while
// row r is computed.
template <int NR>
__device__ __forceinline__ void load_row_pk(const int16_t* p, uint32_t (&P)[NR], uint32_t& prev)
{
    if constexpr (NR % 4 == 0)
    {
#pragma unroll
        for (int q = 0; q < NR / 4; q++)
        {
            const uint4 v = *reinterpret_cast<const uint4*>(p + 1 + 8 * q);
            P[4 * q] = v.x, P[4 * q + 1] = v.y, P[4 * q + 2] = v.z, P[4 * q + 3] = v.w;
        }
    }
    else
    {
        static_assert(NR == 2, "4 or a multiple of 8 cells per lane");
        const uint2 v = *reinterpret_cast<const uint2*>(p + 1);
        P[0] = v.x, P[1] = v.y;
    }
    prev = uint32_t(uint16_t(p[0]));
}

template <int CPL, int NW, typename SizeT>
__device__ int nw_forward_lds_pk(WinGraph<SizeT> g, const RowProg& P, int V, const uint8_t* read, int L,
                                 int16_t* ring, int ring_stride, int16_t* spill, int stride, uint8_t* codes,
                                 int code_stride, const Scores sc, GWAMD_LDS uint8_t* shb, int16_t* carry_hbm,
                                 int tid, FwdProf& fp)
{
    g = as_global(g);
    constexpr int NR    = CPL / 2;
    constexpr int kSpan = kWave * CPL;
    const int lane      = tid & (kWave - 1);
    const int wave      = uniform(tid / kWave);
    V                   = uniform(V);
    L                   = uniform(L);
    const int gap       = sc.gap;
    const int s_eq      = sc.match - gap;
    const int s_ne      = sc.mismatch - gap;
    const uint32_t gap2 = pk_bcast(gap);
    const uint32_t one2 = opaque_u32(0x00010001u);
    const uint32_t two2 = opaque_u32(0x00020002u);
    // wave-uniform (an SGPR): P arrives through a flat pointer, and a value
    // first used inside the row loop made the compiler wait for vmcnt(0) --
    // every outstanding code / spill store -- at the top of every row
    const int mask      = uniform(P.ring_mask);
    GWAMD_LDS int* prog          = (GWAMD_LDS int*)(shb + kShProg);
    GWAMD_LDS int16_t* bnd       = (GWAMD_LDS int16_t*)(shb + kShBnd) + wave * (mask + 1);
    GWAMD_LDS uint32_t* chan     = (GWAMD_LDS uint32_t*)(shb + kShChan);
    volatile GWAMD_LDS uint32_t* chan_in  = chan + (wave - 1) * kChanRows; // wave > 0
    volatile GWAMD_LDS uint32_t* chan_out = chan + wave * kChanRows;       // wave < NW-1
    volatile GWAMD_LDS int* prog_v        = prog;
    // owner of the last column (L-1): span, lane, cell
    const int jl        = L > 0 ? L - 1 : 0;
    const int own_span  = jl / kSpan;
    const int own_lane  = (jl % kSpan) / CPL;
    const int own_c     = jl % CPL;
    const int nspan     = max(1, (L + kSpan - 1) / kSpan);
    const int nsweep    = (nspan + NW - 1) / NW;
    int best_row        = 0;
    int best_val        = INT_MIN;
    for (int sweep = 0; sweep < nsweep; sweep++)
    {
    if (sweep > 0)
    {
        // channels restart empty; the previous sweep's carries are in HBM
        __syncthreads();
        for (int t = tid; t < (kShChan - kShProg) / 4 + (NW - 1) * kChanRows; t += kWave * NW)
            reinterpret_cast<GWAMD_LDS int*>(shb + kShProg)[t] = 0;
        __syncthreads();
    }
    const int span      = sweep * NW + wave;
    const int cb        = span * kSpan;
    const bool first    = span == 0;                // holds column 0
    const bool wact     = cb < L || first;
    const bool feed     = wave + 1 < NW && cb + kSpan < L;  // next span, same sweep
    const bool to_hbm   = wave == NW - 1 && cb + kSpan < L; // next span, next sweep
    const bool from_hbm = wave == 0 && sweep > 0;
    const bool owner    = span == own_span;
    const int jb        = cb + lane * CPL;
    const bool active   = jb < L;
    const int ja        = active ? jb : 0; // address used by inactive lanes
    if (wact && V >= 1)
    {
        // per-read substitution profiles for A, C, G, T
        uint32_t sig_acgt[4][NR];
#pragma unroll
        for (int i = 0; i < NR; i++)
        {
            const int c0 = int(read[ja + 2 * i]), c1 = int(read[ja + 2 * i + 1]);
            const char bases[4] = {'A', 'C', 'G', 'T'};
#pragma unroll
            for (int b = 0; b < 4; b++)
                sig_acgt[b][i] = uint32_t(uint16_t(c0 == bases[b] ? s_eq : s_ne)) |
                                 (uint32_t(uint16_t(c1 == bases[b] ? s_eq : s_ne)) << 16);
        }
        uint32_t Eprev[NR]; // final E of row r-1 (row 0: zeros)
#pragma unroll
        for (int i = 0; i < NR; i++)
            Eprev[i] = 0;
        int cin_prev = 0;
        int hbm_c    = 0; // carries of 64 rows from the previous sweep, one per lane
        // software pipeline: predecessor rows of
        // rows r and r+1, records of rows r+1 and r+2; row r issues the loads
        // of row r+2's predecessors and row r+3's record
        uint32_t rec_c = uniform(int(P.rec[1]));
        uint32_t rec_a = uniform(int(P.rec[min(2, V)]));
        uint32_t rec_b = uniform(int(P.rec[min(3, V)]));
        int np_c, np_a = 1;
        int pv_c       = row_preds<SizeT>(P, g, 1, rec_c, lane, np_c);
        int pv_a       = V >= 2 ? row_preds<SizeT>(P, g, 2, rec_a, lane, np_a) : 0;
        uint8_t* crow  = codes + code_stride;
        int16_t* srow  = spill + stride;
        for (int r = 1; r <= V; r++, crow += code_stride, srow += stride)
        {
            GWAMD_FP_START(fp);
            int np_b = 1, pv_b = 0;
            if (r + 2 <= V)
                pv_b = row_preds<SizeT>(P, g, r + 2, rec_b, lane, np_b);
            const uint32_t rec_bb = P.rec[min(r + 3, V)];
            GWAMD_FP_LAP(fp, 4);

            const uint32_t rec = rec_c;
            const int np       = np_c;
            const int pv       = pv_c;
            const int base     = row_base<SizeT>(g, rec, r); // bit 7: general-path flag (build_row_program)
            const bool spill_r = (rec >> 15) & 1;
            int16_t* row       = ring + (r & mask) * ring_stride;
            const bool anyfar  = __builtin_amdgcn_ballot_w64(lane < np && pv != 0 && r - pv > mask) != 0;
            uint32_t sig[NR];
            // 'A' 'C' 'G' 'T' are bits 1, 3, 7, 20 of 0x40..0x7f; (base >> 1) & 3
            // gives A 0, C 1, T 2, G 3 (branch-free, a few scalar ops)
            const uint32_t ub = uint32_t(base);
            if ((ub & 0xc0u) == 0x40u && ((0x10008aull >> (ub & 0x3fu)) & 1u))
            {
                // bitwise selects (a select between the profile arrays would
                // index them dynamically, i.e. through scratch)
                const uint32_t bcode = (ub >> 1) & 3u;
                const uint32_t m1    = opaque_u32(((bcode ^ (bcode >> 1)) & 1u) ? ~0u : 0u); // C or T
                const uint32_t m2    = opaque_u32((bcode >> 1) ? ~0u : 0u);                  // G or T
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    const uint32_t lo = (sig_acgt[1][i] & m1) | (sig_acgt[0][i] & ~m1);
                    const uint32_t hi = (sig_acgt[3][i] & m1) | (sig_acgt[2][i] & ~m1);
                    sig[i]            = (hi & m2) | (lo & ~m2);
                }
            }
            else
            {
                const uint32_t* rw = reinterpret_cast<const uint32_t*>(read + ja);
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    const uint32_t wv = rw[i / 2] >> ((i & 1) * 16);
                    const int ch0 = int(wv & 0xff), ch1 = int((wv >> 8) & 0xff);
                    sig[i]        = uint32_t(uint16_t(ch0 == base ? s_eq : s_ne)) |
                             (uint32_t(uint16_t(ch1 == base ? s_eq : s_ne)) << 16);
                }
            }
            GWAMD_FP_LAP(fp, 5);
            // E values of predecessor row p for the lane's cells, and E_p[jb]
            auto load_pred = [&](int p, uint32_t(&Q)[NR], uint32_t& qprev) {
                if (p == r - 1)
                {
#pragma unroll
                    for (int i = 0; i < NR; i++)
                        Q[i] = Eprev[i];
                    qprev = uint32_t(__builtin_amdgcn_update_dpp(int(uint32_t(uint16_t(cin_prev))),
                                                                 int(Eprev[NR - 1] >> 16), 0x138, 0xf, 0xf, false));
                }
                else if (p == 0)
                {
#pragma unroll
                    for (int i = 0; i < NR; i++)
                        Q[i] = 0;
                    qprev = 0;
                }
                else if (anyfar && r - p > mask)
                {
                    load_row_pk<NR>(spill + size_t(p) * stride + ja + kColShift, Q, qprev);
                    settle_vm<NR>(Q, qprev);
                }
                else
                {
                    load_row_pk<NR>(ring + (p & mask) * ring_stride + ja + kColShift, Q, qprev);
                    {
                        const uint32_t bv = uint32_t(uint16_t(bnd[p & mask]));
                        if (lane == 0 && cb > 0)
                            qprev = bv;
                    }
                }
            };
            uint32_t dg[NR], vt[NR], kd[NR], kv[NR], E[NR];
            int c0v, c0kv = 0;
            {
                uint32_t Pv[NR], prev;
                load_pred(__builtin_amdgcn_readfirstlane(pv), Pv, prev);
                c0v = int(int16_t(prev)); // wave 0, lane 0: E_p[0]
                diag_src<NR>(Pv, prev, dg);
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    dg[i] = pk_add(dg[i], sig[i]);
                    vt[i] = pk_add(Pv[i], gap2);
                }
            }
            GWAMD_FP_LAP(fp, 6);
            // in-lane prefix maximum: per register pair max(diag, vertical),
            // then its low half into its high half, then the previous pair's
            // high half into both (op_sel forms, no shifts or permutes)
            auto prefix = [&]() {
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    const uint32_t s = pk_max_lo_into_hi(pk_max(dg[i], vt[i]));
                    E[i]             = i == 0 ? s : pk_max_hi_carry(s, E[i - 1]);
                }
            };
            if (np > 1)
            {
                // rows with several predecessors track the first maximising
                // slot of each cell, pre-scaled to the code layout: kd = 4 *
                // slot, kv = 4 * slot + 1 (codes: 0 diagonal, 1 vertical,
                // 2 horizontal, + slot << 2)
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    kd[i] = 0;
                    kv[i] = one2;
                }
                for (int k = 1; k < np; k++)
                {
                    uint32_t Q[NR], qprev, dq[NR];
                    load_pred(__builtin_amdgcn_readlane(pv, k), Q, qprev);
                    {
                        // column 0: first maximising predecessor slot
                        const int pe = int(int16_t(qprev));
                        c0kv         = pe > c0v ? k : c0kv;
                        c0v          = max(c0v, pe);
                    }
                    diag_src<NR>(Q, qprev, dq);
                    const uint32_t kk4 = pk_bcast(4 * k);
                    const uint32_t kk1 = pk_bcast(4 * k + 1);
#pragma unroll
                    for (int i = 0; i < NR; i++)
                    {
                        // running maxima with the first maximising predecessor slot
                        const uint32_t d  = pk_add(dq[i], sig[i]);
                        const uint32_t nd = pk_max(dg[i], d);
                        kd[i]             = pk_mad(pk_min_u(pk_sub(nd, dg[i]), one2), pk_sub(kk4, kd[i]), kd[i]);
                        dg[i]             = nd;
                        const uint32_t v  = pk_add(Q[i], gap2);
                        const uint32_t nv = pk_max(vt[i], v);
                        kv[i]             = pk_mad(pk_min_u(pk_sub(nv, vt[i]), one2), pk_sub(kk1, kv[i]), kv[i]);
                        vt[i]             = nv;
                    }
                }
                prefix();
            }
            else
                prefix();
            const int m    = active ? int(int16_t(E[NR - 1] >> 16)) : kNeg;
            GWAMD_FP_LAP(fp, 0);
            const int incl = wave_incl_max_dpp(m);
            const int excl = __builtin_amdgcn_update_dpp(kNeg, incl, 0x138, 0xf, 0xf, false);
            const int wtot = __builtin_amdgcn_readlane(incl, kWave - 1);
            int cin;
            if (first)
            {
                cin           = __builtin_amdgcn_readfirstlane(c0v) + gap; // column 0
                const int c0k = __builtin_amdgcn_readfirstlane(c0kv);
                if (lane == 0)
                {
                    row[kColShift]  = int16_t(cin);
                    crow[kColShift] = uint8_t(1 | (c0k << 2));
                    if (spill_r)
                        srow[kColShift] = int16_t(cin);
                }
            }
            else
            {
                if (from_hbm)
                {
                    // carry of this row from the previous sweep's last span
                    if (((r - 1) & (kWave - 1)) == 0)
                    {
                        const int x = r + lane;
                        uint32_t hc = x <= V ? uint32_t(int(carry_hbm[x])) : 0u;
                        settle_vm1(hc); // wait here, once per 64 rows, not at every row's readlane
                        hbm_c = int(hc);
                    }
                    cin = int(int16_t(__builtin_amdgcn_readlane(hbm_c, (r - 1) & (kWave - 1))));
                }
                else
                {
                    // carry of this row from the previous span
                    uint32_t w = uint32_t(uniform(int(chan_in[r & (kChanRows - 1)])));
                    while ((w >> 16) != (uint32_t(r) & 0xffffu))
                    {
                        __builtin_amdgcn_s_sleep(1);
                        w = uint32_t(uniform(int(chan_in[r & (kChanRows - 1)])));
                    }
                    cin = int(int16_t(w & 0xffffu));
                    if ((r & 7) == 0 && lane == 0)
                        prog_v[wave] = r;
                }
                if (lane == 0)
                {
                    bnd[r & mask] = int16_t(cin);
                    if (spill_r)
                        srow[cb + kColShift] = int16_t(cin); // same value as the previous span's last cell
                }
            }
            GWAMD_FP_LAP(fp, 1);
            if (feed)
            {
                // flow control: the consumer must have taken row r-kChanRows+32
                if ((r & 31) == 0 && r >= kChanRows)
                {
                    while (uniform(prog_v[wave + 1]) < r - 32)
                        __builtin_amdgcn_s_sleep(1);
                }
                if (lane == 0)
                    chan_out[r & (kChanRows - 1)] = (uint32_t(r) << 16) | uint32_t(uint16_t(max(cin, wtot)));
            }
            if (to_hbm && lane == 0)
                carry_hbm[r] = int16_t(max(cin, wtot));
            GWAMD_FP_LAP(fp, 2);
            const uint32_t b2v = pk_bcast(max(excl, cin));
#pragma unroll
            for (int i = 0; i < NR; i++)
                E[i] = pk_max(E[i], b2v);
            if (active)
            {
                // codes: 0 diagonal, 1 vertical, 2 horizontal (+ slot << 2)
                uint32_t code[NR];
                if (np > 1)
                {
#pragma unroll
                    for (int i = 0; i < NR; i++)
                    {
                        const uint32_t a   = pk_min_u(pk_sub(E[i], dg[i]), one2); // 0: diagonal match
                        const uint32_t bb  = pk_min_u(pk_sub(E[i], vt[i]), one2); // 0: vertical match
                        const uint32_t cvh = pk_mad(bb, pk_sub(two2, kv[i]), kv[i]); // vertical or horizontal
                        code[i]            = pk_mad(a, pk_sub(cvh, kd[i]), kd[i]);
                    }
                }
                else
                {
                    // one predecessor (slot 0): a * (1 + bb)
#pragma unroll
                    for (int i = 0; i < NR; i++)
                    {
                        const uint32_t a  = pk_min_u(pk_sub(E[i], dg[i]), one2);
                        const uint32_t bb = pk_min_u(pk_sub(E[i], vt[i]), one2);
                        code[i]           = pk_mad(a, bb, a);
                    }
                }
                if constexpr (NR % 4 == 0)
                {
#pragma unroll
                    for (int q = 0; q < NR / 4; q++)
                    {
                        const uint4 ev = make_uint4(E[4 * q], E[4 * q + 1], E[4 * q + 2], E[4 * q + 3]);
                        *reinterpret_cast<uint4*>(row + jb + kColShift + 1 + 8 * q) = ev;
                        if (spill_r)
                            *reinterpret_cast<uint4*>(srow + jb + kColShift + 1 + 8 * q) = ev;
                        const uint32_t w0 = __builtin_amdgcn_perm(code[4 * q + 1], code[4 * q], 0x06040200u);
                        const uint32_t w1 = __builtin_amdgcn_perm(code[4 * q + 3], code[4 * q + 2], 0x06040200u);
                        __builtin_nontemporal_store(uint64_t(w0) | (uint64_t(w1) << 32),
                                                    reinterpret_cast<uint64_t*>(crow + jb + kColShift + 1 + 8 * q));
                    }
                }
                else
                {
                    // 4 cells per lane: 8-byte E stores, one 4-byte code word
                    const uint2 ev = make_uint2(E[0], E[1]);
                    *reinterpret_cast<uint2*>(row + jb + kColShift + 1) = ev;
                    if (spill_r)
                        *reinterpret_cast<uint2*>(srow + jb + kColShift + 1) = ev;
                    __builtin_nontemporal_store(__builtin_amdgcn_perm(code[1], code[0], 0x06040200u),
                                                reinterpret_cast<uint32_t*>(crow + jb + kColShift + 1));
                }
            }
            if ((rec & (1u << 14)) && owner)
            {
                // sink row: E at the last column (column 0 for an empty read)
                int endv = cin;
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    if (2 * i == own_c)
                        endv = int(int16_t(E[i] & 0xffff));
                    if (2 * i + 1 == own_c)
                        endv = int(int16_t(E[i] >> 16));
                }
                const int v = L == 0 ? cin : __builtin_amdgcn_readlane(endv, own_lane);
                if (best_val < v)
                    best_val = v, best_row = r;
            }
#pragma unroll
            for (int i = 0; i < NR; i++)
                Eprev[i] = E[i];
            cin_prev = cin;
            rec_c    = rec_a;
            np_c     = np_a;
            pv_c     = pv_a;
            rec_a    = rec_b;
            np_a     = np_b;
            pv_a     = pv_b;
            rec_b    = uniform(int(rec_bb));
            GWAMD_FP_LAP(fp, 3);
        }
    }
    } // sweeps
    if (nsweep > 1 || NW > 1)
    {
        // publish the end row from the wave that owns the last column
        GWAMD_LDS int* endp = (GWAMD_LDS int*)(shb + kShEnd);
        if (wave == own_span % NW && lane == 0)
            *endp = best_row;
        __syncthreads();
        best_row = uniform(*endp);
    }
    return best_row;
}

// Traceback over the code matrix, run by one wave (lane-uniform walk; code
// tiles of 128 rows x 128 columns staged in LDS).  The tile code and the row
// record are loaded together, so a step waits for at most two LDS round trips
// (code/record, then a predecessor list).  Emitted pairs (node id or -1, read
// position or -1; reversed, as the reference's traceback,
// cudapoa_nw.cuh:361-452) are collected one per lane and stored 64 at a time;
// rows become node ids at the store.
template <typename SizeT>
__device__ int traceback_codes(WinGraph<SizeT> g, const RowProg& P, int V, int L, int end_row,
                               const uint8_t* codes_f, int code_stride, uint8_t* tile_f, SizeT* ag_f, SizeT* ar_f,
                               int aln_cap, int lane, bool rank, int tbmode)
{
    g = as_global(g);
    // typed pointers: this function is called, not inlined (lds_of)
    const GWAMD_GLB uint8_t* codes = glb_of(codes_f);
    GWAMD_LDS uint8_t* tile        = lds_of(tile_f);
    GWAMD_GLB SizeT* ag            = glb_of(ag_f);
    GWAMD_GLB SizeT* ar            = glb_of(ar_f);
    const GWAMD_LDS uint32_t* prec = lds_of(P.rec);
    const GWAMD_LDS uint16_t* pxl  = lds_of(P.xl);

    V       = uniform(V);
    L       = uniform(L);
    int i   = uniform(end_row), j = L;
    int ti0 = INT_MIN / 2, tj0 = INT_MIN / 2;
    int n = 0, loops = 0;
    const int bound = L + V + 2;
    int eg = 0, er = 0; // lane (n & 63) holds pair n until it is stored
    auto flush = [&](int upto) { tb_flush<SizeT>(g.sorted, ag, ar, aln_cap, upto, lane, eg, er); };
    auto load_tile = [&](int ii, int cj) {
        ti0 = max(0, ii - (kTileRows - 1));
        tj0 = max(0, cj - (kTileCols - 16)) & ~15;
        wave_sync();
        // 16 loads per lane, issued 8 at a time before any is waited for
        constexpr int kPer = kTileRows * (kTileCols / 16) / kWave;
        constexpr int kB   = 8;
#pragma unroll
        for (int b0 = 0; b0 < kPer; b0 += kB)
        {
            u32x4 v[kB];
#pragma unroll
            for (int u = 0; u < kB; u++)
            {
                const int t   = (b0 + u) * kWave + lane;
                const int tr  = t / (kTileCols / 16);
                const int tc  = (t % (kTileCols / 16)) * 16;
                const int rr  = ti0 + tr;
                const bool ok = rr <= V && tj0 + tc + 16 <= code_stride;
                v[u] = *reinterpret_cast<const GWAMD_GLB u32x4*>(codes + size_t(ok ? rr : 0) * code_stride +
                                                                 (ok ? tj0 + tc : 0));
                v[u] = ok ? v[u] : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < kB; u++)
            {
                const int t  = (b0 + u) * kWave + lane;
                const int tr = t / (kTileCols / 16);
                const int tc = (t % (kTileCols / 16)) * 16;
                *reinterpret_cast<GWAMD_LDS u32x4*>(tile + tr * kTileCols + tc) = v[u];
            }
        }
        wave_sync();
    };
    // Move window (TbWin, as in the banded traceback, poa_band.hip): the moves
    // of 128 cells decoded in one lane-parallel pass, two cells per lane,
    // packed (row << 16 | column), then walked.  Cells outside the tile or
    // with escaped predecessor lists are kSlow and take the general step.
    constexpr uint32_t kSlow = 0xffffffffu;
    const bool win_ok        = V < 65535 && L < 65535;
    TbWin G;
    G.init(tbmode, i, L, kTileRows);
    uint32_t wpk0 = kSlow, wpk1 = kSlow;
    auto decode_cell = [&](int t) -> uint32_t {
        const int r  = G.row(t);
        const int c  = G.col(t);
        const int cj = c + kColShift;
        uint32_t res = kSlow;
        if (r >= 1 && c >= 0 && r >= ti0 && r < ti0 + kTileRows && cj >= tj0 && cj < tj0 + kTileCols)
        {
            const int code     = int(tile[(r - ti0) * kTileCols + (cj - tj0)]);
            const uint32_t rec = prec[r];
            const int dir      = code & 3;
            const int np       = int((rec >> 8) & 63);
            const int pj       = dir == 1 ? c : c - 1;
            if (pj < 0)
                res = kSlow;
            else if (dir == 2)
                res = (uint32_t(r) << 16) | uint32_t(pj);
            else if (np != int(kRecEscape))
            {
                const int p = np == 0 ? 0 : (np == 1 ? r - int(rec >> 16) : int(pxl[(rec >> 16) + (code >> 2)]));
                res         = (uint32_t(p) << 16) | uint32_t(pj);
            }
        }
        return res;
    };
    while (!(i == 0 && j == 0) && loops < bound)
    {
        i     = uniform(i);
        j     = uniform(j);
        n     = uniform(n);
        loops = uniform(loops);
        ti0   = uniform(ti0);
        tj0   = uniform(tj0);
        G.wi0   = uniform(G.wi0);
        G.wj0   = uniform(G.wj0);
        G.slope = uniform(G.slope);
        G.next  = uniform(G.next);
        if (win_ok && i >= 1)
        {
            if (G.index(i, j) < 0)
            {
                G.refill(i, j);
                const int cj = j + kColShift;
                if (i < ti0 || i >= ti0 + kTileRows || cj < tj0 || cj >= tj0 + kTileCols ||
                    (i - G.row_span() < ti0 && ti0 > 0) || (cj - G.col_span() < tj0 && tj0 > 0))
                    load_tile(i, cj);
                wpk0  = decode_cell(lane);
                wpk1  = decode_cell(lane + kWave);
            }
            // walk the window: every value here is wave-uniform (SGPRs)
            int ci = i, cj = j, cn = n, cl = loops;
            if (rank)
                walk_window_ranked<0>(wpk0, wpk1, G, ci, cj, cn, cl, bound, lane, eg, er,
                                      tile + kTileRows * kTileCols, flush);
            else
                walk_window_scalar<0>(wpk0, wpk1, G, ci, cj, cn, cl, bound, lane, eg, er, nullptr, flush);
            if (cl != loops)
            {
                G.follow(ci, cj);
                i     = ci;
                j     = cj;
                n     = cn;
                loops = cl;
                continue;
            }
        }
        loops++;
        int pi, pj;
        if (i == 0)
        {
            pi = 0;
            pj = j - 1;
        }
        else
        {
            const int cj = j + kColShift;
            if (i < ti0 || i >= ti0 + kTileRows || cj < tj0 || cj >= tj0 + kTileCols)
                load_tile(i, cj);
            const int code_v   = int(tile[(i - ti0) * kTileCols + (cj - tj0)]);
            const int rec_v    = int(prec[i]);
            const int code     = uniform(code_v);
            const uint32_t rec = uint32_t(uniform(rec_v));
            const int dir      = code & 3;
            if (dir == 2)
            {
                pi = i;
                pj = j - 1;
            }
            else
            {
                const int np = int((rec >> 8) & 63), k = code >> 2;
                pi = np == 0 ? 0
                             : (np == 1 ? i - int(rec >> 16)
                                        : (np == int(kRecEscape) ? uniform(pred_row(g, int(g.sorted[i - 1]), k))
                                                                 : uniform(int(pxl[(rec >> 16) + k]))));
                pj = dir == 0 ? j - 1 : j;
            }
        }
        if (lane == (n & (kWave - 1)))
        {
            eg = i == pi ? -1 : i;
            er = j == pj ? -1 : j - 1;
        }
        n++;
        if ((n & (kWave - 1)) == 0)
            flush(n);
        i = pi;
        j = pj;
    }
    if ((n & (kWave - 1)) != 0)
        flush(n);
    wave_sync();
    if (loops >= bound || n > aln_cap)
        return -1;
    return n;
}

#include "poa_fwd2.hpp"
#include "poa_fwd_w.hpp"

// LDS-resident POA kernel: one workgroup of NW waves per window.  The forward
// pass, the graph update (add_alignment_waves) and the level-keyed
// topological sort use every wave; the serial phases (row program, traceback,
// consensus, MSA) run on wave 0 while the other waves wait at the next
// barrier.  W: 32-bit scores (nw_forward_lds_w, the reference's
// use32bitScore batches), else 16-bit.  Two waves per window
// (config B: four windows per CU, two waves per SIMD) need the kernel within
// 256 registers; it is (252 with the per-kernel level sort instance), and a
// second launch bound of 2 to force it costs config B 4% (the traceback
// phase 5.8 -> 8.1 ms per window, same traceback code), so it is not set.
template <bool MSA, int CPL, int NW, bool W>
__global__ void __launch_bounds__(kWave * NW, W ? (NW >= 8 ? 2 : 1) : (NW >= 4 ? 2 : 1))
    poa_window_kernel_lds(Buffers b, Dims d, Scores sc)
{
    using SizeT  = int16_t;
    using RowT   = typename std::conditional<W, int32_t, int16_t>::type; // E-domain row element
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ int sh_status;
    __shared__ int sh_len;

    __shared__ int sh_next;
    if (int(blockIdx.x) >= b.num_windows)
        return;
    const int tid      = threadIdx.x;
    const int lane     = tid & (kWave - 1);
    const int wave     = uniform(tid / kWave);
    constexpr int kThr = kWave * NW;
    const size_t slot  = blockIdx.x; // scratch slot (grid <= slots)

    uint8_t* lread   = lds;
    RowT* ring       = reinterpret_cast<RowT*>(lds + d.lds_ring_off);
    uint8_t* tile    = lds + d.lds_ring_off; // traceback tiles reuse the ring
    const int rstride = d.score_stride;      // ring / spill row stride (elements)
    GWAMD_LDS uint8_t* shb = (GWAMD_LDS uint8_t*)(lds) + d.lds_sh_off;
    // add-alignment scratch lives in the ring region (free between reads)
    const AddScratch AX = lds_add_scratch((GWAMD_LDS uint8_t*)(lds) + d.lds_ring_off, d.max_seq_len, d.max_nodes,
                                          false, (GWAMD_LDS int*)(shb));
    // graph update: 0 every wave (add_alignment_waves; when its scratch fits
    // the ring region), 1 wave 0 with one position per lane, 2 the sequential
    // restatement on lane 0 (kDiagAddWave0, kDiagAddSerial, GWAMD_POA_ADD)
    const bool add_fits = lds_add_fits(d.max_seq_len, d.max_nodes, d.lds_rec_off - d.lds_ring_off);
    const int add_mode  = (d.diag & kDiagAddSerial) ? 2 : (((d.diag & kDiagAddWave0) || !add_fits) ? 1 : 0);

    for (int idx = blockIdx.x; idx < b.num_windows;)
    {
    const int w     = b.order ? b.order[idx] : idx;
    const WinGraph<SizeT> g     = bind_window<SizeT>(b, d.max_nodes, size_t(w));
    const SlotScratch<SizeT> sl = bind_slot<SizeT>(b, d, slot);
    const WinMsa<SizeT> msa     = bind_window_msa<SizeT, MSA>(b, d, size_t(w));
    SizeT *ag = sl.ag, *ar = sl.ar, *cpred = sl.cpred, *seq_begin = msa.seq_begin;
    int32_t* cscore = sl.cscore;
    uint16_t *ecov = msa.ecov, *ecovc = msa.ecov_cnt;
    RowT* spill      = static_cast<RowT*>(b.scores) + slot * d.score_rows * size_t(rstride);
    uint8_t* codes   = b.codes + slot * size_t(d.aux_stride);
    uint32_t* rec    = reinterpret_cast<uint32_t*>(lds + d.lds_rec_off);
    uint16_t* xl     = reinterpret_cast<uint16_t*>(lds + d.lds_xl_off);
    RowT* carry      = reinterpret_cast<RowT*>(codes + d.aux_carry_off);
    RowProg P{rec, xl, d.lds_ring_rows - 1};

    PhaseTimer ph;
    FwdProf fp;
    // round-4 forward pass unless the scores do not fit its byte table (or
    // kDiagFwdV1, GWAMD_POA_FWD=v1 under GWAMD_DIAG, asks for round 3's)
    const bool use_v2 = !W && fwd2_ok(sc) && !(d.diag & kDiagFwdV1);
    const WindowDesc wd = b.windows[w];
    const int nseq      = wd.num_seqs;
    int status          = kSuccess;
    int64_t cells       = 0;
    int node_count      = 0;
    int lv_hint         = 0; // nodes whose critical predecessor of the last level sort is in cpred
    // Row order (poa_order.hpp).  order_kahn: g.sorted is the reference's Kahn
    // order (the backbone's is); else the previous order with the later reads
    // spliced in.  splice_on: this window still splices (not under the racon
    // order per read, the FIFO diagnostic or GWAMD_POA_ORDER=kahn; off for
    // good once it has had more than kSinkCap sinks).  Both are computed from
    // workgroup-uniform values on every thread.
    // tie_hold: reads still to be sorted, not spliced, after a tie between
    // sinks that took a Kahn sort to resolve.  Such ties persist (two ends that
    // no later read matches), and a window that kept splicing would pay the
    // splice, the tie sort and a second row program for every read; it sorts
    // per read instead, keeps watching for ties, and goes back to splicing
    // after two reads without one that needs a sort (a tie the out-list rule
    // settles does not extend the hold).  The 2 is not tuned.
    bool order_kahn = true;
    bool splice_on  = !d.spoa_accurate && !(d.diag & (kDiagTopsortFifo | kDiagOrderKahn));
    int tie_hold    = 0;
    const int sink_cap = (d.diag & kDiagSinkCap2) ? 2 : kSinkCap; // (the diagnostic value: tests of that path)
    const int xcap  = d.lds_xl_cap - kSinkWords; // predecessor lists; the sink list follows them
    GWAMD_LDS uint16_t* sinks = (GWAMD_LDS uint16_t*)(lds + d.lds_xl_off) + xcap;
    int32_t* ostat  = b.order_stats + size_t(w) * kOrderStats;
    auto count      = [&](int k) {
        if (tid == 0)
            __hip_atomic_fetch_add(ostat + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (tid < kOrderStats)
        ostat[tid] = 0;
    // A Kahn sort of the first n nodes into gx.sorted / gx.pos on every wave,
    // with the whole LDS image below the shared region as scratch (the staged
    // read and the row program are lost); lane 0's FIFO sort when the level
    // sort declines.  Barriers: the level sort's, then one.  gx.sorted[0 ..
    // n_prev) is only read as the order in which topsort_levels walks those
    // nodes: any permutation of the ids 0 .. n_prev - 1 will do (a walk in
    // topological order converges fastest), so a spliced order serves as a
    // Kahn order does, and a sort whose output goes elsewhere first copies the
    // order in use there.  cpred[0 .. lv_hint) holds c(v) of the window's last
    // level sort; reads spliced since then have not touched it, and every c(v)
    // is still a predecessor of v (edges are never removed), which is all a
    // hint has to be.
    auto kahn_sort = [&](WinGraph<SizeT> gx, int n, int n_prev) {
        const bool done = topsort_levels<SizeT, NW>(gx, n, n_prev, (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off, tid,
                                                    kThr, cpred, lv_hint);
        if (!done && tid == 0)
            topsort_kahn<SizeT>(gx, n, cscore);
        lv_hint = done ? n : 0;
        __syncthreads();
    };

    if (nseq > 0)
    {
        const int len0      = b.seq_len[wd.first_seq];
        const uint8_t* seq0 = b.seqs + b.seq_off[wd.first_seq];
        const int8_t* w0    = b.wts + b.seq_off[wd.first_seq];
        if (wave == 0)
            build_backbone<SizeT, MSA>(g, seq0, w0, len0, lane, ecov, ecovc, seq_begin, d.max_seqs);
        node_count = len0;
        ph.lap<kPhBackbone>();
        for (int s = 1; s < nseq; s++)
        {
            if (node_count >= d.max_nodes)
            {
                status = kNodeCountExceeded;
                break;
            }
            const int L           = b.seq_len[wd.first_seq + s];
            const int64_t off     = b.seq_off[wd.first_seq + s];
            const uint8_t* read_g = b.seqs + off;
            const int8_t* wts_g   = b.wts + off;
            const int padded      = (L + 32 + 15) & ~15;
            const int V           = node_count;
            // the read staged in LDS and the row program of the order in use,
            // on every wave (build_row_program's two barriers; the caller's
            // follows its last stores)
            auto stage_and_program = [&]() {
                for (int j = tid; j < padded; j += kThr)
                    lread[j] = j < L ? read_g[j] : 0;
                // (spill flags and block counts in the ring region, free until the forward pass)
                build_row_program<NW, NW + (W ? 16 : 0)>(lds_kernel_args(), w, V, (GWAMD_LDS uint8_t*)(lds));
            };
            // the same after a sort that used the LDS image as scratch, the
            // program by wave 0 (the same bytes; no barrier, the caller's
            // follows)
            auto stage_and_program_w0 = [&]() {
                for (int j = tid; j < padded; j += kThr)
                    lread[j] = j < L ? read_g[j] : 0;
                // (spill flags in the ring region, free until the forward pass)
                if (wave == 0)
                    build_row_program_wave0<SizeT>(g, V, rec, xl, xcap, d.lds_ring_rows, lane,
                                                   (GWAMD_LDS uint8_t*)(lds) + d.lds_ring_off, sinks);
            };
            stage_and_program();
            if (NW > 1)
            {
                // forward-pass channels and progress words start empty
                constexpr int kP = W ? kShProgW : kShProg;
                constexpr int kB = W ? kShBytesW(NW) : kShBytes(NW);
                for (int t = tid; t < (kB - kP) / 4; t += kThr)
                    reinterpret_cast<GWAMD_LDS int*>(shb + kP)[t] = 0;
            }
            __syncthreads();
            // sinks of the graph (uniform: an LDS word read after the barrier;
            // only looked at under a spliced order or while ties are watched)
            int nsink = (order_kahn && tie_hold == 0) ? 1 : uniform(int(sinks[kSinkCap]));
            if (nsink > sink_cap && order_kahn)
                nsink = 1;
            if (nsink > sink_cap)
            {
                // more sinks than the tie check lists: back to the Kahn order,
                // now and for the rest of the window.  Barriers, on every wave:
                // this one (the sort's scratch holds the sink count just read),
                // kahn_sort's, one more.
                __syncthreads();
                kahn_sort(g, V, V);
                count(kOsSortSinkCap);
                order_kahn = true;
                splice_on  = false;
                nsink      = 1;
                stage_and_program_w0();
                __syncthreads();
            }
            ph.lap<kPhRowProg>();
            cells += int64_t(V + 1) * (L + 1);
            int end_row;
            // (the diagnostic 24- and 32-column shapes keep the round-3 pass)
            if constexpr (W)
                end_row = nw_forward_lds_w<CPL, NW, SizeT>(g, P, V, lread, L, ring, rstride, spill, rstride, codes,
                                                           d.code_stride, sc, shb, carry, tid);
            else if constexpr (CPL <= 16)
                end_row = use_v2 ? nw_forward_lds_v2<CPL, NW, SizeT>(g, P, V, lread, L, ring, rstride, spill, rstride,
                                                                     codes, d.code_stride, sc, shb, carry, tid,
                                                                     d.lds_xl_cap, fp)
                                 : nw_forward_lds_pk<CPL, NW, SizeT>(g, P, V, lread, L, ring, rstride, spill, rstride,
                                                                     codes, d.code_stride, sc, shb, carry, tid, fp);
            else
                end_row = nw_forward_lds_pk<CPL, NW, SizeT>(g, P, V, lread, L, ring, rstride, spill, rstride, codes,
                                                            d.code_stride, sc, shb, carry, tid, fp);
            __syncthreads();
            ph.lap<kPhForward>();
            if (nsink >= 2)
            {
                // Several sinks, under a spliced order (or a Kahn order while
                // ties are watched): the forward pass took the first sink in row
                // order with the maximal final score, the reference the first in
                // Kahn order.  Every listed sink row was spilled, so E(sink, L)
                // is in its HBM row: wave 0 reads them, one sink per lane.
                //   One maximal sink: end_row stands.
                //   Several, each with one predecessor, the same one: the FIFO
                //     releases them together when it pops that node, in the
                //     order of its out-list, so the one in the lowest slot wins.
                //   Else a Kahn sort into the free part of the slot's cpred
                //     (topsort_levels keeps c(v) in its first max_nodes entries;
                //     the racon stack that fills it is not used on this path),
                //     and the tied sink with the smallest Kahn position wins.
                // Under a Kahn order end_row is right as it is, and only the
                // kind of tie is noted.  Barriers, on every wave: two here; for
                // a sort kahn_sort's, then two, then one after the read and the
                // row program (lost to the sort's scratch) are rebuilt.
                int srow_l = 0, sval = INT_MIN, smax = INT_MIN;
                bool tied  = false;
                if (wave == 0)
                {
                    if (lane < nsink)
                    {
                        srow_l = int(sinks[lane]);
                        sval   = int(glb(spill)[size_t(srow_l) * rstride + L + kColShift]);
                    }
                    smax              = wave_max(sval);
                    tied              = lane < nsink && sval == smax;
                    const uint64_t tm = __builtin_amdgcn_ballot_w64(tied);
                    int code = 0, er = end_row;
                    if (__popcll(tm) >= 2)
                    {
                        int node = 0, ic = 0, pr = -1;
                        if (tied)
                        {
                            node = int(glb(g.sorted)[srow_l - 1]);
                            ic   = int(glb(g.in_cnt)[node]);
                            pr   = ic == 1 ? int(glb(g.in_e)[node * kMaxEdges]) : -1;
                        }
                        const int p0 = __builtin_amdgcn_readlane(pr, uniform(__builtin_ctzll(tm)));
                        if (__builtin_amdgcn_ballot_w64(tied && (ic != 1 || pr != p0)) == 0)
                        {
                            int slot = INT_MAX;
                            if (tied)
                            {
                                const int oc = int(glb(g.out_cnt)[p0]);
                                for (int e = oc - 1; e >= 0; e--)
                                    if (int(glb(g.out_e)[p0 * kMaxEdges + e]) == node)
                                        slot = e;
                            }
                            const int smin = -wave_max(-slot);
                            const uint64_t m = __builtin_amdgcn_ballot_w64(tied && slot == smin);
                            er   = __builtin_amdgcn_readlane(srow_l, uniform(__builtin_ctzll(m)));
                            code = 1;
                        }
                        else
                            code = 2;
                    }
                    if (lane == 0)
                        sh_len = code | (er << 2);
                }
                __syncthreads();
                const int tv = uniform(sh_len);
                __syncthreads();
                const int code = tv & 3;
                if (code == 1 && !order_kahn)
                {
                    end_row = tv >> 2;
                    count(kOsTieQuick);
                }
                if (code == 2 && !order_kahn)
                {
                    const size_t mn    = size_t(d.max_nodes); // cpred: four arrays of max_nodes
                    WinGraph<SizeT> gk = g;
                    gk.sorted          = cpred + mn;
                    gk.pos             = cpred + 2 * mn;
                    for (int i = tid; i < V; i += kThr) // the order the sort walks the nodes in
                        glb(gk.sorted)[i] = glb(g.sorted)[i];
                    kahn_sort(gk, V, V);
                    count(kOsTieSorts);
                    if (wave == 0)
                    {
                        int kp = INT_MAX;
                        if (tied)
                            kp = int(glb(gk.pos)[int(glb(g.sorted)[srow_l - 1])]);
                        const int kmin = -wave_max(-kp);
                        const uint64_t m = __builtin_amdgcn_ballot_w64(kp == kmin);
                        const int er   = __builtin_amdgcn_readlane(srow_l, uniform(__builtin_ctzll(m)));
                        if (lane == 0)
                            sh_len = er;
                    }
                    __syncthreads();
                    end_row = uniform(sh_len);
                    __syncthreads();
                    stage_and_program_w0();
                    __syncthreads();
                }
                tie_hold = code == 2 ? 2 : max(tie_hold - 1, 0);
            }
            else if (tie_hold > 0)
                tie_hold--;
            if (wave == 0)
            {
                const int alen_w = traceback_codes<SizeT>(g, P, V, L, end_row, codes, d.code_stride, tile, ag, ar,
                                                          d.aln_cap, lane, (d.tb_rank & kTbRanked) != 0,
                                                          d.tb_rank);
                if (lane == 0)
                    sh_len = alen_w;
            }
            __syncthreads();
            const int alen = uniform(sh_len);
            __syncthreads();
            ph.lap<kPhTraceback>();
            if (alen == -1)
            {
                status = kLoopCountExceeded;
                break;
            }
            // Graph update.  Workgroup barriers of this step, the same on every
            // wave whatever the outcome (alen == -1 left the loop above on a
            // value every wave read after a barrier, before any of them):
            //   every-wave update: the barriers inside add_alignment_waves (8
            //     when positions conflict, 9 on a node or edge limit, 12 on
            //     success; each count is taken by the whole workgroup, see
            //     there), then the two below;
            //   conflict (0xff): lane 0 of wave 0 then runs the sequential
            //     restatement inside the wave-0 block, which holds no barrier;
            //     the other waves wait at the first of the two below;
            //   one-wave and serial modes: the two below only.
            // The status and node count go to the other waves through
            // sh_status / sh_len between those two barriers; an error status
            // (node limit included) leaves the read loop after the sort step's
            // own two barriers, again on every wave.
            int add_r = -1;
            if (add_mode == 0)
                add_r = add_alignment_waves<MSA, NW, NW + (W ? 16 : 0)>(lds_kernel_args(), w, int(slot), s, off,
                                                                        node_count, alen, L,
                                                                        (GWAMD_LDS uint8_t*)(lds));
            if (wave == 0)
            {
                int nc = node_count;
                int rc = -1;
                if (add_mode == 0)
                {
                    nc = add_r >> 8;
                    rc = (add_r & 0xff) == 0xff ? -1 : (add_r & 0xff);
                }
                else if (add_mode == 1)
                    rc = add_alignment_parallel<SizeT, MSA>(g, nc, ag, ar, alen, L, lread, wts_g, s, ecov, ecovc,
                                                            seq_begin, d.max_seqs, AX, lane);
                if (rc < 0)
                {
                    if (lane == 0)
                    {
                        sh_status = add_alignment<SizeT, MSA>(g, nc, ag, ar, alen, read_g, wts_g, s, ecov, ecovc,
                                                              seq_begin, d.max_seqs);
                        sh_len    = nc;
                    }
                    wave_sync();
                    rc = sh_status;
                    nc = sh_len;
                }
                ph.lap<kPhAdd>();
                if (lane == 0)
                {
                    sh_status = rc;
                    sh_len    = nc;
                }
            }
            __syncthreads();
            int rc       = uniform(sh_status);
            int nc       = uniform(sh_len);
            bool lv_done = false;
            __syncthreads(); // sh_* are rewritten below
            // Row order for the next read: the read's new nodes spliced into
            // the order in use (order_splice, poa_order.hpp) when the
            // every-wave update wrote the graph (its curr / kind arrays still
            // hold the path: nothing has touched the ring region since), the
            // next read is not empty (an empty read is aligned under a Kahn
            // order), this is not the window's last read (the consensus needs
            // Kahn ranks) and no tie between sinks is being waited out
            // (tie_hold); else, or when the splice declines, the full sort
            // below.  Barriers of order_splice, on every wave: 2 when it
            // declines or there is no new node, 4 when it writes; a spliced
            // read skips the sort step and its two barriers.
            int spl = -1;
            if (splice_on && rc == kSuccess)
            {
                const int l_next   = s + 1 < nseq ? b.seq_len[wd.first_seq + s + 1] : -1;
                const bool par_add = add_mode == 0 && uniform(add_r & 0xff) != 0xff;
                if (par_add && l_next > 0 && tie_hold == 0)
                    spl = uniform(order_splice<NW, NW + (W ? 16 : 0)>(lds_kernel_args(), w, V, L,
                                                                      (GWAMD_LDS uint8_t*)(lds)));
                count(spl == kSpliceDone ? kOsSpliced
                      : !par_add         ? kOsSortSeqAdd
                      : l_next < 0       ? kOsSortLast
                      : l_next == 0      ? kOsSortEmptyRead
                      : tie_hold > 0     ? kOsSortAfterTie
                      : spl == kSpliceCheck ? kOsSortCheck
                                            : kOsSortNoOld);
            }
            if (spl == kSpliceDone)
            {
                if (wave == 0)
                    ph.lap<kPhTopsort>();
                order_kahn = false;
                status     = rc;
                node_count = nc;
                continue;
            }
            order_kahn = true;
            // level-keyed Kahn sort on every wave of the workgroup
            // (GWAMD_TOPSORT=fifo, kDiagTopsortFifo, keeps the FIFO below)
            if (rc == kSuccess && !d.spoa_accurate && !(d.diag & kDiagTopsortFifo))
                lv_done = topsort_levels<SizeT, NW>(g, nc, V, (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off, tid, kThr,
                                                    cpred, lv_hint);
            lv_hint = lv_done ? nc : 0; // cpred holds c(v) of this sort for the next one
            if (wave == 0)
            {
                if (rc == kSuccess && !lv_done)
                {
                    if (d.spoa_accurate)
                        rc = topsort_racon_wave<SizeT>(g, nc, cscore, cpred, 4 * d.max_nodes, lane,
                                                       (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off);
                    // scratch: the read and the ring (both free after the add)
                    else if (!topsort_lds<SizeT>(g, nc, (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off, AX.sh, lane, nullptr,
                                                       (d.diag & kDiagTopsortRing) != 0) &&
                             !topsort_lds_big<SizeT>(g, nc, (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off, lane))
                    {
                        if (lane == 0)
                            topsort_kahn<SizeT>(g, nc, cscore);
                        wave_sync();
                    }
                }
                ph.lap<kPhTopsort>();
                wave_sync();
                if (lane == 0)
                {
                    sh_status = rc;
                    sh_len    = nc;
                }
            }
            __syncthreads();
            status     = uniform(sh_status); // LDS values: tell the compiler they are wave-uniform
            node_count = uniform(sh_len);
            __syncthreads(); // sh_* are rewritten by the next read
            if (status != kSuccess)
                break;
        }
    }
    if (wave == 0)
    {
        finish_window<SizeT, MSA, NW>(b, d, w, lane, g, status, nseq, node_count, cscore, cpred, ecov, ecovc,
                                      seq_begin, sh_len, sh_status, (GWAMD_LDS uint8_t*)(lds), d.lds_sh_off);
        ph.lap<kPhOutput>();
        if (lane == 0)
        {
            if (b.phase)
            {
                ph.store(b.phase + size_t(w) * kPhases);
#ifdef GWAMD_FWD_PROFILE
                // cycles / 1000 so the 100 MHz tick scaling reads as kcycles*1e-5
                const int slot[8] = {kPhBackbone, kPhAdd, kPhTopsort, kPhOutput, kPhForward, kPhTraceback, kPhRowProg,
                                     kPhTotal};
                for (int i = 0; i < 8; i++)
                    b.phase[size_t(w) * kPhases + slot[i]] = int64_t(fp.t[i]);
#endif
            }
            b.final_nodes[w] = node_count;
            b.cells[w]       = cells;
        }
    }
#if defined(GWAMD_FWD_PROFILE) && defined(GWAMD_FWD_PROFILE_WAVE)
    // diagnostic: another wave's section timers replace wave 0's
    __syncthreads();
    if (wave == GWAMD_FWD_PROFILE_WAVE && lane == 0 && b.phase)
    {
        const int slot[8] = {kPhBackbone, kPhAdd, kPhTopsort, kPhOutput, kPhForward, kPhTraceback, kPhRowProg,
                             kPhTotal};
        for (int i = 0; i < 8; i++)
            b.phase[size_t(w) * kPhases + slot[i]] = int64_t(fp.t[i]);
    }
#endif
    if (b.head == nullptr)
        break;
    // next queue position; the LDS image is rewritten by the next window
    __syncthreads();
    if (tid == 0)
        sh_next = b.num_slots + atomicAdd(b.head, 1);
    __syncthreads();
    idx = uniform(sh_next);
    }
}

} // namespace poa
} // namespace gwamd

// ---------------------------------------------------------------------------
// Kernel table and launch.  gwamd_internal_poa_kernel resolves a plan to its
// kernel; launch and occupancy are the same few steps over whatever it finds.
extern "C" gwamd::poa::KernelRef gwamd_internal_poa_band_kernel(const gwamd::poa::Dims* d, int score_bits,
                                                                int size_bits, int msa); // poa_band_dispatch.cpp

namespace
{
using namespace gwamd::poa;

// the LDS kernels, instantiated from kLdsShapes: {with, without} the MSA per shape
struct LdsPair
{
    const void* k[2];
};
template <size_t I>
LdsPair lds_kernels_at()
{
    constexpr LdsShape s = kLdsShapes[I];
    return {{reinterpret_cast<const void*>(&poa_window_kernel_lds<true, s.cpl, s.waves, s.wide>),
             reinterpret_cast<const void*>(&poa_window_kernel_lds<false, s.cpl, s.waves, s.wide>)}};
}
template <size_t... I>
const void* lds_kernel(int cpl, int waves, bool wide, bool msa, std::index_sequence<I...>)
{
    const LdsPair table[] = {lds_kernels_at<I>()...};
    for (int i = 0; i < kNumLdsShapes; i++)
        if (kLdsShapes[i].cpl == cpl && kLdsShapes[i].waves == waves && kLdsShapes[i].wide == wide)
            return table[i].k[msa ? 0 : 1];
    return nullptr;
}

// the v1 kernels: one workgroup of one wave per window, any score and size type
template <typename ScoreT, typename SizeT>
const void* v1_kernel(bool banded, bool msa)
{
    const void* k[] = {reinterpret_cast<const void*>(&poa_window_kernel<ScoreT, SizeT, true, true>),
                       reinterpret_cast<const void*>(&poa_window_kernel<ScoreT, SizeT, true, false>),
                       reinterpret_cast<const void*>(&poa_window_kernel<ScoreT, SizeT, false, true>),
                       reinterpret_cast<const void*>(&poa_window_kernel<ScoreT, SizeT, false, false>)};
    return k[(banded ? 0 : 2) + (msa ? 0 : 1)];
}

// above 64 KB of dynamic LDS a kernel has to be told so first
hipError_t prepare(const KernelRef& k)
{
    if (k.fn == nullptr)
        return hipErrorInvalidConfiguration;
    if (k.dynamic_lds <= 65536)
        return hipSuccess;
    return hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(k.dynamic_lds));
}
} // namespace

// The kernel of a planned Dims (fn == nullptr: none, the plan and the table
// disagree).  Taking a kernel's host handle needs no device.
extern "C" gwamd::poa::KernelRef gwamd_internal_poa_kernel(const gwamd::poa::Dims* d, int score_bits, int size_bits,
                                                           int banded, int msa)
{
    if (d->lds_kernel == 3)
        return banded ? gwamd_internal_poa_band_kernel(d, score_bits, size_bits, msa) : KernelRef{nullptr, 0, 0};
    if (d->lds_kernel == 1)
    {
        if (banded || size_bits != 16 || (score_bits != 16 && score_bits != 32))
            return {nullptr, 0, 0};
        return {lds_kernel(d->lds_cpl, d->lds_waves, score_bits == 32, msa != 0,
                           std::make_index_sequence<size_t(kNumLdsShapes)>()),
                kWave * d->lds_waves, size_t(d->lds_bytes)};
    }
    const int lds_bytes = (d->max_seq_len > d->band_width + kBandPad ? d->max_seq_len : d->band_width + kBandPad) + 32;
    const void* fn      = score_bits == 16   ? v1_kernel<int16_t, int16_t>(banded != 0, msa != 0)
                          : size_bits == 16 ? v1_kernel<int32_t, int16_t>(banded != 0, msa != 0)
                                            : v1_kernel<int32_t, int32_t>(banded != 0, msa != 0);
    return {fn, kWave, size_t((lds_bytes + 15) & ~15)};
}

// Workgroups of the planned LDS or banded kernel that are resident on one CU
// at once (the persistent grid is this times the CU count); 0 for the v1
// kernel, which runs one workgroup per window.
extern "C" int gwamd_internal_poa_blocks_per_cu(const gwamd::poa::Dims* d, int score_bits, int size_bits, int banded,
                                                int msa)
{
    if (!d->lds_kernel)
        return 0;
    const KernelRef k = gwamd_internal_poa_kernel(d, score_bits, size_bits, banded, msa);
    int n             = 0;
    if (prepare(k) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, k.threads, k.dynamic_lds) != hipSuccess)
        return 0;
    return n;
}

// Internal launch ABI used by the C++ batch (poa_batch.cpp): one workgroup per
// window, or the persistent grid of one per scratch slot.
extern "C" hipError_t gwamd_internal_poa_launch(const gwamd::poa::Buffers* b, const gwamd::poa::Dims* d,
                                       const gwamd::poa::Scores* sc, int score_bits, int size_bits, int banded,
                                       int msa, hipStream_t stream)
{
    if (b->num_windows <= 0)
        return hipSuccess;
    const KernelRef k = gwamd_internal_poa_kernel(d, score_bits, size_bits, banded, msa);
    if (const hipError_t e = prepare(k))
        return e;
    void* args[] = {const_cast<Buffers*>(b), const_cast<Dims*>(d), const_cast<Scores*>(sc)};
    return hipLaunchKernel(k.fn, dim3((d->lds_kernel && b->head) ? b->num_slots : b->num_windows), dim3(k.threads),
                           args, k.dynamic_lds, stream);
}
