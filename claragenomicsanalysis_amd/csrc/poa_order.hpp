// Row order of the full-alignment LDS kernel between two reads: the previous
// order with the read's new nodes spliced in, instead of a full Kahn sort.
//
// The forward recurrence, the traceback codes and the emitted alignment are
// the same under every topological row order (integer max over a node's
// predecessors; the code of a cell is a direction and a predecessor *slot*;
// the traceback emits node ids), and the host never sees the order.  The
// reference's Kahn order shows in two places only: which of several sinks
// with the same final score ends the alignment (the first in row order; the
// kernel resolves such a tie from the shared predecessor's out-list or with a
// Kahn sort into scratch, poa_window_kernel_lds), and the consensus (the
// window's last read is sorted, not spliced).
//
// One read's new nodes all lie on its path, and every new edge joins two
// consecutive path nodes.  The traceback only moves to lower rows, so the old
// nodes of the path are in increasing rank -- except that a base may land on
// an aligned sibling of the node it was aligned to, whose rank is unrelated;
// that is checked.  A valid order is then the old one with every run of new
// nodes placed directly behind the old path node before it (a leading run in
// front of the first old path node).
#pragma once

#include "poa_wave.hpp"

namespace gwamd
{
namespace poa
{

constexpr int kSinkCap   = 64; // sinks listed by the row program (one per lane of the tie check)
constexpr int kSinkWords = 72; // u16 words kept at the end of the predecessor-list region: the list, then the count

// order_splice_core returns
constexpr int kSpliceDone  = 0;
constexpr int kSpliceCheck = 1; // declined: old path nodes out of order; nothing written
constexpr int kSpliceNoOld = 2; // declined: no old node on the path; nothing written
constexpr int kSpliceLead  = 0xfffe; // key[] of a new node in front of the first old node (ranks are below 32768)

// inclusive max scan over the wave
__device__ __forceinline__ int wave_incl_max_shfl(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1)
    {
        const int t = __shfl_up(v, d, kWave);
        if (lane >= d)
            v = max(v, t);
    }
    return v;
}

// Splices the path of one read into sorted[0..V) / pos[]: curr[rp] is the node
// of read position rp, (kind[rp] & 3) >= 2 marks a new node.  Called by every
// thread of the workgroup (nthr threads, a multiple of kWave) with uniform
// arguments.  LDS scratch: key [L] u16, cnt [V + 1 + L] u16, stage [V] u16,
// ctl two ints.  Workgroup barriers: 2 when it declines or finds no new node,
// 4 when it writes.
template <typename SizeT>
__device__ __forceinline__ int order_splice_core(GWAMD_GLB SizeT* sorted, GWAMD_GLB SizeT* pos, int V, int L,
                                                 const GWAMD_LDS uint16_t* curr, const GWAMD_LDS uint8_t* kind,
                                                 GWAMD_LDS uint16_t* key, GWAMD_LDS uint16_t* cnt,
                                                 GWAMD_LDS uint16_t* stage, GWAMD_LDS int* ctl, int tid, int nthr)
{
    constexpr int kU = 8; // positions / ranks per thread whose HBM loads are issued together
    const int lane   = tid & (kWave - 1);
    // 1. rank of every old path node; run counters cleared
    for (int i = tid; i <= V; i += nthr)
        cnt[i] = 0;
    for (int r0 = tid; r0 < L; r0 += kU * nthr)
    {
        int nd[kU], rk[kU];
#pragma unroll
        for (int u = 0; u < kU; u++)
        {
            const int rp = r0 + u * nthr;
            nd[u]        = (rp < L && (kind[rp] & 3) < 2) ? int(curr[rp]) : -1;
        }
#pragma unroll
        for (int u = 0; u < kU; u++)
            rk[u] = nd[u] >= 0 ? int(pos[nd[u]]) : 0xffff;
#pragma unroll
        for (int u = 0; u < kU; u++)
            if (r0 + u * nthr < L)
                key[r0 + u * nthr] = uint16_t(rk[u]);
    }
    __syncthreads();
    // 2. wave 0, 64 positions at a time: the running maximum of (rank << 16 |
    // position) over the old nodes.  The nodes of a path are distinct, so the
    // old ranks increase along the path exactly when every old node is its own
    // running maximum, and the maximum before a new node is then its anchor:
    // the nearest old node before it.  A new node keeps anchor rank + 1 in
    // key[] and its index in the run in cnt[V + 1 + rp]; the last node of a
    // run leaves the run's length in cnt[anchor rank + 1].  A leading run goes
    // directly in front of the first old node, as if anchored one rank below
    // it (no run of the path has that anchor: the node there, if any, is not
    // on the path before the first old node, and later old nodes rank higher).
    if (tid < kWave)
    {
        int carry      = -1;
        int first_rank = -1, first_pos = 0; // the first old node of the path: its rank, its read position
        bool bad       = false;
        bool any_new   = false;
        for (int r0 = 0; r0 < L; r0 += kWave)
        {
            const int rp   = r0 + lane;
            const bool in  = rp < L;
            const int k    = in ? int(key[rp]) : 0xffff;
            const bool old = in && (kind[rp] & 3) < 2;
            const int v    = old ? ((k << 16) | rp) : -1;
            const int m    = max(wave_incl_max_shfl(v, lane), carry);
            const uint64_t om = __builtin_amdgcn_ballot_w64(old);
            if (carry < 0 && om != 0)
            {
                const int fl = uniform(__builtin_ctzll(om));
                first_rank   = __builtin_amdgcn_readlane(k, fl);
                first_pos    = r0 + fl;
            }
            carry = __builtin_amdgcn_readlane(m, kWave - 1);
            bad |= old && m != v;
            if (in && !old)
            {
                any_new = true;
                if (m < 0) // leading run: anchored in front of the first old node, once that is known
                {
                    key[rp]         = uint16_t(kSpliceLead);
                    cnt[V + 1 + rp] = uint16_t(rp);
                }
                else
                {
                    const int a1    = (m >> 16) + 1;
                    const int idx   = rp - (m & 0xffff) - 1;
                    key[rp]         = uint16_t(a1);
                    cnt[V + 1 + rp] = uint16_t(idx);
                    if (rp + 1 >= L || (kind[rp + 1] & 3) < 2)
                        cnt[a1] = uint16_t(idx + 1);
                }
            }
        }
        const bool wbad = __builtin_amdgcn_ballot_w64(bad) != 0;
        const bool wnew = __builtin_amdgcn_ballot_w64(any_new) != 0;
        if (lane == 0)
        {
            if (first_rank >= 0 && first_pos > 0)
                cnt[first_rank] = uint16_t(first_pos);
            ctl[0] = wbad ? kSpliceCheck : (carry < 0 ? kSpliceNoOld : (wnew ? kSpliceDone : 3));
            ctl[1] = first_rank;
        }
    }
    __syncthreads();
    const int dec  = uniform(ctl[0]);
    const int lead = uniform(ctl[1]); // anchor rank + 1 of a leading run: the rank of the first old node
    if (dec == kSpliceCheck || dec == kSpliceNoOld)
        return dec;
    if (dec == 3) // every base landed on an old node: the order stands
        return kSpliceDone;
    // 3. the old order staged in LDS (it is rewritten in place); wave 0 turns
    // the run lengths into an exclusive sum over anchor ranks
    for (int r0 = tid; r0 < V; r0 += kU * nthr)
    {
        int nd[kU];
#pragma unroll
        for (int u = 0; u < kU; u++)
            nd[u] = r0 + u * nthr < V ? int(sorted[r0 + u * nthr]) : 0;
#pragma unroll
        for (int u = 0; u < kU; u++)
            if (r0 + u * nthr < V)
                stage[r0 + u * nthr] = uint16_t(nd[u]);
    }
    if (tid < kWave)
    {
        int run = 0;
        for (int i0 = 0; i0 <= V; i0 += kWave)
        {
            const int i  = i0 + lane;
            const int c  = i <= V ? int(cnt[i]) : 0;
            int total    = 0;
            const int ex = wave_excl_sum(c, lane, total);
            if (i <= V)
                cnt[i] = uint16_t(run + ex);
            run += total;
        }
    }
    __syncthreads();
    // 4. old rank r moves up by the new nodes anchored below it; a new node
    // follows its anchor by 1 + its index in the run
    for (int r = tid; r < V; r += nthr)
    {
        const int nr = r + int(cnt[r + 1]);
        if (nr != r)
        {
            const int node = int(stage[r]);
            sorted[nr]     = SizeT(node);
            pos[node]      = SizeT(nr);
        }
    }
    for (int rp = tid; rp < L; rp += nthr)
        if ((kind[rp] & 3) >= 2)
        {
            const int kr   = int(key[rp]);
            const int a1   = kr == kSpliceLead ? lead : kr;
            const int nr   = a1 + int(cnt[V + 1 + rp]) + int(cnt[a1]);
            const int node = int(curr[rp]);
            sorted[nr]     = SizeT(node);
            pos[node]      = SizeT(nr);
        }
    __syncthreads();
    return kSpliceDone;
}

// order_splice_core for poa_window_kernel_lds, after a successful every-wave
// graph update (add_alignment_waves) and before anything reuses the ring
// region: curr / kind are the update's, key its gid array, cnt its owner
// array ([max_nodes + max_seq_len] >= V + 1 + L), ctl its control words, and
// the old order is staged in the row-program records (free after the
// traceback, 4 bytes per node).  Out of line with the batch's pointers read
// from the kernel's own kernarg segment, as add_alignment_waves and for the
// same reason; kInst: one instantiation per calling kernel.
template <int NW, int kInst = 0>
__device__ __noinline__ int order_splice(LdsKernelArgsPtr ka_, int w_, int V_, int L_, GWAMD_LDS uint8_t* lds)
{
    using SizeT               = int16_t;
    const LdsKernelArgsPtr ka = uniform_kernarg(ka_);
    const int mn              = ka->d.max_nodes;
    const int max_seq_len     = ka->d.max_seq_len;
    lds                       = uniform_lds(lds);
    const WinGraph<SizeT> g   = bind_window<SizeT>(ka->b, mn, size_t(uniform(w_)));
    const AddScratch X = lds_add_scratch(lds + int(lds_read_bytes(max_seq_len)), max_seq_len, mn, true, nullptr);
    return order_splice_core<SizeT>(glb_of(g.sorted), glb_of(g.pos), uniform(V_), uniform(L_), X.curr,
                                    X.kind, X.gid, X.owner, (GWAMD_LDS uint16_t*)(lds + ka->d.lds_rec_off), X.sh,
                                    int(threadIdx.x), NW * kWave);
}

} // namespace poa
} // namespace gwamd
