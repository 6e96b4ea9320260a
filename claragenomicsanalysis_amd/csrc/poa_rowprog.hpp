// The row program of the LDS-resident POA kernel (poa_kernels.hip): per
// topological row one 32-bit record {base, predecessor rows, sink / spill /
// general-path flags} and the predecessor lists, built in LDS once per read,
// so that the forward pass's row loop reads the graph from LDS alone.
// Device code, included by the kernels and by the test hooks (poa_hooks.hip).
#pragma once

#include "poa_wave.hpp"
#include "poa_order.hpp"

namespace gwamd
{
namespace poa
{

constexpr uint32_t kRecEscape = 63; // np field: predecessor rows read from the graph in HBM


struct RowProg
{
    const uint32_t* rec;
    const uint16_t* xl;
    int ring_mask;
};

// k-th predecessor row of row r (0 = the virtual row 0)
template <typename SizeT>
__device__ __forceinline__ int prog_pred(const RowProg& P, WinGraph<SizeT> g, int r, uint32_t rec, int k)
{
    g = as_global(g);
    const int np = (rec >> 8) & 63;
    if (np == 0)
        return 0; // source node: the virtual row 0
    if (np == 1)
        return r - int(rec >> 16);
    if (np == int(kRecEscape))
    {
        uint32_t t = uint32_t(pred_row(g, int(g.sorted[r - 1]), k));
        asm volatile("" : "+v"(t)); // wait here, not where the paths join
        return int(t);
    }
    return int(P.xl[(rec >> 16) + k]);
}

template <typename SizeT>
__device__ __forceinline__ int prog_np(WinGraph<SizeT> g, int r, uint32_t rec)
{
    g = as_global(g);
    const int np = (rec >> 8) & 63;
    return np == int(kRecEscape) ? int(g.in_cnt[int(g.sorted[r - 1])]) : np;
}

// Row program for rows 1..V (built after every topological sort).  The graph
// lives in HBM, so the loads are batched for memory-level parallelism: each
// lane takes kRP rows per pass and every dependent level (node, its counts,
// its first two predecessors' node ids, their rows) is issued for all of them
// before the next level waits.  A row spills when a successor reads it from
// ring_rows or more rows later; that is marked from the successor's side
// (row s, predecessor row p: s - p >= ring_rows) into byte flags in `flags`
// (V + 2 bytes of free LDS), so no out-edge lists are read.
// Sinks: the rows of the first kSinkCap sinks are left in sinks[0..), their
// number (all of them, capped at 65535) in sinks[kSinkCap], and every listed
// sink row spills, so that E(sink, L) can be read back after the forward pass
// (the tie check of a spliced row order, poa_order.hpp).
// The base of forward-pass row r from its record (build_row_program): bits
// 0-6, or the graph's own byte when they hold 0x7f, which stands for 0x7f and
// for every byte >= 0x80 (the reference compares whole bytes, and bit 7 of
// the record is the general-path flag)
template <typename SizeT>
__device__ __forceinline__ int row_base(WinGraph<SizeT> g, uint32_t rec, int r)
{
    const int b = int(rec & 0x7fu);
    return b == 0x7f ? uniform(int(g.base[g.sorted[r - 1]])) : b;
}

constexpr int kRowProgRP  = 4;                 // rows per lane and block
constexpr int kRowProgBlk = kRowProgRP * kWave;  // rows per block: one wave's pass

// One block of the row program: rows r0 .. r0 + kRowProgBlk - 1 (up to V) by
// one wave.  xbase / nsink: the predecessor-list entries and the sinks of the
// rows before r0 on entry, of the rows through this block on return.
template <typename SizeT>
__device__ __forceinline__ void row_program_block(WinGraph<SizeT> g, int V, uint32_t* rec, uint16_t* xl, int xl_cap,
                                                  int ring_rows, int lane, GWAMD_LDS uint8_t* flags,
                                                  GWAMD_LDS uint16_t* sinks, int r0, int& xbase, int& nsink)
{
    constexpr int kRP = kRowProgRP;
    {
        int node[kRP], np[kRP], base[kRP], oc[kRP], e0[kRP], e1[kRP], p0[kRP], p1[kRP];
#pragma unroll
        for (int u = 0; u < kRP; u++)
        {
            const int r = min(r0 + u * kWave + lane, V);
            node[u]     = int(g.sorted[r - 1]);
        }
#pragma unroll
        for (int u = 0; u < kRP; u++)
        {
            np[u]   = int(g.in_cnt[node[u]]);
            base[u] = int(g.base[node[u]]);
            oc[u]   = int(g.out_cnt[node[u]]);
            e0[u]   = int(g.in_e[node[u] * kMaxEdges]);
            e1[u]   = int(g.in_e[node[u] * kMaxEdges + 1]);
        }
#pragma unroll
        for (int u = 0; u < kRP; u++)
        {
            // slots beyond in_cnt hold stale ids: clamp to a valid node
            p0[u] = int(g.pos[np[u] >= 1 ? e0[u] : 0]) + 1;
            p1[u] = int(g.pos[np[u] >= 2 ? e1[u] : 0]) + 1;
        }
#pragma unroll
        for (int u = 0; u < kRP; u++)
        {
            const int r      = r0 + u * kWave + lane;
            const bool valid = r <= V;
            const int n      = valid ? np[u] : 0;
            int total        = 0;
            const int excl   = wave_excl_sum(n >= 2 ? n : 0, lane, total);
            {
                const bool sink   = valid && oc[u] == 0;
                const uint64_t sm = __builtin_amdgcn_ballot_w64(sink);
                const int si      = nsink + __popcll(sm & ((1ull << lane) - 1));
                if (sink && si < kSinkCap)
                {
                    sinks[si] = uint16_t(r);
                    flags[r]  = 1;
                }
                nsink += __popcll(sm);
            }
            if (valid)
            {
                // bits 0-6: the base, 0x7f standing for 0x7f and for every
                // byte >= 0x80 (the forward passes read such rows' base back
                // from the graph, row_base); bit 7: the forward pass must take
                // its general path (nw_forward_lds_v2): a source, a
                // predecessor beyond the ring, an escaped list or a base
                // other than ACGT
                const uint32_t ub = uint32_t(base[u]);
                uint32_t v        = (ub >= 0x7fu ? 0x7fu : ub) | (uint32_t(oc[u] == 0 ? 1 : 0) << 14);
                bool slow = n == 0 || !((ub & 0xc0u) == 0x40u && ((0x10008aull >> (ub & 0x3fu)) & 1u));
                if (n == 1)
                {
                    v |= (1u << 8) | (uint32_t(r - p0[u]) << 16);
                    if (r - p0[u] >= ring_rows)
                    {
                        flags[p0[u]] = 1;
                        slow         = true;
                    }
                }
                else if (n >= 2)
                {
                    const int off  = xbase + excl;
                    const bool fit = off + n <= xl_cap;
                    for (int k = 0; k < n; k++)
                    {
                        const int pk = k == 0 ? p0[u] : (k == 1 ? p1[u] : pred_row(g, node[u], k));
                        if (fit)
                            xl[off + k] = uint16_t(pk);
                        if (r - pk >= ring_rows)
                        {
                            flags[pk] = 1;
                            slow      = true;
                        }
                    }
                    v |= fit ? (uint32_t(n) << 8) | (uint32_t(off) << 16) : (kRecEscape << 8);
                    slow = slow || !fit;
                }
                rec[r] = v | (slow ? 0x80u : 0u);
            }
            xbase += total;
        }
    }
}

// The row program by one wave, block after block with a running list offset:
// the form the records, lists and marks are defined by.  Before a forward
// pass the kernel builds it on every wave (build_row_program below, byte for
// byte the same: tests/test_poa_order_splice.py compares the two); this one
// rebuilds it on the two rare paths that lose it to a sort's scratch (a sink
// tie that takes a Kahn sort, more sinks than the tie check holds).
template <typename SizeT>
__device__ void build_row_program_wave0(WinGraph<SizeT> g, int V, uint32_t* rec, uint16_t* xl, int xl_cap,
                                        int ring_rows, int lane, GWAMD_LDS uint8_t* flags,
                                        GWAMD_LDS uint16_t* sinks)
{
    g = as_global(g);
    for (int r = lane; r <= V + 1; r += kWave)
        flags[r] = 0;
    wave_sync();
    int xbase = 0;
    int nsink = 0;
    for (int r0 = 1; r0 <= V; r0 += kRowProgBlk)
        row_program_block<SizeT>(g, V, rec, xl, xl_cap, ring_rows, lane, flags, sinks, r0, xbase, nsink);
    if (lane == 0)
        sinks[kSinkCap] = uint16_t(min(nsink, 65535));
    wave_sync();
    for (int r = lane + 1; r <= V; r += kWave)
        if (flags[r])
            rec[r] |= 1u << 15;
    wave_sync();
}

// The row program on every wave of the workgroup (nthr threads, a multiple of
// kWave; called by all of them with uniform arguments): wave w takes blocks w,
// w + nwv, ...  A block's list offset and sink index depend on the blocks
// before it, so a first pass counts each block's list entries and sinks (node
// -> in- and out-degree, the loads of up to kCB blocks per wave in flight
// together) into one LDS word per block behind the flags, and a block then
// starts from the sum over the blocks before it.  Spill flags are plain LDS
// byte stores, as before; the bit-15 pass over them runs on every thread.
// flags: V + 2 bytes, then (V + kRowProgBlk - 1) / kRowProgBlk words at the
// next 16-byte boundary.  Workgroup barriers: 2 (after the counts, after the
// blocks); the caller's follows the last stores.
template <typename SizeT>
__device__ __forceinline__ void build_row_program_core(WinGraph<SizeT> g, int V, uint32_t* rec, uint16_t* xl,
                                                       int xl_cap, int ring_rows,
                                  int tid, int nthr, GWAMD_LDS uint8_t* flags, GWAMD_LDS uint16_t* sinks)
{
    g = as_global(g);
    constexpr int kRP = kRowProgRP, kCB = 4;
    const int lane = tid & (kWave - 1);
    const int wv   = uniform(tid / kWave);
    const int nwv  = nthr / kWave;
    const int nblk = (V + kRowProgBlk - 1) / kRowProgBlk;
    GWAMD_LDS int* blk = (GWAMD_LDS int*)(flags + ((V + 2 + 15) & ~15));
    for (int r = tid; r <= V + 1; r += nthr)
        flags[r] = 0;
    // per block: list entries | sinks << 20 (at most 256 x 50 and 256)
    for (int b0 = wv; b0 < nblk; b0 += nwv * kCB)
    {
        int node[kCB][kRP], ic[kCB][kRP], oc[kCB][kRP];
#pragma unroll
        for (int j = 0; j < kCB; j++)
#pragma unroll
            for (int u = 0; u < kRP; u++)
            {
                const int r = 1 + (b0 + j * nwv) * kRowProgBlk + u * kWave + lane;
                node[j][u]  = int(g.sorted[min(r, V) - 1]);
            }
#pragma unroll
        for (int j = 0; j < kCB; j++)
#pragma unroll
            for (int u = 0; u < kRP; u++)
            {
                ic[j][u] = int(g.in_cnt[node[j][u]]);
                oc[j][u] = int(g.out_cnt[node[j][u]]);
            }
#pragma unroll
        for (int j = 0; j < kCB; j++)
        {
            const int b = b0 + j * nwv;
            int c       = 0;
#pragma unroll
            for (int u = 0; u < kRP; u++)
            {
                const int r = 1 + b * kRowProgBlk + u * kWave + lane;
                if (b < nblk && r <= V)
                    c += (ic[j][u] >= 2 ? ic[j][u] : 0) + (oc[j][u] == 0 ? 1 << 20 : 0);
            }
            int total = 0;
            (void)wave_excl_sum(c, lane, total);
            if (lane == 0 && b < nblk)
                blk[b] = total;
        }
    }
    __syncthreads();
    int xbase = 0, nsink = 0, bnext = 0;
    for (int b = wv; b < nblk; b += nwv)
    {
        for (int q = bnext; q < b; q++)
        {
            const int c = uniform(blk[q]);
            xbase += c & 0xfffff;
            nsink += c >> 20;
        }
        bnext = b + 1; // (the block's own counts are added as it is built)
        row_program_block<SizeT>(g, V, rec, xl, xl_cap, ring_rows, lane, flags, sinks, 1 + b * kRowProgBlk, xbase,
                                 nsink);
    }
    if (tid == 0)
    {
        int ns = 0;
        for (int q = 0; q < nblk; q++)
            ns += blk[q] >> 20;
        sinks[kSinkCap] = uint16_t(min(ns, 65535));
    }
    __syncthreads();
    for (int r = tid + 1; r <= V; r += nthr)
        if (flags[r])
            rec[r] |= 1u << 15;
}

// build_row_program_core out of line with plain arguments, for the test
// kernel.  (Inlined into a kernel, ROCm 7.2.0's backend stops on this file
// with "Illegal instruction detected ... V_CMP_NE_U32_e32 0,
// $src_shared_base".)
template <typename SizeT>
__device__ __noinline__ void build_row_program_args(WinGraph<SizeT> g, int V, uint32_t* rec, uint16_t* xl, int xl_cap,
                                                    int ring_rows, int tid, int nthr, GWAMD_LDS uint8_t* flags,
                                                    GWAMD_LDS uint16_t* sinks)
{
    build_row_program_core<SizeT>(g, V, rec, xl, xl_cap, ring_rows, tid, nthr, flags, sinks);
}

// build_row_program_core for poa_window_kernel_lds: window w_ with V_ rows,
// `lds` the start of the LDS image; records, lists, sink words and flags at
// the offsets of Dims.  Called by every thread of the workgroup.  Out of
// line with the batch's pointers read from the kernel's own kernarg segment,
// as add_alignment_waves; kInst: one instantiation per calling kernel.  One
// call site per kernel: with this routine also at the two rebuilds after a
// sort (build_row_program_wave0 there), config B's kernel came out at 256
// VGPRs + 1 AGPR, one wave per SIMD and half the resident workgroups.
template <int NW, int kInst = 0>
__device__ __noinline__ void build_row_program(LdsKernelArgsPtr ka_, int w_, int V_, GWAMD_LDS uint8_t* lds)
{
    using SizeT               = int16_t;
    const LdsKernelArgsPtr ka = uniform_kernarg(ka_);
    lds                       = uniform_lds(lds);
    const WinGraph<SizeT> g   = bind_window<SizeT>(ka->b, ka->d.max_nodes, size_t(uniform(w_)));
    const int xcap            = ka->d.lds_xl_cap - kSinkWords;
    build_row_program_core<SizeT>(g, uniform(V_), (uint32_t*)(lds + ka->d.lds_rec_off),
                                  (uint16_t*)(lds + ka->d.lds_xl_off), xcap, ka->d.lds_ring_rows, int(threadIdx.x),
                                  NW * kWave, lds + ka->d.lds_ring_off,
                                  (GWAMD_LDS uint16_t*)(lds + ka->d.lds_xl_off) + xcap);
}

} // namespace poa
} // namespace gwamd
