// Heaviest-bundle consensus of one finished window by the whole wave, on a
// compact copy of the graph in the workgroup's free LDS
// (cudapoa_generate_consensus.cuh:28-347; bit-identical to consensus_raw in
// poa_device.hpp, which stays as the path for graphs that do not fit).
//
// The copy is indexed by rank (position in the topological order), so the
// scoring loop walks it front to back and a predecessor is a smaller index:
//   rec[r]    u32  first in-edge of rank r (low 16 bits) | in-degree << 16
//   score[r]  i32  heaviest-path score (later reused as the path, u16)
//   edge[k]   u32  predecessor's rank (low 16 bits) | weight << 16, the
//                  in-edges of a rank in slot order
//   pred[r]   u16  rank of the chosen predecessor (kConsNoPred: none)
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "poa_device.hpp"

#ifndef GWAMD_LDS
#define GWAMD_LDS __attribute__((address_space(3)))
#endif
#ifndef GWAMD_GLB
#define GWAMD_GLB __attribute__((address_space(1)))
#endif

namespace gwamd
{
namespace poa
{

// LDS bytes of the compact graph of n nodes and m in-edges: the fit rule of
// the kernels (consensus_lds) and of the tests (gwamd_internal_consensus_lds_bytes)
__host__ __device__ constexpr int64_t consensus_lds_bytes(int64_t n, int64_t m)
{
    return 4 * n /* rec */ + 4 * n /* score */ + 4 * m /* edge */ + 2 * n /* pred */;
}
// ranks and edge offsets are 16-bit fields (0xffff: no predecessor)
__host__ __device__ constexpr bool consensus_lds_fits(int64_t n, int64_t m, int64_t scratch_bytes)
{
    return n > 0 && n <= 65535 && m >= 0 && m <= 65535 && consensus_lds_bytes(n, m) <= scratch_bytes;
}

constexpr int kConsNoPred  = 0xffff;
constexpr int kConsNoFit   = INT_MIN; // consensus_lds: the graph does not fit, nothing was written

__device__ __forceinline__ int wave_excl_sum(int v, int lane, int& total); // poa_wave.hpp

// A pointer argument of an out-of-line function arrives in vector registers;
// it is the same in every lane, so it is moved to scalar registers (the
// routine then stays within the registers a callee need not save).
template <typename T>
__device__ __forceinline__ GWAMD_GLB T* uniform_glb(T* p)
{
    const uint64_t v  = uint64_t(uintptr_t(p));
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))));
    return (GWAMD_GLB T*)(uintptr_t((uint64_t(hi) << 32) | lo));
}

// The scoring loop over ranks [r0, n) (cudapoa_generate_consensus.cuh:28-118
// with skip, :279-330 without): edges in slot order, an edge is taken if
// s < w || (s == w && score[pred] <= score[b]); the last maximal rank wins.
// skip: predecessors whose score is -1 are passed over (branch completion).
// Every lane runs the same loop on the same values; lane 0 stores.  The
// record two ranks ahead and the first four edge words of the next rank are
// loaded while this rank's scores are awaited (they do not depend on them),
// and an in-degree-1 rank whose predecessor is the rank before it takes that
// score from a register.
__device__ __forceinline__ void consensus_scan(GWAMD_LDS const uint32_t* rec, GWAMD_LDS const uint32_t* edge,
                                               GWAMD_LDS int32_t* score, GWAMD_LDS uint16_t* pred, int n, int m,
                                               int r0, bool skip, int lane, int& max_score, int& max_rank)
{
    if (r0 >= n)
        return;
    auto edge_at = [&](int k) -> uint32_t { return m > 0 ? edge[min(k, m - 1)] : 0u; };
    uint32_t rc  = uint32_t(uniform(int(rec[r0])));
    uint32_t rc1 = uint32_t(uniform(int(rec[min(r0 + 1, n - 1)])));
    uint32_t ew[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        ew[j] = edge_at(int(rc & 0xffffu) + j);
    int prev_s = 0; // score of rank r - 1 (r > r0)
    for (int r = r0; r < n; r++)
    {
        const int off = int(rc & 0xffffu), ic = int(rc >> 16);
        // ahead: rank r + 2's record, rank r + 1's first edges
        const uint32_t rc2v = rec[min(r + 2, n - 1)];
        uint32_t ewn[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            ewn[j] = edge_at(int(rc1 & 0xffffu) + j);
        int s = -1, p = kConsNoPred, ps = 0;
        for (int e0 = 0; e0 < ic; e0 += 4)
        {
            uint32_t cw[4];
            int sb[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                cw[j] = uint32_t(uniform(int(e0 == 0 ? ew[j] : edge_at(off + e0 + j))));
            if (ic == 1 && r > r0 && int(cw[0] & 0xffffu) == r - 1)
                sb[0] = prev_s, sb[1] = sb[2] = sb[3] = 0;
            else
            {
                int sv[4];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    sv[j] = score[e0 + j < ic ? int(cw[j] & 0xffffu) : 0];
#pragma unroll
                for (int j = 0; j < 4; j++)
                    sb[j] = uniform(sv[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                if (e0 + j >= ic || (skip && sb[j] == -1))
                    continue;
                const int w = int(cw[j] >> 16);
                if (s < w || (s == w && ps <= sb[j]))
                    s = w, p = int(cw[j] & 0xffffu), ps = sb[j];
            }
        }
        if (p != kConsNoPred)
            s += ps;
        if (max_score <= s)
            max_score = s, max_rank = r;
        if (lane == 0)
        {
            score[r] = s;
            pred[r]  = uint16_t(p);
        }
        wave_sync();
        prev_s = s;
        rc     = rc1;
        rc1    = uint32_t(uniform(int(rc2v)));
#pragma unroll
        for (int j = 0; j < 4; j++)
            ew[j] = ewn[j];
    }
}

// Consensus and coverage of the graph's n nodes into cons / cov in host order
// (first base first).  Returns the length, -status on an error of the
// reference (kLoopCountExceeded, kExceededMaxSeqSize; nothing is written), or
// kConsNoFit when the compact graph does not fit scratch_bytes (nothing is
// written; the caller runs consensus_raw).  All 64 lanes of one wave call it;
// the result is wave-uniform.
// Out of line, so that its registers are allocated apart from the calling
// kernel's (inlined, it changed the allocation of the LDS kernel's forward
// pass); the graph's pointers are retyped global here (they arrive flat).
// kInst: one instantiation per calling kernel family, as topsort_levels.
template <typename SizeT, int kInst = 0>
__device__ __noinline__ int consensus_lds_impl(const uint8_t* g_base, const uint16_t* g_in_cnt,
                                               const uint16_t* g_out_cnt, const uint16_t* g_aln_cnt,
                                               const uint16_t* g_cov, const uint16_t* g_in_w, const SizeT* g_in_e,
                                               const SizeT* g_out_e, const SizeT* g_aln, const SizeT* g_sorted,
                                               const SizeT* g_pos, int n, GWAMD_LDS uint8_t* scratch,
                                               int scratch_bytes, uint8_t* cons_, uint16_t* cov_, int max_cons)
{
    // (30 argument registers: a WinGraph by value would be passed on the
    // stack and add its 96 bytes to every calling kernel's scratch frame)
    const int lane                    = int(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
    GWAMD_GLB const uint8_t* base     = uniform_glb<const uint8_t>(g_base);
    GWAMD_GLB const uint16_t* in_cnt  = uniform_glb<const uint16_t>(g_in_cnt);
    GWAMD_GLB const uint16_t* out_cnt = uniform_glb<const uint16_t>(g_out_cnt);
    GWAMD_GLB const uint16_t* aln_cnt = uniform_glb<const uint16_t>(g_aln_cnt);
    GWAMD_GLB const uint16_t* ncov    = uniform_glb<const uint16_t>(g_cov);
    GWAMD_GLB const uint16_t* in_w    = uniform_glb<const uint16_t>(g_in_w);
    GWAMD_GLB const SizeT* in_e       = uniform_glb<const SizeT>(g_in_e);
    GWAMD_GLB const SizeT* out_e      = uniform_glb<const SizeT>(g_out_e);
    GWAMD_GLB const SizeT* aln        = uniform_glb<const SizeT>(g_aln);
    GWAMD_GLB const SizeT* sorted     = uniform_glb<const SizeT>(g_sorted);
    GWAMD_GLB const SizeT* pos        = uniform_glb<const SizeT>(g_pos);
    GWAMD_GLB uint8_t* cons           = uniform_glb<uint8_t>(cons_);
    GWAMD_GLB uint16_t* cov           = uniform_glb<uint16_t>(cov_);
    n             = uniform(n);
    scratch_bytes = uniform(scratch_bytes);
    max_cons      = uniform(max_cons);
    scratch       = (GWAMD_LDS uint8_t*)(uintptr_t)(uint32_t)uniform(int((uint32_t)(uintptr_t)scratch));
    if (n <= 0 || n > 65535)
        return kConsNoFit;
    // in-edge total (the counts by node id: coalesced)
    int m = 0;
    {
        int part = 0;
        for (int v0 = 0; v0 < n; v0 += 4 * kWave)
        {
            int c[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
            {
                const int v = v0 + u * kWave + lane;
                c[u]        = v < n ? int(in_cnt[v]) : 0;
            }
            part += c[0] + c[1] + c[2] + c[3];
        }
        (void)wave_excl_sum(part, lane, m);
    }
    if (!consensus_lds_fits(n, m, scratch_bytes))
        return kConsNoFit;
    GWAMD_LDS uint32_t* rec  = (GWAMD_LDS uint32_t*)(scratch);
    GWAMD_LDS int32_t* score = (GWAMD_LDS int32_t*)(scratch + 4 * n);
    GWAMD_LDS uint32_t* edge = (GWAMD_LDS uint32_t*)(scratch + 8 * n);
    GWAMD_LDS uint16_t* pred = (GWAMD_LDS uint16_t*)(scratch + 8 * n + 4 * m);

    // 1. stage: two 64-rank chunks per step, the first kPre in-edge slots of
    // every rank and their predecessors' ranks loaded together (one HBM round
    // trip per dependent level); longer lists one entry at a time
    {
        constexpr int kPre = 4, kU = 2;
        int ebase = 0;
        for (int r0 = 0; r0 < n; r0 += kU * kWave)
        {
            int node[kU], ic[kU], ie[kU][kPre], iw[kU][kPre], pr[kU][kPre];
#pragma unroll
            for (int u = 0; u < kU; u++)
            {
                const int r = r0 + u * kWave + lane;
                node[u]     = r < n ? int(sorted[r]) : 0;
            }
#pragma unroll
            for (int u = 0; u < kU; u++)
                ic[u] = r0 + u * kWave + lane < n ? int(in_cnt[node[u]]) : 0;
#pragma unroll
            for (int u = 0; u < kU; u++)
#pragma unroll
                for (int j = 0; j < kPre; j++)
                {
                    ie[u][j] = j < ic[u] ? int(in_e[node[u] * kMaxEdges + j]) : 0;
                    iw[u][j] = j < ic[u] ? int(in_w[node[u] * kMaxEdges + j]) : 0;
                }
#pragma unroll
            for (int u = 0; u < kU; u++)
#pragma unroll
                for (int j = 0; j < kPre; j++)
                    pr[u][j] = j < ic[u] ? int(pos[ie[u][j]]) : 0;
#pragma unroll
            for (int u = 0; u < kU; u++)
            {
                const int r   = r0 + u * kWave + lane;
                int total     = 0;
                const int off = ebase + wave_excl_sum(ic[u], lane, total);
                ebase += total;
                if (r < n)
                    rec[r] = uint32_t(off) | (uint32_t(ic[u]) << 16);
#pragma unroll
                for (int j = 0; j < kPre; j++)
                    if (j < ic[u] && off + j < m) // (off + ic <= m when sorted[] is a permutation)
                        edge[off + j] = uint32_t(pr[u][j] & 0xffff) | (uint32_t(iw[u][j]) << 16);
                for (int e = kPre; e < ic[u] && off + e < m; e++)
                {
                    const int b  = int(in_e[node[u] * kMaxEdges + e]);
                    const int w  = int(in_w[node[u] * kMaxEdges + e]);
                    edge[off + e] = uint32_t(int(pos[b]) & 0xffff) | (uint32_t(w) << 16);
                }
            }
        }
    }
    wave_sync();

    // 2. score.  The reference starts from max_id = 0 (node 0), max_score = -1;
    // every score is >= -1, so rank 0 already replaces it
    const int rank_of_0 = uniform(int(pos[0]) & 0xffff);
    int max_score = -1, max_rank = rank_of_0;
    consensus_scan(rec, edge, score, pred, n, m, 0, false, lane, max_score, max_rank);

    // 3. branch completion (cudapoa_generate_consensus.cuh:28-118, 332-347):
    // while the best node has out-edges, the other predecessors of its
    // successors are marked -1 and the ranks above it rescored without them
    int loops = 0;
    int oc    = uniform(int(out_cnt[uniform(int(sorted[max_rank]))]));
    while (oc != 0 && loops < n)
    {
        const int node = uniform(int(sorted[max_rank]));
        for (int l = lane; l < oc; l += kWave)
        {
            const int o       = int(out_e[node * kMaxEdges + l]);
            const uint32_t rw = rec[int(pos[o]) & 0xffff];
            const int off = int(rw & 0xffffu), ic = int(rw >> 16);
            for (int e = 0; e < ic; e++)
            {
                const int b = int(edge[off + e] & 0xffffu);
                if (b != max_rank)
                    score[b] = -1;
            }
        }
        wave_sync();
        int ms = 0, mr = rank_of_0; // (max_id = 0, max_score = 0 there)
        consensus_scan(rec, edge, score, pred, n, m, max_rank + 1, true, lane, ms, mr);
        max_rank = mr;
        loops++;
        oc = uniform(int(out_cnt[uniform(int(sorted[max_rank]))]));
    }
    if (loops >= n)
        return -int(kLoopCountExceeded);

    // 4. emit: the path from the best rank down its predecessors (the score
    // array is free and holds it), then one consensus position per lane
    GWAMD_LDS uint16_t* path = (GWAMD_LDS uint16_t*)(score);
    int count = 0, cur = max_rank;
    while (true)
    {
        const int p = uniform(int(pred[cur]));
        if (lane == 0)
            path[count] = uint16_t(cur);
        if (p == kConsNoPred)
            break;
        cur = p;
        count++;
        if (count >= max_cons - 1)
            return -int(kExceededMaxSeqSize);
        if (count >= n) // (a predecessor's rank is below its successor's: cannot happen)
            return -int(kGenericError);
    }
    if (count >= max_cons - 1) // (max_cons <= 1)
        return -int(kExceededMaxSeqSize);
    wave_sync();
    const int len = count + 1;
    constexpr int kE = 4, kPreA = 2;
    for (int k0 = 0; k0 < len; k0 += kE * kWave)
    {
        int node[kE], ac[kE], c[kE], al[kE][kPreA];
        uint8_t bs[kE];
#pragma unroll
        for (int u = 0; u < kE; u++)
        {
            const int k = k0 + u * kWave + lane;
            node[u]     = k < len ? int(path[k]) : -1;
        }
#pragma unroll
        for (int u = 0; u < kE; u++)
            node[u] = node[u] >= 0 ? int(sorted[node[u]]) : -1;
#pragma unroll
        for (int u = 0; u < kE; u++)
        {
            const bool in = node[u] >= 0;
            bs[u]         = in ? base[node[u]] : uint8_t(0);
            c[u]          = in ? int(ncov[node[u]]) : 0;
            ac[u]         = in ? int(aln_cnt[node[u]]) : 0;
#pragma unroll
            for (int a = 0; a < kPreA; a++)
                al[u][a] = (in && a < ac[u]) ? int(aln[node[u] * kMaxAlignments + a]) : -1;
        }
#pragma unroll
        for (int u = 0; u < kE; u++)
        {
            int ca[kPreA];
#pragma unroll
            for (int a = 0; a < kPreA; a++)
                ca[a] = al[u][a] >= 0 ? int(ncov[al[u][a]]) : 0;
#pragma unroll
            for (int a = 0; a < kPreA; a++)
                c[u] += ca[a];
        }
#pragma unroll
        for (int u = 0; u < kE; u++)
        {
            const int k = k0 + u * kWave + lane;
            if (k >= len)
                continue;
            for (int a = kPreA; a < ac[u]; a++)
                c[u] += int(ncov[int(aln[node[u] * kMaxAlignments + a])]);
            cons[len - 1 - k] = bs[u];
            cov[len - 1 - k]  = uint16_t(c[u]); // (uint16 sums wrap as the reference's do)
        }
    }
    return len;
}

template <typename SizeT, int kInst = 0>
__device__ __forceinline__ int consensus_lds(WinGraph<SizeT> g, int n, GWAMD_LDS uint8_t* scratch, int scratch_bytes,
                                             uint8_t* cons, uint16_t* cov, int max_cons)
{
    return consensus_lds_impl<SizeT, kInst>(g.base, g.in_cnt, g.out_cnt, g.aln_cnt, g.cov, g.in_w, g.in_e, g.out_e,
                                            g.aln, g.sorted, g.pos, n, scratch, scratch_bytes, cons, cov, max_cons);
}

// The consensus of one finished window: consensus_lds when the graph fits
// scratch_bytes (0: no LDS scratch, the v1 kernel) and force_hbm is not set,
// else consensus_raw on lane 0 and the reversal to host order.  len / status
// are wave-uniform (sh_len / sh_status: two LDS words of the caller); returns
// 1 when the LDS path ran, 0 for the HBM path.
template <typename SizeT, int kInst = 0>
__device__ __forceinline__ int consensus_window(WinGraph<SizeT> g, int n, int32_t* cscore, SizeT* cpred,
                                                uint8_t* cons_out, uint16_t* cov_out, int max_cons,
                                                GWAMD_LDS uint8_t* scratch, int scratch_bytes, bool force_hbm,
                                                int lane, int& sh_len, int& sh_status, int& len, int& status)
{
    if (scratch_bytes > 0 && !force_hbm)
    {
        const int r = consensus_lds<SizeT, kInst>(g, n, scratch, scratch_bytes, cons_out, cov_out, max_cons);
        if (r != kConsNoFit)
        {
            len    = r < 0 ? 0 : r;
            status = r < 0 ? -r : int(kSuccess);
            return 1;
        }
    }
    if (lane == 0)
    {
        const int r = consensus_raw<SizeT>(g, n, cscore, cpred, cons_out, cov_out, max_cons);
        sh_len      = r < 0 ? 0 : r;
        sh_status   = r < 0 ? -r : int(kSuccess);
    }
    wave_sync();
    len    = uniform(sh_len);
    status = uniform(sh_status);
    // reverse in place to host order (cudapoa_batch.cuh:241-246 does this on the host)
    for (int k = lane; k < len / 2; k += kWave)
    {
        uint8_t c0  = cons_out[k];
        uint8_t c1  = cons_out[len - 1 - k];
        uint16_t v0 = cov_out[k];
        uint16_t v1 = cov_out[len - 1 - k];
        cons_out[k] = c1, cons_out[len - 1 - k] = c0;
        cov_out[k] = v1, cov_out[len - 1 - k] = v0;
    }
    return 0;
}

} // namespace poa
} // namespace gwamd
