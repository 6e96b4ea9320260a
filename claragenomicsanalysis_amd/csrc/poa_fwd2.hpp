// Forward pass of the LDS-resident POA kernel, round-4 row loop.
//
// Same recurrence, same outputs (E-domain ring rows, spill rows, one traceback
// code per cell with the reference's tie order, cudapoa_nw.cuh:222-327 and
// :361-443) as nw_forward_lds_pk; what changes is the instruction stream per
// graph row, which is what bounds config B (one wave issues at most one
// instruction every 4 cycles, and the round-3 loop spent ~390 issue slots per
// wave-row on 512 cells, 150 of them scalar):
//
//  * the row program marks every row the short paths cannot take (bit 7 of
//    its record, free because bases are ASCII): source nodes, predecessor
//    lists kept in HBM, predecessors farther back than the LDS ring, and
//    bases other than A/C/G/T.  Unmarked rows never test for any of these;
//  * a row with one predecessor takes a straight path: row r-1 from registers
//    (its last cell per lane by one DPP shift), any other from the ring.  The
//    finished row is carried to the next row as the register tuple it was
//    stored from (pin_row); the compiler still moves that tuple once per row
//    (two 64-bit moves) and one register on the r-1 path;
//  * the substitution scores come from a byte table per lane (score of the
//    lane's read column against A, C, T, G in one 32-bit word per column)
//    selected for the row's base with one v_perm per register pair, when
//    both scores fit a byte (otherwise the caller keeps nw_forward_lds_pk);
//  * the first span (column 0) and what a wave does with its carries (none,
//    next wave, HBM for the next sweep) are template parameters of the row
//    loop, so each wave runs a loop without the other roles' branches;
//  * the loop runs block by block (poa_handover.hpp): the hand-over's waits,
//    loads and stores sit between blocks of kHandBlock rows, and a row tests
//    once each for its kind, for a spill row and for a sink row.
//
// Included by poa_kernels.hip inside namespace gwamd::poa, after the round-3
// forward pass whose helpers (RowProg, load_row_pk, diag_src, pk_*) it uses.
#pragma once

// Rows per hand-over of carries between neighbouring waves (poa_handover.hpp);
// 0: the per-row tagged channel of nw_forward_lds_pk, for A/B builds.
#ifndef GWAMD_HAND_BLOCK
#define GWAMD_HAND_BLOCK 16
#endif
constexpr int kHandBlock = GWAMD_HAND_BLOCK;

// v with lane `sel` replaced by the wave-uniform x.  A compare and a select:
// this compiler has no builtin for v_writelane, and inline assembly for it
// has to put the lane select into m0, a register the compiler reserves and
// does not accept on a clobber list.
__device__ __forceinline__ int write_lane(int v, int x, int sel, int lane) { return lane == sel ? x : v; }

// 0 <= score <= 255 for both substitution scores in the E domain
__device__ __forceinline__ bool fwd2_ok(const Scores sc)
{
    const int s_eq = sc.match - sc.gap, s_ne = sc.mismatch - sc.gap;
    return s_eq >= 0 && s_eq <= 255 && s_ne >= 0 && s_ne <= 255;
}

// inclusive max-scan over the wave (builtins, so the scheduler can place
// other work in the DPP hazard slots)
__device__ __forceinline__ int wave_incl_max_b(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x143, 0xc, 0xf, false));
    return v;
}

// The row loop addresses the ring, the read and the row program through LDS
// pointers (lds_of) and the code and spill rows through global ones, so no
// access is a flat one: a flat access counts against the LDS counter too, and
// every LDS wait would then wait for the HBM code stores (measured: forward
// 45.3 -> 36.8 ms per window at config B).
typedef u32x4 fwd_u32x4;
typedef u32x2 fwd_u32x2;

// v stays one register tuple here (an empty statement the compiler cannot see through)
__device__ __forceinline__ void pin_row(fwd_u32x4& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin_row(fwd_u32x2& v) { asm volatile("" : "+v"(v)); }

template <int NR>
__device__ __forceinline__ void load_row_glb(const GWAMD_GLB int16_t* p, uint32_t (&P)[NR], uint32_t& prev)
{
    static_assert(NR % 4 == 0 || NR == 2, "4 or a multiple of 8 cells per lane");
    if constexpr (NR % 4 == 0)
    {
#pragma unroll
        for (int q = 0; q < NR / 4; q++)
        {
            const fwd_u32x4 v = *reinterpret_cast<const GWAMD_GLB fwd_u32x4*>(p + 1 + 8 * q);
            P[4 * q] = v.x, P[4 * q + 1] = v.y, P[4 * q + 2] = v.z, P[4 * q + 3] = v.w;
        }
    }
    else
    {
        const fwd_u32x2 v = *reinterpret_cast<const GWAMD_GLB fwd_u32x2*>(p + 1);
        P[0] = v.x, P[1] = v.y;
    }
    prev = uint32_t(uint16_t(p[0]));
}

template <int NR>
__device__ __forceinline__ void load_row_lds(const GWAMD_LDS int16_t* p, uint32_t (&P)[NR], uint32_t& prev)
{
    static_assert(NR % 4 == 0 || NR == 2, "4 or a multiple of 8 cells per lane");
    if constexpr (NR % 4 == 0)
    {
#pragma unroll
        for (int q = 0; q < NR / 4; q++)
        {
            const fwd_u32x4 v = *reinterpret_cast<const GWAMD_LDS fwd_u32x4*>(p + 1 + 8 * q);
            P[4 * q] = v.x, P[4 * q + 1] = v.y, P[4 * q + 2] = v.z, P[4 * q + 3] = v.w;
        }
    }
    else
    {
        const fwd_u32x2 v = *reinterpret_cast<const GWAMD_LDS fwd_u32x2*>(p + 1);
        P[0] = v.x, P[1] = v.y;
    }
    prev = uint32_t(uint16_t(p[0]));
}

// What a wave does with its rows' carries: nothing (the last span), hand
// them to the next wave of this sweep, or keep them in HBM for the next sweep
// (block hand-over only; the per-row channel build tests to_hbm per row).
enum : int
{
    kPostNone = 0,
    kPostFeed = 1,
    kPostHbm  = 2
};

template <int CPL, int NW, bool FIRST, int POST, int HB, typename SizeT>
__device__ __forceinline__ void fwd2_rows(WinGraph<SizeT> g, const RowProg& P, int V, const uint8_t* read_f, int L,
                                          int16_t* ring_f, int ring_stride, int16_t* spill_f, int stride,
                                          uint8_t* codes_f, int code_stride, const Scores sc,
                                          GWAMD_LDS uint8_t* shb, int16_t* carry_f, int lane, int wave, int cb,
                                          bool to_hbm, bool from_hbm, bool owner, int xl_cap, int& best_row,
                                          int& best_val, FwdProf& fp)
{
    static_assert(HB == 0 || (hand_block_ok(HB) && HB + kMaxRingRows16 <= kHandSlots && kChanRows == kHandSlots),
                  "a block and the ring's reach fit the 64 lanes of the carry register");
    static_assert(POST != kPostHbm || HB > 0, "the HBM carries are batched per block");
    constexpr bool FEED = POST == kPostFeed;
    g = as_global(g);
    GWAMD_LDS int16_t* ring          = lds_of(ring_f);
    const GWAMD_LDS uint8_t* read    = lds_of(read_f);
    const GWAMD_LDS uint32_t* prec   = lds_of(P.rec);
    const GWAMD_LDS uint16_t* pxl    = lds_of(P.xl);
    GWAMD_GLB int16_t* spill         = (GWAMD_GLB int16_t*)(spill_f);
    GWAMD_GLB uint8_t* codes         = (GWAMD_GLB uint8_t*)(codes_f);
    GWAMD_GLB int16_t* carry_hbm     = (GWAMD_GLB int16_t*)(carry_f);
    constexpr int NR    = CPL / 2;
    const int gap       = sc.gap;
    // end row so far, on the scalar unit
    int bval = uniform(best_val), brow = uniform(best_row);
    const int s_eq      = sc.match - gap;
    const int s_ne      = sc.mismatch - gap;
    const uint32_t gap2 = pk_bcast(gap);
    const uint32_t one2 = opaque_u32(0x00010001u);
    const uint32_t two2 = opaque_u32(0x00020002u);
    // wave-uniform (an SGPR): P arrives through a flat pointer, and a value
    // first used inside the row loop made the compiler wait for vmcnt(0) --
    // every outstanding code / spill store -- at the top of every row
    const int mask      = uniform(P.ring_mask);
    GWAMD_LDS int16_t* bnd               = (GWAMD_LDS int16_t*)(shb + kShBnd) + wave * (mask + 1);
    GWAMD_LDS uint32_t* chan             = (GWAMD_LDS uint32_t*)(shb + kShChan);
    volatile GWAMD_LDS uint32_t* chan_in  = chan + (wave - 1) * kChanRows; // wave > 0
    volatile GWAMD_LDS uint32_t* chan_out = chan + wave * kChanRows;       // wave < NW-1
    volatile GWAMD_LDS int* prog_v        = (GWAMD_LDS int*)(shb + kShProg); // [wave]: rows taken (tail)
    volatile GWAMD_LDS int* head_v        = (GWAMD_LDS int*)(shb + kShHead); // [wave]: rows posted (head)
    const int jb     = cb + lane * CPL;
    const bool active = jb < L;
    const int ja     = active ? jb : 0; // address used by inactive lanes
    // owner of the last column (L-1) within the span: lane, cell
    const int own_lane = ((L > 0 ? L - 1 : 0) % (kWave * CPL)) / CPL;
    const int own_c    = (L > 0 ? L - 1 : 0) % CPL;
    // a whole-wave list read at offset xl_cap still ends inside the shared
    // region that follows the lists (>= 64 entries), and real lists end
    // before xl_cap
    const int xl_last = xl_cap;
    // bit 14 of a record marks a sink row; only the wave that owns the last
    // column looks at it
    const uint32_t sink_bit = uniform(int(owner)) ? (1u << 14) : 0u;

    // substitution byte table: byte b of T[c] = score of read column jb + c + 1
    // (read[jb + c]) against base code b = (base >> 1) & 3 (A 0, C 1, T 2, G 3)
    uint32_t T[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++)
    {
        const int ch = int(read[ja + c]);
        T[c] = uint32_t(ch == 'A' ? s_eq : s_ne) | (uint32_t(ch == 'C' ? s_eq : s_ne) << 8) |
               (uint32_t(ch == 'T' ? s_eq : s_ne) << 16) | (uint32_t(ch == 'G' ? s_eq : s_ne) << 24);
    }
    // Final E of row r-1 (row 0: zeros), carried from row to row as the
    // register tuples the row was stored from: as separate 32-bit values the
    // compiler kept them in registers of their own and copied the finished
    // row there (and back for a row with the predecessor r-1) on every row.
    // pin_row keeps each tuple whole across the loop's back edge.
    constexpr int VW = NR % 4 == 0 ? 4 : 2;
    constexpr int NV = NR / VW;
    using RowVec     = std::conditional_t<VW == 4, fwd_u32x4, fwd_u32x2>;
    RowVec Ev[NV];
#pragma unroll
    for (int q = 0; q < NV; q++)
    {
        Ev[q] = RowVec(0);
        pin_row(Ev[q]);
    }
    auto Eprev = [&](int i) __attribute__((always_inline)) { return uint32_t(Ev[i / VW][i % VW]); };
    int cin_prev = 0;
    // Carries by row, lane r & 63.  Received ones (wave > 0: from the channel;
    // wave 0 of a later sweep: from HBM; never both), HB > 0: the block of the
    // current row and the 64 - HB rows before it, which covers the ring's
    // reach.  Posted ones (FEED, HB > 0): the block being filled.
    int cv  = 0;
    int pvr = 0;
    uint32_t rec_c = uint32_t(uniform(int(prec[1])));
    uint32_t rec_n = uint32_t(uniform(int(prec[min(2, V)])));
    // lanes k < np: predecessor rows of row r (rows with a list in LDS)
    auto xls_at = [&](int i) { return int(pxl[i]); };
    int pv_c = xls_at(min(int(rec_c >> 16), xl_last) + lane);
    GWAMD_GLB uint8_t* crow = codes + code_stride;
    GWAMD_GLB int16_t* srow = spill + stride;
    GWAMD_FP_START(fp);
    // Outer loop: one hand-over block of rows [r, rl] (HB == 0: every row in
    // one block), which opens before its first row and is posted after its
    // last; the rows inside test for neither.
    for (int r = 1, rl; r <= V; r = rl + 1)
    {
        rl = HB > 0 ? hand_block_last(r, V, HB) : V;
        if constexpr (HB > 0)
        {
            GWAMD_FP_MARK(fp, 4);
            if (!FIRST)
            {
                // the carries of this block of rows, into their lanes of cv
                if (from_hbm)
                {
                    const int x = hand_lane_row(lane, r);
                    uint32_t hc = x >= 1 && x <= V ? uint32_t(int(carry_hbm[x])) : 0u;
                    settle_vm1(hc); // wait here, once per block, not at every row's readlane
                    cv = hand_lane_in_block(lane, r, HB) ? int(hc) : cv;
                }
                else
                {
                    const int need = hand_need_head(r, V, HB);
                    while (uniform(head_v[wave - 1]) < need)
                    {
                        GWAMD_FP_COUNT(fp, 4);
                        __builtin_amdgcn_s_sleep(1);
                    }
                    const int w = int(chan_in[lane]);
                    cv          = hand_lane_in_block(lane, r, HB) ? w : cv;
                    if (lane == 0)
                        prog_v[wave] = hand_new_tail(r, V, HB); // after the load, from the same wave
                }
            }
            if (FEED && hand_must_wait(r))
            {
                // flow control: the consumer must have taken the block whose slots this one reuses
                const int need = hand_free_tail(r, HB);
                while (uniform(prog_v[wave + 1]) < need)
                {
                    GWAMD_FP_COUNT(fp, 5);
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            GWAMD_FP_LAP(fp, 4);
        }
        for (; r <= rl; r++, crow += code_stride, srow += stride)
        {
            GWAMD_FP_COUNT(fp, 7);
            const uint32_t rec = rec_c;
            // next rows: the record of row r+2, the predecessor list of row r+1
            const uint32_t rec_nn = prec[min(r + 2, V)];
            // (read for every row: rows without a list get garbage they never
            // use; the offset is clamped into the list region)
            const int pv_n = xls_at(min(int(rec_n >> 16), xl_last) + lane);
            const int np       = int((rec >> 8) & 63);
            GWAMD_LDS int16_t* row = ring + (r & mask) * ring_stride;
            uint32_t sig[NR];
            {
                const uint32_t bsel = 0x0c040c00u + ((rec >> 1) & 3u) * 0x00010001u;
#pragma unroll
                for (int i = 0; i < NR; i++)
                    sig[i] = __builtin_amdgcn_perm(T[2 * i + 1], T[2 * i], bsel);
            }
            GWAMD_FP_LAP(fp, 0);
            int cin = 0;
            // Rest of the row once dg, vt (and kd, kv) hold the maxima over the
            // predecessors: in-lane prefix, closure across lanes and spans,
            // codes and stores.  Instantiated once per path so each path is
            // straight-line code.
            auto finish = [&](auto multi_tag, const uint32_t(&dg)[NR], const uint32_t(&vt)[NR],
                              const uint32_t(&kd)[NR], const uint32_t(&kv)[NR], int c0v,
                              int c0kv) __attribute__((always_inline)) {
                constexpr bool kMulti = decltype(multi_tag)::value;
                uint32_t E[NR];
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    const uint32_t s = pk_max_lo_into_hi(pk_max(dg[i], vt[i]));
                    E[i]             = i == 0 ? s : pk_max_hi_carry(s, E[i - 1]);
                }
                const int m    = active ? int(int16_t(E[NR - 1] >> 16)) : kNeg;
                const int incl = wave_incl_max_b(m);
                const int excl = __builtin_amdgcn_update_dpp(kNeg, incl, 0x138, 0xf, 0xf, false);
                const int wtot = __builtin_amdgcn_readlane(incl, kWave - 1);
                GWAMD_FP_LAP(fp, 3);
                GWAMD_FP_MARK(fp, 4);
                if (FIRST)
                {
                    cin = c0v + gap; // column 0
                    if (lane == 0)
                    {
                        row[kColShift]  = int16_t(cin);
                        crow[kColShift] = uint8_t(1 | (c0kv << 2));
                    }
                }
                else
                {
                    if constexpr (HB > 0)
                        cin = int(int16_t(__builtin_amdgcn_readlane(cv, hand_slot(r))));
                    else if (from_hbm)
                    {
                        // carry of this row from the previous sweep's last span
                        if (((r - 1) & (kWave - 1)) == 0)
                        {
                            const int x = r + lane;
                            uint32_t hc = x <= V ? uint32_t(int(carry_hbm[x])) : 0u;
                            settle_vm1(hc); // wait here, once per 64 rows, not at every row's readlane
                            cv = int(hc);
                        }
                        cin = int(int16_t(__builtin_amdgcn_readlane(cv, (r - 1) & (kWave - 1))));
                    }
                    else
                    {
                        // carry of this row from the previous span
                        uint32_t w = uint32_t(uniform(int(chan_in[r & (kChanRows - 1)])));
                        while ((w >> 16) != (uint32_t(r) & 0xffffu))
                        {
                            GWAMD_FP_COUNT(fp, 4);
                            __builtin_amdgcn_s_sleep(1);
                            w = uint32_t(uniform(int(chan_in[r & (kChanRows - 1)])));
                        }
                        cin = int(int16_t(w & 0xffffu));
                        if ((r & 7) == 0 && lane == 0)
                            prog_v[wave] = r;
                    }
                    if constexpr (HB == 0)
                    {
                        if (lane == 0)
                            bnd[r & mask] = int16_t(cin);
                    }
                }
                if constexpr (HB > 0)
                {
                    if (POST != kPostNone)
                        pvr = write_lane(pvr, max(cin, wtot), hand_slot(r), lane);
                }
                else if (FEED)
                {
                    // flow control: the consumer must have taken row r-kChanRows+32
                    if ((r & 31) == 0 && r >= kChanRows)
                    {
                        while (uniform(prog_v[wave + 1]) < r - 32)
                        {
                            GWAMD_FP_COUNT(fp, 5);
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    if (lane == 0)
                        chan_out[r & (kChanRows - 1)] = (uint32_t(r) << 16) | uint32_t(uint16_t(max(cin, wtot)));
                }
                if (HB == 0 && to_hbm && lane == 0)
                    carry_hbm[r] = int16_t(max(cin, wtot));
                GWAMD_FP_LAP(fp, 4);
                const uint32_t b2v = pk_bcast(max(excl, cin));
#pragma unroll
                for (int i = 0; i < NR; i++)
                    E[i] = pk_max(E[i], b2v);
                if (active)
                {
                    // codes: 0 diagonal, 1 vertical, 2 horizontal (+ slot << 2)
                    uint32_t code[NR];
#pragma unroll
                    for (int i = 0; i < NR; i++)
                    {
                        if constexpr (kMulti)
                        {
                            const uint32_t a   = pk_min_u(pk_sub(E[i], dg[i]), one2); // 0: diagonal match
                            const uint32_t bb  = pk_min_u(pk_sub(E[i], vt[i]), one2); // 0: vertical match
                            const uint32_t cvh = pk_mad(bb, pk_sub(two2, kv[i]), kv[i]); // vertical or horizontal
                            code[i]            = pk_mad(a, pk_sub(cvh, kd[i]), kd[i]);
                        }
                        else
                        {
                            // one predecessor (slot 0): a + min(a, E - vt)
                            const uint32_t a = pk_min_u(pk_sub(E[i], dg[i]), one2);
                            code[i]          = pk_add(a, pk_min_u(pk_sub(E[i], vt[i]), a));
                        }
                    }
                    if constexpr (NR % 4 == 0)
                    {
#pragma unroll
                        for (int q = 0; q < NR / 4; q++)
                        {
                            const fwd_u32x4 ev = {E[4 * q], E[4 * q + 1], E[4 * q + 2], E[4 * q + 3]};
                            *reinterpret_cast<GWAMD_LDS fwd_u32x4*>(row + jb + kColShift + 1 + 8 * q) = ev;
                            const uint32_t w0 = __builtin_amdgcn_perm(code[4 * q + 1], code[4 * q], 0x06040200u);
                            const uint32_t w1 = __builtin_amdgcn_perm(code[4 * q + 3], code[4 * q + 2], 0x06040200u);
                            __builtin_nontemporal_store(uint64_t(w0) | (uint64_t(w1) << 32),
                                                        reinterpret_cast<GWAMD_GLB uint64_t*>(crow + jb + kColShift + 1 + 8 * q));
                        }
                    }
                    else
                    {
                        const fwd_u32x2 ev = {E[0], E[1]};
                        *reinterpret_cast<GWAMD_LDS fwd_u32x2*>(row + jb + kColShift + 1) = ev;
                        __builtin_nontemporal_store(__builtin_amdgcn_perm(code[1], code[0], 0x06040200u),
                                                    reinterpret_cast<GWAMD_GLB uint32_t*>(crow + jb + kColShift + 1));
                    }
                }
                if (rec & (1u << 15))
                {
                    // the row's copy in HBM, tested once per row: the span's
                    // first column (column 0, or the previous span's last cell)
                    // from lane 0, then the lanes' cells
                    if (lane == 0)
                        srow[cb + kColShift] = int16_t(cin);
                    if (active)
                    {
                        if constexpr (NR % 4 == 0)
                        {
#pragma unroll
                            for (int q = 0; q < NR / 4; q++)
                            {
                                const fwd_u32x4 ev = {E[4 * q], E[4 * q + 1], E[4 * q + 2], E[4 * q + 3]};
                                *reinterpret_cast<GWAMD_GLB fwd_u32x4*>(srow + jb + kColShift + 1 + 8 * q) = ev;
                            }
                        }
                        else
                        {
                            const fwd_u32x2 ev = {E[0], E[1]};
                            *reinterpret_cast<GWAMD_GLB fwd_u32x2*>(srow + jb + kColShift + 1) = ev;
                        }
                    }
                }
                GWAMD_FP_LAP(fp, 5);
                if (rec & sink_bit)
                {
                    // sink row: E at the last column (column 0 for an empty read),
                    // read back from the ring row just stored
                    int endv = cin;
#pragma unroll
                    for (int i = 0; i < NR; i++)
                    {
                        if (2 * i == own_c)
                            endv = int(int16_t(E[i] & 0xffff));
                        if (2 * i + 1 == own_c)
                            endv = int(int16_t(E[i] >> 16));
                    }
                    // (compared on the scalar unit: a vector compare put an exec
                    // region with the loop-carried copies behind every row)
                    const int v = uniform(L == 0 ? cin : __builtin_amdgcn_readlane(endv, own_lane));
                    if (bval < v)
                        bval = v, brow = r;
                }
#pragma unroll
                for (int q = 0; q < NV; q++)
                {
#pragma unroll
                    for (int k = 0; k < VW; k++)
                        Ev[q][k] = E[VW * q + k];
                    pin_row(Ev[q]);
                }
            };
            // one compare for the commonest kind: no mark (bit 7) and a
            // predecessor count (bits 8-13) of one
            if ((rec & 0x3f80u) == 0x0100u)
            {
                // one predecessor, in registers (row r-1) or in the ring
                const int d = int(rec >> 16);
                uint32_t Pr[NR], prev;
                if (d == 1)
                {
                    GWAMD_FP_COUNT(fp, 0);
#pragma unroll
                    for (int i = 0; i < NR; i++)
                        Pr[i] = Eprev(i);
                    prev = uint32_t(__builtin_amdgcn_update_dpp(int(uint32_t(uint16_t(cin_prev))),
                                                                int(Eprev(NR - 1) >> 16), 0x138, 0xf, 0xf, false));
                }
                else
                {
                    GWAMD_FP_COUNT(fp, 1);
                    const int ps = (r - d) & mask;
                    load_row_lds<NR>(ring + ps * ring_stride + ja + kColShift, Pr, prev);
                    if (!FIRST)
                    {
                        const uint32_t bv = HB > 0 ? uint32_t(__builtin_amdgcn_readlane(cv, hand_slot(r - d))) & 0xffffu
                                                   : uint32_t(uint16_t(bnd[ps]));
                        prev              = lane == 0 ? bv : prev;
                    }
                }
                const int c0v = FIRST ? int(int16_t(__builtin_amdgcn_readfirstlane(prev))) : 0;
                uint32_t dg[NR], vt[NR];
                diag_src<NR>(Pr, prev, dg);
#pragma unroll
                for (int i = 0; i < NR; i++)
                {
                    dg[i] = pk_add(dg[i], sig[i]);
                    vt[i] = pk_add(Pr[i], gap2);
                }
                GWAMD_FP_LAP(fp, 1);
                finish(std::false_type{}, dg, vt, dg, vt, c0v, 0);
            }
            else
            {
                // Several predecessors (slot by slot with the first maximising
                // slot), and the rows the row program marked (sources, far or
                // escaped predecessors, other bases).  The two kinds get separate
                // predecessor loaders: a loader that tested the mark per slot was
                // miscompiled (ROCm 7.2: the flag reached the slot tests inverted).
                auto rows_general = [&](auto slow_tag, int pv, int n) __attribute__((always_inline)) {
                    constexpr bool kSlow = decltype(slow_tag)::value;
                    auto load_pred = [&](int p, uint32_t(&Q)[NR], uint32_t& qprev) __attribute__((always_inline)) {
                        if (p == r - 1)
                        {
#pragma unroll
                            for (int i = 0; i < NR; i++)
                                Q[i] = Eprev(i);
                            qprev = uint32_t(__builtin_amdgcn_update_dpp(int(uint32_t(uint16_t(cin_prev))),
                                                                         int(Eprev(NR - 1) >> 16), 0x138, 0xf, 0xf,
                                                                         false));
                            return;
                        }
                        if constexpr (kSlow)
                        {
                            if (p == 0)
                            {
#pragma unroll
                                for (int i = 0; i < NR; i++)
                                    Q[i] = 0;
                                qprev = 0;
                                return;
                            }
                            if (r - p > mask)
                            {
                                load_row_glb<NR>(spill + size_t(p) * stride + ja + kColShift, Q, qprev);
                                settle_vm<NR>(Q, qprev);
                                return;
                            }
                        }
                        load_row_lds<NR>(ring + (p & mask) * ring_stride + ja + kColShift, Q, qprev);
                        if (!FIRST)
                        {
                            const uint32_t bv = HB > 0 ? uint32_t(__builtin_amdgcn_readlane(cv, hand_slot(p))) & 0xffffu
                                                       : uint32_t(uint16_t(bnd[p & mask]));
                            qprev             = lane == 0 ? bv : qprev;
                        }
                    };
                    uint32_t dg[NR], vt[NR];
                    int c0v = 0, c0kv = 0;
                    {
                        uint32_t Pv[NR], prev;
                        load_pred(__builtin_amdgcn_readfirstlane(pv), Pv, prev);
                        if (FIRST)
                            c0v = int(int16_t(__builtin_amdgcn_readfirstlane(prev)));
                        diag_src<NR>(Pv, prev, dg);
#pragma unroll
                        for (int i = 0; i < NR; i++)
                        {
                            dg[i] = pk_add(dg[i], sig[i]);
                            vt[i] = pk_add(Pv[i], gap2);
                        }
                    }
                    if (n > 1)
                    {
                        uint32_t kd[NR], kv[NR];
#pragma unroll
                        for (int i = 0; i < NR; i++)
                        {
                            kd[i] = 0;
                            kv[i] = one2;
                        }
                        for (int k = 1; k < n; k++)
                        {
                            uint32_t Q[NR], qprev, dq[NR];
                            load_pred(__builtin_amdgcn_readlane(pv, k), Q, qprev);
                            if (FIRST)
                            {
                                // column 0: first maximising predecessor slot
                                const int pe = int(int16_t(__builtin_amdgcn_readfirstlane(qprev)));
                                c0kv         = pe > c0v ? k : c0kv;
                                c0v          = max(c0v, pe);
                            }
                            diag_src<NR>(Q, qprev, dq);
                            const uint32_t kk4 = pk_bcast(4 * k);
                            const uint32_t kk1 = pk_bcast(4 * k + 1);
#pragma unroll
                            for (int i = 0; i < NR; i++)
                            {
                                const uint32_t d  = pk_add(dq[i], sig[i]);
                                const uint32_t nd = pk_max(dg[i], d);
                                kd[i] = pk_mad(pk_min_u(pk_sub(nd, dg[i]), one2), pk_sub(kk4, kd[i]), kd[i]);
                                dg[i] = nd;
                                const uint32_t v  = pk_add(Q[i], gap2);
                                const uint32_t nv = pk_max(vt[i], v);
                                kv[i] = pk_mad(pk_min_u(pk_sub(nv, vt[i]), one2), pk_sub(kk1, kv[i]), kv[i]);
                                vt[i] = nv;
                            }
                        }
                        GWAMD_FP_LAP(fp, 2);
                        finish(std::true_type{}, dg, vt, kd, kv, c0v, c0kv);
                    }
                    else
                    {
                        GWAMD_FP_LAP(fp, 2);
                        finish(std::false_type{}, dg, vt, dg, vt, c0v, 0);
                    }
                };
                if (!(rec & 0x80u))
                {
                    GWAMD_FP_COUNT(fp, 2);
                    rows_general(std::false_type{}, pv_c, np); // np >= 2, every predecessor in the ring
                }
                else
                {
                    GWAMD_FP_COUNT(fp, 3);
                    // predecessor rows (sources: n = 1, row 0); lists through the
                    // typed LDS pointer (P's own is flat: its loads count in
                    // vmcnt, so a wait for them also waits for every code store)
                    int n  = np;
                    int pv = 0;
                    if (np == int(kRecEscape))
                        pv = row_preds<SizeT>(P, g, r, rec, lane, n);
                    else
                    {
                        if (np >= 2)
                            pv = lane < np ? int(pxl[(rec >> 16) + lane]) : 0;
                        else if (np == 1)
                            pv = r - int(rec >> 16);
                        if (np == 0)
                            n = 1;
                    }
                    const uint32_t ub = uint32_t(row_base<SizeT>(g, rec, r));
                    if (!((ub & 0xc0u) == 0x40u && ((0x10008aull >> (ub & 0x3fu)) & 1u)))
                    {
                        const GWAMD_LDS uint32_t* rw = reinterpret_cast<const GWAMD_LDS uint32_t*>(read + ja);
#pragma unroll
                        for (int i = 0; i < NR; i++)
                        {
                            const uint32_t wv = rw[i / 2] >> ((i & 1) * 16);
                            const int ch0 = int(wv & 0xff), ch1 = int((wv >> 8) & 0xff);
                            sig[i]        = uint32_t(uint16_t(ch0 == int(ub) ? s_eq : s_ne)) |
                                     (uint32_t(uint16_t(ch1 == int(ub) ? s_eq : s_ne)) << 16);
                        }
                    }
                    rows_general(std::true_type{}, pv, uniform(n));
                }
            }
            cin_prev = cin;
            rec_c    = rec_n;
            rec_n    = uint32_t(uniform(int(rec_nn)));
            pv_c     = pv_n;
            GWAMD_FP_LAP(fp, 6);
        } // rows of the block
        if constexpr (HB > 0)
        {
            // rl closes the block: its last row, or row V (a partial block)
            if (FEED)
            {
                GWAMD_FP_MARK(fp, 4);
                // post the block: its carries, then the head, from the same wave
                if (hand_lane_in_block(lane, rl, HB))
                    chan_out[lane] = uint32_t(pvr);
                if (lane == 0)
                    head_v[wave] = rl;
                GWAMD_FP_LAP(fp, 4);
            }
            else if (POST == kPostHbm)
            {
                // the block's carries for the next sweep, one store per lane
                const int x = hand_lane_row(lane, rl);
                if (hand_lane_in_block(lane, rl, HB) && x >= 1 && x <= rl)
                    carry_hbm[x] = int16_t(pvr);
            }
        }
    }
    GWAMD_FP_STOP(fp);
    best_val = bval;
    best_row = brow;
}

// Drop-in for nw_forward_lds_pk (same arguments and result) when fwd2_ok(sc).
template <int CPL, int NW, typename SizeT>
__device__ int nw_forward_lds_v2(WinGraph<SizeT> g, const RowProg& P, int V, const uint8_t* read, int L,
                                 int16_t* ring, int ring_stride, int16_t* spill, int stride, uint8_t* codes,
                                 int code_stride, const Scores sc, GWAMD_LDS uint8_t* shb, int16_t* carry_hbm,
                                 int tid, int xl_cap, FwdProf& fp)
{
    constexpr int kSpan = kWave * CPL;
    const int lane      = tid & (kWave - 1);
    const int wave      = uniform(tid / kWave);
    V                   = uniform(V);
    L                   = uniform(L);
    const int jl        = L > 0 ? L - 1 : 0;
    const int own_span  = jl / kSpan;
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
        if (!wact || V < 1)
            continue;
        auto rows = [&](auto first_tag, auto post_tag) __attribute__((always_inline)) {
            fwd2_rows<CPL, NW, decltype(first_tag)::value, decltype(post_tag)::value, kHandBlock>(
                g, P, V, read, L, ring, ring_stride, spill, stride, codes, code_stride, sc, shb, carry_hbm, lane, wave,
                cb, to_hbm, from_hbm, owner, xl_cap, best_row, best_val, fp);
        };
        // (feed and to_hbm exclude each other: a wave with a next span in
        // this sweep is not the sweep's last)
        auto rows_post = [&](auto first_tag) __attribute__((always_inline)) {
            if (feed)
            {
                rows(first_tag, std::integral_constant<int, kPostFeed>{});
                return;
            }
            if constexpr (kHandBlock > 0)
            {
                if (to_hbm)
                {
                    rows(first_tag, std::integral_constant<int, kPostHbm>{});
                    return;
                }
            }
            rows(first_tag, std::integral_constant<int, kPostNone>{});
        };
        if (first)
            rows_post(std::true_type{});
        else
            rows_post(std::false_type{});
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
