// Host model of the block hand-over as the row loop is now written (fwd2_rows,
// poa_fwd2.hpp): an outer loop whose step is one block [r0, rl] with
// rl = hand_block_last(r0, V, B), the waits, loads and stores between blocks,
// and no hand_opens / hand_closes test inside.  One producer against one
// consumer, stepped one shared-memory action at a time by the schedulers of
// tests/handover_model.cpp.  Built and run by
// tests/test_poa_handover_block_model.py.
//
// Checked for every V in 1 .. 3*64 + 2*B, B in {8, 16} and every scheduler:
//  * the blocks of the outer loop are those of the per-row tests: row r0 opens
//    one, rl closes it, and no row between does either;
//  * the consumer finds the carry of every row and of the ring predecessors
//    r-1 .. r-7 in its register, written by the producer;
//  * no slot is rewritten before the consumer has loaded the row in it;
//  * the sweep's last wave stores every row's carry to carry[1 .. V] exactly
//    once, from the lane that holds it, and nothing outside;
//  * both sides finish within a step bound, with head = tail = V.
#include "poa_handover.hpp"

#include <cstdint>
#include <cstdio>
#include <initializer_list>

using namespace gwamd::poa;

namespace
{

constexpr int kRingReach = 7;
constexpr int kMaxV      = 4 * kHandSlots + 64;

struct Word
{
    int row = 0, val = 0;
};
int carry_of(int r) { return (r * 2654435761u >> 7) & 0x7fff; }

struct Shared
{
    Word slot[kHandSlots];
    int head = 0, tail = 0;
};
struct Fail
{
    const char* what;
    int r;
};

struct Producer
{
    enum St { kFlow, kRows, kSlots, kHead, kDone } st = kFlow;
    int r = 1, rl = 0, V, B;
    Word reg[kHandSlots];
    Producer(int V_, int B_) : V(V_), B(B_) { open(); }
    void open()
    {
        if (r > V)
        {
            st = kDone;
            return;
        }
        if (!hand_opens(r, B))
            throw Fail{"block starts at a row that does not open one", r};
        rl = hand_block_last(r, V, B);
        st = kFlow;
    }
    bool blocked(const Shared& s) const { return st == kFlow && hand_must_wait(r) && s.tail < hand_free_tail(r, B); }
    void step(Shared& s, const bool* taken)
    {
        switch (st)
        {
        case kFlow:
            if (!blocked(s))
                st = kRows;
            break;
        case kRows: // the inner loop: one register write per row, no test
            for (; r <= rl; r++)
            {
                if (r < rl && hand_closes(r, V, B))
                    throw Fail{"a row inside the block closes one", r};
                reg[hand_slot(r)] = Word{r, carry_of(r)};
            }
            if (!hand_closes(rl, V, B))
                throw Fail{"block's last row does not close it", rl};
            st = kSlots;
            break;
        case kSlots:
            for (int l = 0; l < kHandSlots; l++)
                if (hand_lane_in_block(l, rl, B))
                {
                    const int old = s.slot[l].row;
                    if (old >= 1 && old <= V && old != reg[l].row && !taken[old])
                        throw Fail{"slot rewritten before its row was taken", old};
                    s.slot[l] = reg[l];
                }
            st = kHead;
            break;
        case kHead:
            s.head = rl;
            r      = rl + 1;
            open();
            break;
        case kDone: break;
        }
    }
};

struct Consumer
{
    enum St { kWait, kLoad, kTail, kRows, kDone } st = kWait;
    int r = 1, rl = 0, V, B;
    Word reg[kHandSlots];
    Consumer(int V_, int B_) : V(V_), B(B_) { open(); }
    void open()
    {
        if (r > V)
        {
            st = kDone;
            return;
        }
        rl = hand_block_last(r, V, B);
        st = kWait;
    }
    bool blocked(const Shared& s) const { return st == kWait && s.head < hand_need_head(r, V, B); }
    void step(Shared& s, bool* taken)
    {
        switch (st)
        {
        case kWait:
            if (!blocked(s))
                st = kLoad;
            break;
        case kLoad:
            for (int l = 0; l < kHandSlots; l++)
                if (hand_lane_in_block(l, r, B))
                {
                    reg[l] = s.slot[l];
                    if (reg[l].row >= 1)
                        taken[reg[l].row] = true;
                }
            st = kTail;
            break;
        case kTail:
            s.tail = hand_new_tail(r, V, B);
            st     = kRows;
            break;
        case kRows:
            for (; r <= rl; r++)
            {
                for (int p = r; p >= 1 && p >= r - kRingReach; p--)
                {
                    const Word w = reg[hand_slot(p)];
                    if (w.row != p || w.val != carry_of(p))
                        throw Fail{p == r ? "carry of the row not in the register" : "ring predecessor's carry lost", p};
                }
            }
            open();
            break;
        case kDone: break;
        }
    }
};

// the sweep's last wave: the block's lanes to carry[row] after the block's last row
bool hbm_carries(int V, int B)
{
    static int written[kMaxV];
    for (int& w : written)
        w = 0;
    Word reg[kHandSlots];
    for (int r = 1, rl; r <= V; r = rl + 1)
    {
        rl = hand_block_last(r, V, B);
        for (int q = r; q <= rl; q++)
            reg[hand_slot(q)] = Word{q, carry_of(q)};
        for (int l = 0; l < kHandSlots; l++)
        {
            const int x = hand_lane_row(l, rl);
            if (hand_lane_in_block(l, rl, B) && x >= 1 && x <= rl)
            {
                if (reg[l].row != x || reg[l].val != carry_of(x))
                {
                    std::printf("FAIL V=%d B=%d: lane %d does not hold row %d\n", V, B, l, x);
                    return false;
                }
                written[x]++;
            }
        }
    }
    for (int x = 0; x < kMaxV; x++)
        if (written[x] != (x >= 1 && x <= V ? 1 : 0))
        {
            std::printf("FAIL V=%d B=%d: carry[%d] stored %d times\n", V, B, x, written[x]);
            return false;
        }
    return true;
}

enum Sched { kProducerFirst, kConsumerFirst, kAlternate, kRandom, kScheds };

bool run(int V, int B, Sched sched, uint32_t seed)
{
    Shared s;
    static bool taken[kMaxV];
    for (bool& t : taken)
        t = false;
    const long bound = 16L * (V + 4);
    long steps       = 0;
    uint32_t rng     = seed * 747796405u + 2891336453u;
    bool turn        = false;
    int pr = 0, cr = 0;
    try
    {
        Producer p(V, B);
        Consumer c(V, B);
        while (p.st != Producer::kDone || c.st != Consumer::kDone)
        {
            pr = p.r, cr = c.r;
            if (++steps > bound)
                throw Fail{"step bound reached", p.r};
            const bool pcan = p.st != Producer::kDone && !p.blocked(s);
            const bool ccan = c.st != Consumer::kDone && !c.blocked(s);
            if (!pcan && !ccan)
                throw Fail{"both sides wait", p.r};
            bool pick_p;
            switch (sched)
            {
            case kProducerFirst: pick_p = true; break;
            case kConsumerFirst: pick_p = false; break;
            case kAlternate: pick_p = (turn = !turn); break;
            default:
                rng    = rng * 1664525u + 1013904223u;
                pick_p = ((rng >> 16) & 7) < ((rng >> 28) & 1 ? 6u : 2u);
                break;
            }
            if (pick_p && !pcan)
                pick_p = false;
            else if (!pick_p && !ccan)
                pick_p = true;
            if (pick_p)
                p.step(s, taken);
            else
                c.step(s, taken);
        }
        if (s.head != V || s.tail != V)
            throw Fail{"head and tail do not end at V", s.head};
    }
    catch (const Fail& f)
    {
        std::printf("FAIL V=%d B=%d sched=%d seed=%u: %s (row %d; producer row %d, consumer row %d, head %d, tail %d)\n",
                    V, B, int(sched), seed, f.what, f.r, pr, cr, s.head, s.tail);
        return false;
    }
    return true;
}

} // namespace

int main()
{
    int bad = 0, runs = 0;
    for (int B : {8, 16})
        for (int V = 1; V <= 3 * kHandSlots + 2 * B; V++)
        {
            bad += !hbm_carries(V, B), runs++;
            for (int sc = 0; sc < kScheds; sc++)
                for (uint32_t seed = 0; seed < (sc == kRandom ? 8u : 1u); seed++, runs++)
                    bad += !run(V, B, Sched(sc), seed);
        }
    std::printf("%d runs, %d failed\n", runs, bad);
    return bad ? 1 : 0;
}
