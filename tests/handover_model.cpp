// Host model of the block hand-over between two neighbouring waves of the
// 16-bit LDS forward pass: one producer and one consumer, each a small state
// machine over the arithmetic of csrc/poa_handover.hpp, stepped one shared-
// memory action at a time by a deterministic scheduler.  Built and run by
// tests/test_poa_handover_model.py.
//
// Checked for every V in 1 .. 3*64 + 2*B, B in {8, 16} and every scheduler:
//  * the consumer reads the carry of every row, and of the ring predecessors
//    r-1 .. r-7, from its register after the producer wrote it;
//  * no slot is rewritten before the consumer has loaded the row in it;
//  * both sides finish within a step bound (no deadlock, no livelock).
#include "poa_handover.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace gwamd::poa;

namespace
{

constexpr int kRingReach = 7; // ring predecessors: r - p <= ring_mask (8 ring rows)

struct Word
{
    int row = 0; // 0: never written
    int val = 0;
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
    enum St { kFlow, kReg, kSlots, kHead, kDone } st = kFlow;
    int r = 1, V, B;
    Word reg[kHandSlots];
    Producer(int V_, int B_) : V(V_), B(B_) { settle(); }
    void settle()
    {
        if (r > V)
            st = kDone;
    }
    bool blocked(const Shared& s) const
    {
        return st == kFlow && hand_opens(r, B) && hand_must_wait(r) && s.tail < hand_free_tail(r, B);
    }
    // taken[row]: the consumer has loaded row
    void step(Shared& s, const bool* taken)
    {
        switch (st)
        {
        case kFlow:
            if (!blocked(s))
                st = kReg;
            break;
        case kReg:
            reg[hand_slot(r)] = Word{r, carry_of(r)};
            st                = hand_closes(r, V, B) ? kSlots : kFlow;
            if (st == kFlow)
                r++, settle();
            break;
        case kSlots:
            for (int l = 0; l < kHandSlots; l++)
                if (hand_lane_in_block(l, r, B))
                {
                    const int old = s.slot[l].row;
                    if (old >= 1 && old <= V && old != reg[l].row && !taken[old])
                        throw Fail{"slot rewritten before its row was taken", old};
                    s.slot[l] = reg[l];
                }
            st = kHead;
            break;
        case kHead:
            s.head = r;
            st     = kFlow;
            r++, settle();
            break;
        case kDone: break;
        }
    }
};

struct Consumer
{
    enum St { kWait, kLoad, kTail, kUse, kDone } st = kWait;
    int r = 1, V, B;
    Word reg[kHandSlots];
    Consumer(int V_, int B_) : V(V_), B(B_)
    {
        if (r > V)
            st = kDone;
    }
    bool blocked(const Shared& s) const { return st == kWait && hand_opens(r, B) && s.head < hand_need_head(r, V, B); }
    void step(Shared& s, bool* taken)
    {
        switch (st)
        {
        case kWait:
            if (!hand_opens(r, B))
                st = kUse;
            else if (!blocked(s))
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
            st     = kUse;
            break;
        case kUse:
            for (int p = r; p >= 1 && p >= r - kRingReach; p--)
            {
                const Word w = reg[hand_slot(p)];
                if (w.row != p || w.val != carry_of(p))
                    throw Fail{p == r ? "carry of the row not in the register" : "ring predecessor's carry lost", p};
            }
            r++;
            st = r > V ? kDone : kWait;
            break;
        case kDone: break;
        }
    }
};

enum Sched { kProducerFirst, kConsumerFirst, kAlternate, kRandom, kScheds };

bool run(int V, int B, Sched sched, uint32_t seed)
{
    Shared s;
    Producer p(V, B);
    Consumer c(V, B);
    static bool taken[4 * kHandSlots + 64];
    for (bool& t : taken)
        t = false;
    const long bound = 16L * (V + 4); // every row is at most 4 actions a side
    long steps       = 0;
    uint32_t rng     = seed * 747796405u + 2891336453u;
    bool turn        = false;
    try
    {
        while (p.st != Producer::kDone || c.st != Consumer::kDone)
        {
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
                // runs of one side: the random schedule leans one way for a while
                pick_p = ((rng >> 16) & 7) < ((rng >> 28) & 1 ? 6u : 2u);
                break;
            }
            // a side that waits (or is done) yields; its spin is a step of the other
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
                    V, B, int(sched), seed, f.what, f.r, p.r, c.r, s.head, s.tail);
        return false;
    }
    return true;
}

} // namespace

int main()
{
    static_assert(hand_block_ok(8) && hand_block_ok(16) && !hand_block_ok(24), "B divides 64");
    static_assert(hand_opens(1, 16) && hand_closes(15, 100, 16) && hand_closes(5, 5, 16), "first block");
    static_assert(hand_free_tail(64, 16) == 15 && hand_need_head(64, 70, 16) == 70, "thresholds");
    int bad = 0, runs = 0;
    for (int B : {8, 16})
        for (int V = 1; V <= 3 * kHandSlots + 2 * B; V++)
            for (int sc = 0; sc < kScheds; sc++)
                for (uint32_t seed = 0; seed < (sc == kRandom ? 8u : 1u); seed++, runs++)
                    bad += !run(V, B, Sched(sc), seed);
    std::printf("%d runs, %d failed\n", runs, bad);
    return bad ? 1 : 0;
}
