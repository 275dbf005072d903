// tools/check_offer_host.cpp — runs rays1bench_amd/csrc/r1_offer.h on the host (tests/test_offer_rule_host.py):
//   check_offer_host offer <random cases> <seed>   r1_offer_better against the written-out rule (t < best) | (t == best & id < best_id)
// Prints "name value" lines; exit status 1 and "MISMATCH ..." lines on stderr (the first few) where the two sides differ.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../rays1bench_amd/csrc/r1_offer.h"

static float from_bits(const uint32_t u)
{
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
static uint32_t bits_of(const float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

static unsigned long long mismatches = 0;
static void report(const char *what, const float t, const uint32_t id, const float best, const uint32_t best_id)
{
    if (mismatches++ < 10)
        fprintf(stderr, "MISMATCH %s t=%08x id=%08x best=%08x best_id=%08x\n", what, bits_of(t), id, bits_of(best), best_id);
}

// the rule as the kernels wrote it out before, on floats (volatile: no compiler may reason the two sides into one)
static bool rule(const float t, const uint32_t id, const float best, const uint32_t best_id)
{
    volatile float vt = t, vb = best;
    return (vt < vb) | ((vt == vb) & (id < best_id));
}

static uint64_t rng_state;
static uint32_t rnd32()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

static int run_offer(const unsigned long long n_random, const uint64_t seed)
{
    const uint32_t b001 = bits_of(0.001f), bmax = bits_of(FLT_MAX);
    const float ts[] = {from_bits(b001 - 1u), 0.001f,  from_bits(b001 + 1u), FLT_MIN, 1.0f, from_bits(bmax - 1u),
                        FLT_MAX,              INFINITY, from_bits(0x7FC00000u), from_bits(0xFFC00000u)};
    const uint32_t ids[] = {0u, 1u, 0xFFFFFFFEu}, best_ids[] = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    unsigned long long grid = 0, grid_raw = 0, grid_updates = 0, ties = 0, tie_wins = 0, none_state_flt_max = 0;
    for (const float t : ts)
    {
        const float bests[] = {0.001f, FLT_MAX, t};
        for (const float best : bests)
            for (const uint32_t id : ids)
                for (const uint32_t best_id : best_ids)
                {
                    ++grid;
                    const bool b = r1_offer_better(t, id, best, best_id), r = rule(t, id, best, best_id);
                    const bool pre = t > 0.001f, below = t < FLT_MAX;
                    // the update predicate of the kernels, and the function under its precondition alone
                    if ((pre & below & b) != (pre & below & r))
                        report("update", t, id, best, best_id);
                    if ((pre & b) != (pre & r))
                        report("precondition", t, id, best, best_id);
                    // without the precondition the two agree wherever `best` is a number (r1_offer.h)
                    if (best == best)
                    {
                        ++grid_raw;
                        if (b != r)
                            report("raw", t, id, best, best_id);
                    }
                    grid_updates += (pre & below & r) ? 1 : 0;
                    // what keeps `t < FLT_MAX` a compare of its own: the "none" state loses to no t of FLT_MAX in the rule, and does in the key
                    if (bits_of(t) == bmax && bits_of(best) == bmax && best_id == 0xFFFFFFFFu)
                        none_state_flt_max += (b && !(below & b)) ? 1 : 0;
                }
    }
    rng_state = seed;
    unsigned long long updates = 0;
    for (unsigned long long i = 0; i < n_random; ++i)
    {
        // t > 0.001: bits in (bits(0.001), bits(+inf)]
        const uint32_t span = 0x7F800000u - b001;
        const float t = from_bits(b001 + 1u + rnd32() % span);
        const uint32_t how = rnd32() % 4u;
        float best;
        if (how == 0u)
            best = t;
        else if (how == 1u)
            best = FLT_MAX;
        else if (how == 2u)
            best = from_bits(bits_of(t) + (rnd32() % 5u) - 2u); // a neighbour of t, either side
        else
            best = from_bits(b001 + rnd32() % (bmax - b001 + 1u));
        if (!(best >= 0.001f) || best > FLT_MAX)
            best = FLT_MAX;
        const bool small = (rnd32() & 1u) != 0u;
        const uint32_t id = small ? rnd32() % 4u : rnd32(), best_id = small ? rnd32() % 4u : ((rnd32() & 7u) == 0u ? 0xFFFFFFFFu : rnd32());
        const bool b = r1_offer_better(t, id, best, best_id), r = rule(t, id, best, best_id);
        if (b != r)
            report("random", t, id, best, best_id);
        if (t == best)
            ++ties, tie_wins += r ? 1 : 0;
        updates += r ? 1 : 0;
    }
    // Sequences: the state a walk hands on after a run of offers — the header's update predicate and its settle step (after the run, and
    // sometimes in the middle of it: a walk carried over several calls) against the written-out update with `t < FLT_MAX`.  The walk starts
    // at "none" or, a query's, at a t_max with no index.  Form 2 may hold (FLT_MAX, id) on the way; what it hands on must be the same.
    const float vals[] = {FLT_MAX, FLT_MAX, from_bits(bmax - 1u), INFINITY, 1.0f, 2.0f, 0.001f, from_bits(b001 + 1u), 0.0005f, -1.0f, from_bits(0x7FC00000u), from_bits(0xFFC00000u)};
    const float starts[] = {FLT_MAX, FLT_MAX, FLT_MAX, from_bits(bmax - 1u), 1.5f, 2.0f};
    unsigned long long sequences = 0, held_flt_max = 0, ended_none = 0;
    for (unsigned long long i = 0; i < n_random; ++i, ++sequences)
    {
        float b0 = starts[rnd32() % 6u], b1 = b0;
        uint32_t i0 = 0xFFFFFFFFu, i1 = 0xFFFFFFFFu;
        const float first_best = b0;
        const uint32_t len = 1u + rnd32() % 6u;
        bool held = false;
        for (uint32_t k = 0; k < len; ++k)
        {
            const float t = (rnd32() & 3u) ? vals[rnd32() % 12u] : from_bits(b001 + 1u + rnd32() % (0x7F800000u - b001));
            const uint32_t id = rnd32() % 4u;
            volatile float vt = t;
            const bool u0 = (vt > 0.001f) & (vt < FLT_MAX) & rule(t, id, b0, i0);
            b0 = u0 ? t : b0, i0 = u0 ? id : i0;
            const bool u1 = r1_offer_update_form<R1_OFFER_FORM>(t, id, b1, i1);
            b1 = u1 ? t : b1, i1 = u1 ? id : i1;
            held |= bits_of(b1) == bmax && i1 != 0xFFFFFFFFu;
            if ((rnd32() & 3u) == 0u)
                i1 = r1_offer_settle_form<R1_OFFER_FORM>(b1, i1);
        }
        i1 = r1_offer_settle_form<R1_OFFER_FORM>(b1, i1);
        held_flt_max += held ? 1 : 0, ended_none += i0 == 0xFFFFFFFFu ? 1 : 0;
        if (bits_of(b0) != bits_of(b1) || i0 != i1)
            report("sequence", b1, i1, first_best, i0);
    }
    printf("sequences %llu\nsequences_that_held_flt_max %llu\nsequences_ending_none %llu\n", sequences, held_flt_max, ended_none);
    printf("grid_cases %llu\ngrid_raw_cases %llu\ngrid_updates %llu\nnone_state_flt_max %llu\nrandom_cases %llu\nrandom_updates %llu\nrandom_ties %llu\n"
           "random_tie_wins %llu\nform %d\nmismatches %llu\n",
           grid, grid_raw, grid_updates, none_state_flt_max, n_random, updates, ties, tie_wins, (int)R1_OFFER_FORM, mismatches);
    return mismatches ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "offer"))
        return run_offer(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1000000ull, argc > 3 ? strtoull(argv[3], nullptr, 10) : 1ull);
    fprintf(stderr, "usage: check_offer_host offer <random cases> <seed>\n");
    return 2;
}
