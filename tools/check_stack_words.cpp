// tools/check_stack_words.cpp — runs rays1bench_amd/csrc/r1_stack_words.h on the host (tests/test_stack_words_host.py) against the forms it
// replaces, written out here:
//   * r1_stack_word / r1_stack_shift against sp / 3 and 10 (sp % 3) for every sp in [0, 51], and the quotient as far as the header claims it;
//   * a path's pushes — r1_stack_push_word: a word opened with the pad in its upper slots, later entries put in — against the plain merge into a word of
//     arbitrary old contents: the slots taken agree, the slots above the top entry hold the pad;
//   * the padded word's fold — every slot multiplies, the pad's row being {0, 1, 1, 1} — against the select form (a slot above the top entry
//     multiplies by a selected 1.0f), bit for bit, on 10^6 random albedos, radiances and fills (xorshift64: the same cases every run).
// Prints "name value" lines; exit status 1 and "MISMATCH ..." lines on stderr (the first few) where the two sides differ.
// A stand-alone program: it may be built with -fsanitize=address,undefined as it is.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../rays1bench_amd/csrc/r1_stack_words.h"

static unsigned long long mismatches = 0;
static void report(const char *what, const unsigned long long at)
{
    if (mismatches++ < 10)
        fprintf(stderr, "MISMATCH %s at %llu\n", what, at);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
static uint32_t bits(const float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}
// an albedo or a radiance: mostly in [0, 2), sometimes any finite or infinite bit pattern (a NaN compares by its bits too: x * 1.0f keeps them)
static float draw()
{
    const uint64_t r = rng();
    if ((r & 15u) == 0u)
    {
        const uint32_t u = (uint32_t)(r >> 32);
        float f;
        memcpy(&f, &u, sizeof f);
        return f == f ? f : 0.5f; // (no NaN: the GPU's and the host's NaN payload rules are not what this checks)
    }
    return (float)((r >> 40) & 0xFFFFFFu) * (2.0f / 16777216.0f);
}

int main()
{
    // ---- quotient and shift ----
    unsigned long long slots = 0, quotients = 0;
    for (uint32_t sp = 0; sp <= 51; ++sp, ++slots)
    {
        const uint32_t w = r1_stack_word(sp), sh = r1_stack_shift(sp, w);
        if (w != sp / 3u)
            report("word", sp);
        if (sh != 10u * (sp % 3u))
            report("shift", sp);
    }
    for (uint32_t sp = 0; sp < 32768u; ++sp, ++quotients)
        if (r1_stack_word(sp) != sp / 3u)
            report("word beyond the stack", sp);

    // ---- pushes: opened and merged words against the plain merge ----
    unsigned long long pushes = 0;
    for (int round = 0; round < 20000; ++round)
    {
        uint32_t padded[17], plain[17];
        for (int w = 0; w < 17; ++w)
            padded[w] = plain[w] = (uint32_t)rng(); // whatever an earlier path left
        const uint32_t depth = 1u + (uint32_t)(rng() % 51u);
        for (uint32_t sp = 0; sp < depth; ++sp, ++pushes)
        {
            const uint32_t idx = (uint32_t)(rng() % 1023u); // 0 .. 1022
            const uint32_t w = r1_stack_word(sp), sh = r1_stack_shift(sp, w);
            padded[w] = r1_stack_push_word(padded[w], sh, idx);
            if (sh == 0u && padded[w] != r1_stack_open(idx))
                report("open", (unsigned long long)round * 64u + sp);
            plain[sp / 3u] = (plain[sp / 3u] & ~(0x3FFu << (10u * (sp % 3u)))) | (idx << (10u * (sp % 3u)));
            // every entry so far reads the same from both; the slots of the top word above the top entry hold the pad
            for (uint32_t e = 0; e <= sp; ++e)
                if (((padded[e / 3u] >> (10u * (e % 3u))) & 0x3FFu) != ((plain[e / 3u] >> (10u * (e % 3u))) & 0x3FFu))
                    report("entry", (unsigned long long)round * 64u + e);
            for (uint32_t e = sp + 1u; e < 3u * (sp / 3u + 1u); ++e)
                if (((padded[e / 3u] >> (10u * (e % 3u))) & 0x3FFu) != R1_STACK_PAD_INDEX)
                    report("pad", (unsigned long long)round * 64u + e);
        }
    }

    // ---- the fold: padded word against the select form ----
    unsigned long long folds = 0;
    const float identity[3] = {1.0f, 1.0f, 1.0f}; // albedo rgb of the pad's row {0, 1, 1, 1}
    unsigned long long by_fill[3] = {0, 0, 0};
    for (int i = 0; i < 1000000; ++i, ++folds)
    {
        float a[3][3], col[3], want[3];
        for (int s = 0; s < 3; ++s)
            for (int c = 0; c < 3; ++c)
                a[s][c] = draw();
        for (int c = 0; c < 3; ++c)
            col[c] = want[c] = draw();
        const int j = (int)(rng() % 3u); // the top entry's slot: slots above it are empty
        ++by_fill[j];
        // the select form (shade_level before the pad): u2 = j >= 2, u1 = j >= 1
        const bool u2 = j >= 2, u1 = j >= 1;
        for (int c = 0; c < 3; ++c)
            want[c] = (u2 ? a[2][c] : 1.0f) * want[c];
        for (int c = 0; c < 3; ++c)
            want[c] = (u1 ? a[1][c] : 1.0f) * want[c];
        for (int c = 0; c < 3; ++c)
            want[c] = a[0][c] * want[c];
        // the padded form: an empty slot's gather returns the pad's row
        r1_stack_fold(col, u2 ? a[2] : identity, u1 ? a[1] : identity, a[0]);
        for (int c = 0; c < 3; ++c)
            if (bits(col[c]) != bits(want[c]))
                report("fold", (unsigned long long)i);
    }

    printf("slots %llu\nquotients %llu\npushes %llu\nfolds %llu\nfill0 %llu\nfill1 %llu\nfill2 %llu\nmismatches %llu\n", slots, quotients, pushes, folds, by_fill[0],
           by_fill[1], by_fill[2], mismatches);
    return mismatches ? 1 : 0;
}
