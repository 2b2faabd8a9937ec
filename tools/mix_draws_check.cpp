// mix_draws_check.cpp -- perm and lam of leaf_draw_mixup computed on the CPU by the very functions the kernel calls
// (csrc/leaf_mix_draws.hpp: draw_mix_clip, draw_mix_lam), printed as text.  Host only, no HIP:
//
//     g++ -std=c++17 -O1 -ffp-contract=off -I leaf_pytorch_amd/csrc tools/mix_draws_check.cpp -o /tmp/mix_draws_check
//     /tmp/mix_draws_check B=5 alpha=0.3 seed=7 base=0 step=2 steps=1
//     /tmp/mix_draws_check alpha=0.01 words=0:0,0:2147483648,4294967295:5
//
// Arguments are key=value, in any order: B (1), alpha (1.0), seed (0), base (0), step (0), steps (1: how many consecutive steps), and
// words= (a comma list of r0:r1 pairs).  Without words: one line per clip and step,
//
//     step b perm[b] lam[b]
//
// perm[k] being the b with the k-th smallest key (std::sort of the header's keys: the definition is the order, not the method) and
// lam the hexadecimal bit pattern of the float32.  With words: one line `r0 r1 lam` per pair, the weight draw_mix_lam gives for
// these two words in place of Philox's.  tests/test_host_mix_draws.py compares the lines with its NumPy oracle.
//
// B outside [1, 4096] is refused as the entry refuses it (exit status 3).  alpha is NOT checked: built with
// -fsanitize=undefined,address the program walks the header over an alpha the entry would never launch (NaN, 0, negative, infinite).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_mix_draws.hpp"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    int B = 1;
    double alpha = 1.0;
    unsigned long long seed = 0, base = 0, step = 0, steps = 1;
    const char* words = nullptr;
    for (int a = 1; a < argc; ++a) {
        const char* eq = std::strchr(argv[a], '=');
        if (!eq) { std::fprintf(stderr, "not key=value: %s\n", argv[a]); return 2; }
        const std::string key(argv[a], (size_t)(eq - argv[a]));
        const char* val = eq + 1;
        if (key == "B") B = std::atoi(val);
        else if (key == "alpha") alpha = std::strtod(val, nullptr);
        else if (key == "seed") seed = std::strtoull(val, nullptr, 0);
        else if (key == "base") base = std::strtoull(val, nullptr, 0);
        else if (key == "step") step = std::strtoull(val, nullptr, 0);
        else if (key == "steps") steps = std::strtoull(val, nullptr, 0);
        else if (key == "words") words = val;
        else { std::fprintf(stderr, "unknown key: %s\n", key.c_str()); return 2; }
    }
    if (words) {
        for (const char* s = words; *s;) {
            char* end;
            const unsigned long long r0 = std::strtoull(s, &end, 0);
            if (end == s || *end != ':') { std::fprintf(stderr, "words: r0:r1[,r0:r1...]\n"); return 2; }
            s = end + 1;
            const unsigned long long r1 = std::strtoull(s, &end, 0);
            if (end == s || r0 > 0xFFFFFFFFull || r1 > 0xFFFFFFFFull) { std::fprintf(stderr, "words: r0:r1[,r0:r1...]\n"); return 2; }
            s = *end == ',' ? end + 1 : end;
            std::printf("%llu %llu %08x\n", r0, r1, bits(draw_mix_lam((unsigned)r0, (unsigned)r1, alpha)));
        }
        return 0;
    }
    if (B < 1 || B > kMixMaxBatch) {
        std::fprintf(stderr, "refused: a B leaf_draw_mixup answers with a status\n");
        return 3;
    }
    std::vector<unsigned long long> keys((size_t)B);      // exactly the sizes the entry documents: an index outside one is a report
    std::vector<float> lam((size_t)B);
    for (unsigned long long n = 0; n < steps; ++n) {
        const unsigned long long s = step + n;
        for (int b = 0; b < B; ++b) {
            const MixDraw d = draw_mix_clip(seed, base, s, B, b, alpha);
            keys[(size_t)b] = d.key;
            lam[(size_t)b] = d.lam;
        }
        std::sort(keys.begin(), keys.end());
        for (int b = 0; b < B; ++b) std::printf("%llu %d %u %08x\n", s, b, (unsigned)keys[(size_t)b], bits(lam[(size_t)b]));
    }
    return 0;
}
