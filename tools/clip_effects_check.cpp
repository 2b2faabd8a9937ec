// clip_effects_check.cpp -- leaf_clip_effects_f32 computed on the CPU by the sequential definition, from the very functions the
// kernel calls (csrc/leaf_clip_effects.hpp: fx_clip_sequential and the steps under it), printed as text.  Host only, no HIP:
//
//     g++ -std=c++17 -O1 -ffp-contract=off -I leaf_pytorch_amd/csrc tools/clip_effects_check.cpp -o /tmp/clip_effects_check
//     /tmp/clip_effects_check plans.txt          (or: /tmp/clip_effects_check - < plans.txt)
//     /tmp/clip_effects_check hostile
//     /tmp/clip_effects_check time 16000 64      (seconds per clip of S samples at 16 kHz, over that many clips, one core)
//
// The plan file is whitespace-separated words; every float32 is the hexadecimal pattern of its bits:
//
//     sample_rate wet B S
//     then per clip:  factor feedback damp c0 c1 c2 c3 c4 c5 c6 c7   x[0] ... x[S-1]
//
// factor below 0 skips ClipValue, c0 <= 0 the reverb; the other lengths are clamped into [1, cap] as the kernel clamps them.  The
// output is one line per clip, y[0] ... y[S-1] as bit patterns.  tests/test_host_clip_effects.py compares the lines with its NumPy
// oracle, bit for bit.  A sample rate the entry refuses -- a length below 1, or lines beyond the LDS budget -- is refused here too
// (exit status 3).
//
// `hostile` walks the definition over plans no validated caller sends: lengths 0, negative and INT_MAX, S = 0 and S = 1, at 8 kHz
// and 48 kHz.  Every buffer has exactly the documented size, so built with -fsanitize=undefined,address an index outside one is a
// report.
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_clip_effects.hpp"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float unbits(unsigned u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static bool lengths_for(int sample_rate, FxLengths& L) {
    return fx_lengths(sample_rate, L) && fx_clips_per_group(L, 256) >= 1;
}

// one clip through the definition, in buffers of exactly the documented sizes
static std::vector<float> run_clip(const std::vector<float>& x, float factor, float feedback, float damp, const int* comb, const FxLengths& L,
                                   float wet) {
    std::vector<float> y(x.size()), lines((size_t)fx_clip_floats(L) - (size_t)L.allpass[0]);
    fx_clip_sequential(x.data(), y.data(), (long long)x.size(), factor, feedback, damp, comb, L, wet, lines.data());
    return y;
}

static int hostile() {
    const int rates[] = {8000, 48000};
    const int plans[][kFxCombs] = {{INT_MAX, 0, -7, INT_MAX, 1, 0, INT_MIN, 1000000000},
                                   {1, 1, 1, 1, 1, 1, 1, 1},
                                   {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX},
                                   {0, 5, 5, 5, 5, 5, 5, 5},
                                   {-1, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX}};
    const size_t sizes[] = {0, 1, 2, 700, 5000};
    unsigned long long sum = 0;
    for (int rate : rates) {
        FxLengths L;
        if (!lengths_for(rate, L)) return 1;
        for (const auto& plan : plans)
            for (size_t S : sizes)
                for (float factor : {-1.0f, 0.0f, 0.5f}) {
                    std::vector<float> x(S);
                    for (size_t n = 0; n < S; ++n) x[n] = (float)((int)((n * 2654435761u) >> 20 & 0xfff) - 2048) / 2048.0f;
                    const std::vector<float> y = run_clip(x, factor, 0.98f, 0.5f, plan, L, 0.015f);
                    for (float v : y) {
                        if (!(v == v) || v > 1e30f || v < -1e30f) {
                            std::fprintf(stderr, "hostile: a sample is not finite\n");
                            return 1;
                        }
                        sum += bits(v);
                    }
                }
        const std::vector<float> none = run_clip(std::vector<float>(3, 0.25f), 0.5f, 0.5f, 0.5f, nullptr, L, 0.015f);
        sum += bits(none[0]);
    }
    std::printf("hostile ok %llu\n", sum);
    return 0;
}

static int timing(int S, int clips) {
    FxLengths L;
    if (S < 1 || clips < 1 || !lengths_for(16000, L)) return 2;
    const int comb[kFxCombs] = {223, 237, 255, 271, 284, 298, 311, 323};   // room_scale 50 at 16 kHz
    std::vector<float> x((size_t)S);
    for (int n = 0; n < S; ++n) x[(size_t)n] = (float)((int)(((unsigned)n * 2654435761u) >> 20 & 0xfff) - 2048) / 2048.0f;
    unsigned long long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int c = 0; c < clips; ++c) {
        x[0] = (float)c;
        sum += bits(run_clip(x, 0.1f, 0.88f, 0.3f, comb, L, 0.015f)[(size_t)S - 1]);
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%d clips of %d samples: %.1f us per clip on one core (checksum %llu)\n", clips, S, 1e6 * s / clips, sum);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "hostile") == 0) return hostile();
    if (argc == 4 && std::strcmp(argv[1], "time") == 0) return timing(std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc != 2) {
        std::fprintf(stderr, "usage: clip_effects_check <plans.txt | - | hostile | time S clips>\n");
        return 2;
    }
    FILE* in = std::strcmp(argv[1], "-") == 0 ? stdin : std::fopen(argv[1], "r");
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int sample_rate = 0, B = 0;
    long long S = -1;
    unsigned wet = 0;
    if (std::fscanf(in, "%d %x %d %lld", &sample_rate, &wet, &B, &S) != 4 || B < 0 || S < 0) {
        std::fprintf(stderr, "header: sample_rate wet B S\n");
        return 2;
    }
    FxLengths L;
    if (!lengths_for(sample_rate, L)) {
        std::fprintf(stderr, "refused: a sample rate leaf_clip_effects_f32 answers with a status\n");
        return 3;
    }
    for (int b = 0; b < B; ++b) {
        unsigned w[3];
        int comb[kFxCombs];
        if (std::fscanf(in, "%x %x %x", &w[0], &w[1], &w[2]) != 3) return 2;
        for (int i = 0; i < kFxCombs; ++i)
            if (std::fscanf(in, "%d", &comb[i]) != 1) return 2;
        std::vector<float> x((size_t)S);
        for (long long n = 0; n < S; ++n) {
            unsigned u;
            if (std::fscanf(in, "%x", &u) != 1) return 2;
            x[(size_t)n] = unbits(u);
        }
        const std::vector<float> y = run_clip(x, unbits(w[0]), unbits(w[1]), unbits(w[2]), comb, L, unbits(wet));
        std::string line;
        line.reserve(y.size() * 9 + 1);
        char word[16];
        for (size_t n = 0; n < y.size(); ++n) {
            std::snprintf(word, sizeof word, n ? " %08x" : "%08x", bits(y[n]));
            line += word;
        }
        std::puts(line.c_str());
    }
    if (in != stdin) std::fclose(in);
    return 0;
}
