// resample_check.cpp -- leaf_resample_f32's arithmetic on the CPU, by the very functions the kernel calls (csrc/leaf_resample.hpp): the
// table and the outputs of one recording, printed as text.  Host only, no HIP:
//
//     g++ -std=c++17 -O1 -ffp-contract=off -I leaf_pytorch_amd/csrc tools/resample_check.cpp -o /tmp/resample_check
//     /tmp/resample_check orig=3 new=2 x=0.5,-0.25,1,0,0.125
//     /tmp/resample_check orig=44100 new=16000 pcm=1 seed=7 L=1000
//     /tmp/resample_check hostile=1
//
// Arguments are key=value, in any order: orig new W (6) rolloff (0.99) pcm (0: float32 samples, 1: int16) and the samples -- x= a comma
// list (floats, hexadecimal floats included; integers with pcm=1) or seed= and L= (a 64-bit LCG: int16 over the full range, float32
// uniform in [-1, 1) on a 2^-24 grid) -- and table=0 to leave the table lines out.  Floats are printed as the hexadecimal bit pattern
// of the float32:
//
//     plan o n width K stride bytes taps_in_lds window_in_lds out_len
//     phase p k0 cnt h...                  (one line per phase: the span's taps)
//     y j bits q                           (one line per output: the float32 output and its int16 quantisation)
//
// tests/test_host_resample.py compares the lines with its NumPy oracle, tests/test_gpu_resample.py the kernel's bits with them.
// hostile=1 pushes records far outside any store through the clamps (offsets and lengths negative, near 2^63, out_off beyond
// out_total) and runs the staged-window arithmetic of a tile on them; built with -fsanitize=undefined,address every overflow or index
// outside an array is a report.
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_resample.hpp"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

// one recording through the per-output function, samples outside [0, L) zero: what a tile computes, without the tiling
static std::vector<float> resample_all(const ResamplePlan& q, const ResampleTableShape& s, const std::vector<int>& table,
                                       const std::vector<float>& x) {
    const int* k0s = table.data() + kResampleHeaderInts;
    const int* cnts = k0s + q.n;
    const float* taps = reinterpret_cast<const float*>(cnts + q.n);
    const long long L = (long long)x.size(), out_len = resample_length(L, q.o, q.n);
    std::vector<float> y((size_t)out_len);
    for (long long j = 0; j < out_len; ++j) {
        const long long i = j / q.n;
        const int p = (int)(j % q.n);
        int k0 = k0s[p], cnt = cnts[p];
        resample_clamp_span(k0, cnt, q.K, s.stride);
        const float* h = taps + (size_t)p * s.stride;
        const long long first = i * q.o - q.width;
        y[(size_t)j] = resample_output(k0, cnt, [h](int t) { return h[t]; }, [&](int k) {
            const long long at = first + k;
            return at >= 0 && at < L ? x[(size_t)at] : 0.0f;
        });
    }
    return y;
}

static int hostile() {
    const long long big = LLONG_MAX, small = LLONG_MIN;
    const long long offs[] = {0, 1, -1, 5, 1000, big, big - 1, small, small + 1, 1ll << 62, -(1ll << 62), 4294967296ll};
    const int lens[] = {0, 1, -1, 7, INT_MAX, INT_MIN, 1000, 65536};
    const long long totals[] = {0, 1, 17, 1000, big};
    const int ratios[][2] = {{1, 1}, {3, 2}, {2, 3}, {441, 160}, {65535, 1}, {1, 65535}, {65535, 65534}};
    const long long store_len = 1000;
    std::vector<float> store((size_t)store_len, 1.0f);
    unsigned long long seen = 0;
    for (const auto& ra : ratios)
        for (long long off : offs)
            for (int len : lens)
                for (long long ooff : offs)
                    for (long long total : totals) {
                        const ResampleRecord r = resample_record(off, len, store_len, ooff, total, ra[0], ra[1]);
                        if (r.off < 0 || r.off > store_len || r.L < 0 || r.off + r.L > store_len || r.out_off < 0 || r.out_off > total ||
                            r.out_len < 0 || r.out_off + r.out_len > total) {
                            std::fprintf(stderr, "a clamp failed: off=%lld len=%d out_off=%lld total=%lld\n", off, len, ooff, total);
                            return 1;
                        }
                        for (long long s = r.off; s < r.off + r.L; s += 97) seen += (unsigned long long)store[(size_t)s];   // the reads a kernel would make
                    }
    for (long long L : {small, -1ll, 0ll, 1ll, (1ll << 31) - 1, 1ll << 40, big - 1, big})
        for (const auto& ra : ratios) seen += (unsigned long long)resample_length(L, ra[0], ra[1]);
    // spans from a table that lies: the clamp keeps them inside [0, K)
    const int spans[][2] = {{0, 0}, {-1, 5}, {INT_MIN, INT_MAX}, {INT_MAX, INT_MAX}, {INT_MAX, INT_MIN}, {3, 100}, {100, 3}};
    for (const auto& sp : spans)
        for (int K : {1, 13, 100})
            for (int stride : {1, 13, 35}) {
                int k0 = sp[0], cnt = sp[1];
                resample_clamp_span(k0, cnt, K, stride);
                if (cnt < 0 || cnt > stride || k0 < 0 || k0 + cnt > K) {
                    std::fprintf(stderr, "the span clamp failed: %d %d K=%d stride=%d\n", sp[0], sp[1], K, stride);
                    return 1;
                }
            }
    // plans at the edges of what the entry takes
    for (const auto& ra : ratios) {
        ResamplePlan q;
        if (!resample_plan(ra[0], ra[1], 6, 0.99, q)) continue;
        const ResampleTableShape s = resample_table_shape(q);
        seen += (unsigned long long)s.bytes + (unsigned long long)resample_window_samples(q);
    }
    ResamplePlan q;
    seen += resample_plan(INT_MAX, INT_MAX - 1, 6, 0.99, q) ? 1 : 0;      // refused: the reduced ratio
    seen += resample_plan(3, 2, INT_MAX, 1e-300, q) ? 1 : 0;              // refused: the width
    seen += resample_plan(65535, 1, INT_MAX, 1.0, q) ? 1 : 0;
    std::printf("hostile ok %llu\n", seen);
    return 0;
}

int main(int argc, char** argv) {
    int orig = 3, fresh = 2, W = 6, pcm = 0, show_table = 1, run_hostile = 0;
    double rolloff = 0.99;
    long long L = -1;
    unsigned long long seed = 0;
    std::string xs;
    for (int a = 1; a < argc; ++a) {
        const char* eq = std::strchr(argv[a], '=');
        if (!eq) { std::fprintf(stderr, "not key=value: %s\n", argv[a]); return 2; }
        const std::string key(argv[a], (size_t)(eq - argv[a]));
        const char* val = eq + 1;
        if (key == "orig") orig = std::atoi(val);
        else if (key == "new") fresh = std::atoi(val);
        else if (key == "W") W = std::atoi(val);
        else if (key == "rolloff") rolloff = std::strtod(val, nullptr);
        else if (key == "pcm") pcm = std::atoi(val);
        else if (key == "table") show_table = std::atoi(val);
        else if (key == "hostile") run_hostile = std::atoi(val);
        else if (key == "seed") seed = std::strtoull(val, nullptr, 0);
        else if (key == "L") L = std::strtoll(val, nullptr, 0);
        else if (key == "x") xs = val;
        else { std::fprintf(stderr, "unknown key: %s\n", key.c_str()); return 2; }
    }
    if (run_hostile) return hostile();
    // the entry's own refusals (csrc/inst_resample.hip): nothing below runs on arguments it would not take
    if (orig <= 0 || fresh <= 0 || W < 1 || !(rolloff > 0.0 && rolloff <= 1.0)) { std::fprintf(stderr, "bad shape\n"); return 3; }
    ResamplePlan q;
    if (!resample_plan(orig, fresh, W, rolloff, q)) { std::fprintf(stderr, "unsupported\n"); return 4; }
    const ResampleTableShape s = resample_table_shape(q);
    if (s.bytes == 0) { std::fprintf(stderr, "unsupported\n"); return 4; }
    std::vector<int> table((size_t)(s.bytes / 4));
    resample_table_fill(q, s, table.data());

    std::vector<float> x;
    if (L >= 0) {                                                         // a 64-bit LCG (Knuth's MMIX constants), the high bits
        unsigned long long st = seed;
        for (long long i = 0; i < L; ++i) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            if (pcm) x.push_back(resample_widen((short)((int)(st >> 48) - 32768)));
            else x.push_back((float)((double)(long long)(st >> 39) * 0x1p-24 - 1.0));
        }
    } else {
        const char* c = xs.c_str();
        while (*c) {
            char* end;
            const double v = std::strtod(c, &end);
            if (end == c) break;
            x.push_back(pcm ? resample_widen((short)(long long)v) : (float)v);
            c = *end == ',' ? end + 1 : end;
        }
    }

    bool win, taps;
    resample_paths(q, s, win, taps);
    const std::vector<float> y = resample_all(q, s, table, x);
    std::printf("plan %d %d %d %d %d %lld %d %d %zu\n", q.o, q.n, q.width, q.K, s.stride, s.bytes, taps ? 1 : 0, win ? 1 : 0, y.size());
    if (show_table) {
        const int* k0s = table.data() + kResampleHeaderInts;
        const int* cnts = k0s + q.n;
        const float* h = reinterpret_cast<const float*>(cnts + q.n);
        for (int p = 0; p < q.n; ++p) {
            std::printf("phase %d %d %d", p, k0s[p], cnts[p]);
            for (int i = 0; i < cnts[p]; ++i) std::printf(" %08x", bits(h[(size_t)p * s.stride + i]));
            std::printf("\n");
        }
    }
    for (size_t j = 0; j < y.size(); ++j) std::printf("y %zu %08x %d\n", j, bits(y[j]), (int)resample_quantize(y[j]));
    return 0;
}
