// resample_stream_check.cpp -- leaf_resample_stream_step_f32's arithmetic on the CPU, by the very functions the library calls
// (csrc/leaf_resample_stream.hpp for the position, csrc/leaf_resample.hpp for the outputs): one recording fed chunk by chunk, the
// outputs printed as tools/resample_check.cpp prints those of the whole recording.  Host only, no HIP:
//
//     g++ -std=c++17 -O1 -ffp-contract=off -I leaf_pytorch_amd/csrc tools/resample_stream_check.cpp -o /tmp/resample_stream_check
//     /tmp/resample_stream_check orig=44100 new=16000 pcm=1 seed=7 L=1000 chunks=0,1,300,5
//     /tmp/resample_stream_check hostile=1
//
// Arguments are key=value: orig new W (6) rolloff (0.99) pcm (0 / 1), the samples as x= or seed= and L= (exactly as resample_check),
// and chunks= a comma list of chunk sizes: the recording goes in by these sizes, what is left behind the list in one last chunk, and
// the stream ends WITH the last chunk (flush=1: with a step of its own behind it, without samples).  Lines:
//
//     plan o n width K H out_len
//     step i Tc hist_len shift phase n drop_samples       (one line per step: the record the plan fills)
//     y j bits q                                          (one line per output, as resample_check prints it)
//
// Each step stages nothing: an output reads its samples through the window coordinates of the step (+0.0f in front of the stream and
// behind what has arrived, the history, the chunk), which is what the kernel's staged window holds.  hostile=1 walks extreme positions
// and records through the plan and the step's checks, and reads every sample a passing record makes the kernel read or keep from
// exact-size arrays; built with -fsanitize=undefined,address every overflow or index outside an array is a report.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_resample_stream.hpp"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Table {
    ResamplePlan q;
    ResampleTableShape s;
    std::vector<int> words;
};

// the n outputs of one step, by the record (hist_len, shift, phase) and the two sources
static void step_outputs(const Table& t, const std::vector<float>& hist, const float* chunk, int Tc, int shift, int phase, long long n,
                         std::vector<float>& y) {
    const ResamplePlan& q = t.q;
    const int* k0s = t.words.data() + kResampleHeaderInts;
    const int* cnts = k0s + q.n;
    const float* taps = reinterpret_cast<const float*>(cnts + q.n);
    const int hist_len = (int)hist.size();
    for (long long j = 0; j < n; ++j) {
        const long long tt = phase + j, g = tt / q.n;
        const int p = (int)(tt - g * q.n);
        int k0 = k0s[p], cnt = cnts[p];
        resample_clamp_span(k0, cnt, q.K, t.s.stride);
        const float* h = taps + (size_t)p * t.s.stride;
        y.push_back(resample_output(k0, cnt, [h](int i) { return h[i]; }, [&](int k) {
            const long long s = resample_stream_source(g * q.o + k, shift, hist_len, Tc);
            return s < 0 ? 0.0f : (s < hist_len ? hist[(size_t)s] : chunk[s - hist_len]);
        }));
    }
}

static int hostile() {
    const int ratios[][2] = {{1, 1}, {3, 2}, {2, 3}, {441, 160}, {147, 160}, {3, 1}, {1, 3}, {65535, 65534}, {1, 65535}, {16, 1}};
    const int ints[] = {0, 1, -1, 2, 7, 40, 474, 475, 65535, 65536, 1 << 20, (1 << 20) + 1, INT_MAX, INT_MIN, INT_MAX - 1};
    unsigned long long passed = 0, seen = 0;
    for (const auto& ra : ratios) {
        ResamplePlan q;
        if (!resample_plan(ra[0], ra[1], 6, 0.99, q)) continue;
        const int H = q.K - 1;
        // records as a caller might hand them in: the checks decide, and what passes is read from exact-size arrays
        std::vector<int> hists(ints, ints + sizeof(ints) / sizeof(ints[0]));
        hists.push_back(H);
        hists.push_back(H + 1);
        for (int hist_len : hists)
            for (int Tc : ints)
                for (int shift : {0, 1, -1, q.width, q.width + 1, INT_MAX})
                    for (int phase : {0, 1, -1, q.n - 1, q.n, INT_MAX})
                        for (int end : {0, 1, 2}) {
                            // (long chunks at the two ends of the history and of the shift only: the walk stays short)
                            if (Tc > 4096 && Tc <= kResampleStreamMaxChunk && !((hist_len == 0 || hist_len == H) && (shift == 0 || shift == q.width)))
                                continue;
                            const bool ok_range = hist_len >= 0 && hist_len <= H && shift >= 0 && shift <= q.width && phase >= 0 && phase < q.n &&
                                                  Tc >= 0 && Tc <= kResampleStreamMaxChunk && (end & ~1) == 0;
                            long long n = 0, drop = 0;
                            if (ok_range) {
                                const ResampleStreamMove m = resample_stream_move(q, ResampleStreamPos{hist_len, shift, phase}, Tc, end != 0);
                                n = m.n;
                                drop = m.drop;
                                if (m.drop < 0 || m.drop > (long long)hist_len + Tc || m.next.shift < 0 || m.next.shift > q.width ||
                                    m.next.phase < 0 || m.next.phase >= q.n || m.next.hist_len < 0 || m.n < 0) {
                                    std::fprintf(stderr, "the move left its ranges: %d:%d hist=%d Tc=%d shift=%d phase=%d end=%d\n", ra[0], ra[1],
                                                 hist_len, Tc, shift, phase, end);
                                    return 1;
                                }
                            }
                            for (long long nn : {n, n + 1, n - 1, 0ll, (long long)INT_MAX})
                                for (long long dd : {drop, drop + 1, -1ll, 0ll, (long long)INT_MAX}) {
                                    if (nn < INT_MIN || nn > INT_MAX) continue;
                                    const int n_max = nn > 0 ? (int)nn : 0;
                                    const int bad = resample_stream_slot_bad(q, hist_len, Tc, 0, shift, phase, (int)nn, (int)dd, end, n_max);
                                    if (bad) continue;
                                    if (!ok_range || nn != n) {
                                        std::fprintf(stderr, "a bad record passed: %d:%d hist=%d Tc=%d shift=%d phase=%d end=%d n=%lld\n", ra[0], ra[1],
                                                     hist_len, Tc, shift, phase, end, nn);
                                        return 1;
                                    }
                                    ++passed;
                                    // what the kernel reads for the outputs and keeps for the next step, from exact-size arrays
                                    std::vector<float> hist((size_t)hist_len, 1.0f), chunk((size_t)Tc, 1.0f), next((size_t)H, 0.0f);
                                    const long long Lv = (long long)hist_len + Tc;
                                    for (long long j = 0; j < nn; j += (nn > 64 ? nn / 64 : 1)) {
                                        const long long tt = phase + j, g = tt / q.n;
                                        for (int k = 0; k < q.K; k += (q.K > 64 ? q.K / 64 : 1)) {
                                            const long long s = resample_stream_source(g * q.o + k, shift, hist_len, Tc);
                                            if (s >= 0) seen += (unsigned long long)(s < hist_len ? hist[(size_t)s] : chunk[(size_t)(s - hist_len)]);
                                        }
                                    }
                                    if (!end)
                                        for (long long e = 0; e < Lv - dd; ++e) {
                                            const long long v = dd + e;
                                            next[(size_t)e] = v < hist_len ? hist[(size_t)v] : chunk[(size_t)(v - hist_len)];
                                        }
                                }
                        }
        // counts at the edges of what a position can be
        for (long long Lv : {0ll, 1ll, (long long)H, (long long)H + kResampleStreamMaxChunk})
            for (int phase : {0, q.n - 1})
                for (int end : {0, 1}) seen += (unsigned long long)resample_stream_count(q, q.width, Lv, phase, end != 0);
    }
    std::printf("hostile ok %llu %llu\n", passed, seen);
    return 0;
}

int main(int argc, char** argv) {
    int orig = 3, fresh = 2, W = 6, pcm = 0, run_hostile = 0, flush = 0;
    double rolloff = 0.99;
    long long L = -1;
    unsigned long long seed = 0;
    std::string xs, cs;
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
        else if (key == "hostile") run_hostile = std::atoi(val);
        else if (key == "flush") flush = std::atoi(val);
        else if (key == "seed") seed = std::strtoull(val, nullptr, 0);
        else if (key == "L") L = std::strtoll(val, nullptr, 0);
        else if (key == "x") xs = val;
        else if (key == "chunks") cs = val;
        else { std::fprintf(stderr, "unknown key: %s\n", key.c_str()); return 2; }
    }
    if (run_hostile) return hostile();
    if (orig <= 0 || fresh <= 0 || W < 1 || !(rolloff > 0.0 && rolloff <= 1.0)) { std::fprintf(stderr, "bad shape\n"); return 3; }
    Table t;
    if (!resample_plan(orig, fresh, W, rolloff, t.q)) { std::fprintf(stderr, "unsupported\n"); return 4; }
    t.s = resample_table_shape(t.q);
    bool win = false, taps = false;
    if (t.s.bytes != 0) resample_paths(t.q, t.s, win, taps);
    if (t.s.bytes == 0 || !win) { std::fprintf(stderr, "unsupported\n"); return 4; }   // the step's own refusal
    t.words.resize((size_t)(t.s.bytes / 4));
    resample_table_fill(t.q, t.s, t.words.data());

    std::vector<float> x;
    if (L >= 0) {                                                         // resample_check's generator
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
    std::vector<long long> sizes;
    for (const char* c = cs.c_str(); *c;) {
        char* end;
        const long long v = std::strtoll(c, &end, 0);
        if (end == c) break;
        sizes.push_back(v < 0 ? 0 : v);
        c = *end == ',' ? end + 1 : end;
    }

    const ResamplePlan& q = t.q;
    std::printf("plan %d %d %d %d %d %lld\n", q.o, q.n, q.width, q.K, q.K - 1, resample_length((long long)x.size(), q.o, q.n));
    std::vector<float> hist, y;
    ResampleStreamPos at = resample_stream_begin(q);
    size_t fed = 0;
    int step = 0;
    for (size_t i = 0;; ++i) {
        const bool last = i >= sizes.size();
        size_t Tc = last ? x.size() - fed : (size_t)sizes[i];
        if (Tc > x.size() - fed) Tc = x.size() - fed;
        if (Tc > (size_t)kResampleStreamMaxChunk) Tc = (size_t)kResampleStreamMaxChunk;
        const bool final_samples = fed + Tc == x.size() && last;
        const bool end = final_samples && !flush;
        const ResampleStreamMove m = resample_stream_move(q, at, (int)Tc, end);
        if (resample_stream_slot_bad(q, at.hist_len, (int)Tc, 0, at.shift, at.phase, (int)m.n, (int)m.drop, end, INT_MAX)) {
            std::fprintf(stderr, "the plan's own record fails the step's checks\n");
            return 5;
        }
        std::printf("step %d %zu %d %d %d %lld %lld\n", step++, Tc, at.hist_len, at.shift, at.phase, m.n, m.drop);
        step_outputs(t, hist, x.data() + fed, (int)Tc, at.shift, at.phase, m.n, y);
        std::vector<float> next;
        if (!end)
            for (long long v = m.drop; v < (long long)hist.size() + (long long)Tc; ++v)
                next.push_back(v < (long long)hist.size() ? hist[(size_t)v] : x[fed + (size_t)(v - (long long)hist.size())]);
        hist.swap(next);
        at = m.next;
        fed += Tc;
        if (final_samples) break;
    }
    if (flush) {
        const ResampleStreamMove m = resample_stream_move(q, at, 0, true);
        std::printf("step %d 0 %d %d %d %lld %lld\n", step, at.hist_len, at.shift, at.phase, m.n, m.drop);
        step_outputs(t, hist, nullptr, 0, at.shift, at.phase, m.n, y);
    }
    for (size_t j = 0; j < y.size(); ++j) std::printf("y %zu %08x %d\n", j, bits(y[j]), (int)resample_quantize(y[j]));
    return 0;
}
