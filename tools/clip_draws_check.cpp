// clip_draws_check.cpp -- the plan of leaf_draw_clip_plan computed on the CPU by the very functions the kernel calls
// (csrc/leaf_clip_draws.hpp: draw_plan_clip), printed as text.  Host only, no HIP:
//
//     g++ -std=c++17 -O1 -ffp-contract=off -I leaf_pytorch_amd/csrc tools/clip_draws_check.cpp -o /tmp/clip_draws_check
//     /tmp/clip_draws_check B=5 S=64 lengths=1,7,63,64,65,197 index=0,1,2,3,4 M=3 tperc=0.2 nlengths=5,64,129 gaussp=0.5 seed=7 step=2
//
// Arguments are key=value, in any order (defaults in main below): B S train mode0 mode1 M wrap gainp glo ghi tperc noisep snrlo snrhi
// gaussp alo ahi seed base step, lengths= and nlengths= (comma lists; no nlengths: no noise group), and index= (B entries) or order=
// (any number: clip b is order[(step B + b) mod N]).  The recordings lie back to back: offsets are the lengths' running sum.  One line
// per clip, floats as the hexadecimal bit pattern of the float32:
//
//     b index rec_off rec_len start pad_mode gain | t0 n (M pairs) | noise_off noise_len noise_start noise_pad_mode c c' | amp stream
//
// tests/test_host_clip_draws.py compares the lines with its NumPy oracle.  Built with -fsanitize=undefined,address the same program
// walks hostile constants: every array below has exactly the size the entry documents, so an index outside one is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "leaf_clip_draws.hpp"

static std::vector<long long> list_of(const char* s) {
    std::vector<long long> v;
    while (*s) {
        char* end;
        const long long x = std::strtoll(s, &end, 0);
        if (end == s) break;
        v.push_back(x);
        s = *end == ',' ? end + 1 : end;
    }
    return v;
}

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    DrawParams p{};
    p.B = 1; p.k.S = 16; p.k.train = 1; p.k.mode0 = 2; p.k.mode1 = 1; p.k.M = 0;
    p.k.wrap_pad_prob = 0.5; p.k.gain_prob = 0.25; p.k.gain_lo = -18.0; p.k.gain_hi = 6.0; p.k.time_perc = 0.0;
    p.k.noise_prob = 0.5; p.k.snr_lo = 10.0; p.k.snr_hi = 25.0; p.k.gauss_prob = 0.0; p.k.amp_lo = 0.001; p.k.amp_hi = 0.015;
    unsigned long long step = 0;
    std::vector<long long> lengths{16}, nlengths, index, order;
    for (int a = 1; a < argc; ++a) {
        const char* eq = std::strchr(argv[a], '=');
        if (!eq) { std::fprintf(stderr, "not key=value: %s\n", argv[a]); return 2; }
        const std::string key(argv[a], (size_t)(eq - argv[a]));
        const char* val = eq + 1;
        if (key == "B") p.B = std::atoi(val);
        else if (key == "S") p.k.S = std::atoi(val);
        else if (key == "train") p.k.train = std::atoi(val);
        else if (key == "mode0") p.k.mode0 = std::atoi(val);
        else if (key == "mode1") p.k.mode1 = std::atoi(val);
        else if (key == "M") p.k.M = std::atoi(val);
        else if (key == "wrap") p.k.wrap_pad_prob = std::strtod(val, nullptr);
        else if (key == "gainp") p.k.gain_prob = std::strtod(val, nullptr);
        else if (key == "glo") p.k.gain_lo = std::strtod(val, nullptr);
        else if (key == "ghi") p.k.gain_hi = std::strtod(val, nullptr);
        else if (key == "tperc") p.k.time_perc = std::strtod(val, nullptr);
        else if (key == "noisep") p.k.noise_prob = std::strtod(val, nullptr);
        else if (key == "snrlo") p.k.snr_lo = std::strtod(val, nullptr);
        else if (key == "snrhi") p.k.snr_hi = std::strtod(val, nullptr);
        else if (key == "gaussp") p.k.gauss_prob = std::strtod(val, nullptr);
        else if (key == "alo") p.k.amp_lo = std::strtod(val, nullptr);
        else if (key == "ahi") p.k.amp_hi = std::strtod(val, nullptr);
        else if (key == "seed") p.seed = std::strtoull(val, nullptr, 0);
        else if (key == "base") p.stream_base = std::strtoull(val, nullptr, 0);
        else if (key == "step") step = std::strtoull(val, nullptr, 0);
        else if (key == "lengths") lengths = list_of(val);
        else if (key == "nlengths") nlengths = list_of(val);
        else if (key == "index") index = list_of(val);
        else if (key == "order") order = list_of(val);
        else { std::fprintf(stderr, "unknown key: %s\n", key.c_str()); return 2; }
    }
    // the entry's own refusals (csrc/inst_clips.hip): nothing below runs on arguments it would not launch
    const int B = p.B, M = p.k.M;
    if (B < 1 || p.k.S < 1 || lengths.empty() || M < 0 || M > kDrawMaxMasks || index.empty() == order.empty() ||
        (!index.empty() && (long long)index.size() != B) || p.k.mode0 < 0 || p.k.mode0 > 3 || p.k.mode1 < 0 || p.k.mode1 > 3) {
        std::fprintf(stderr, "refused: the arguments leaf_draw_clip_plan answers with a status\n");
        return 3;
    }
    auto offsets_of = [](const std::vector<long long>& len, std::vector<long long>& off, std::vector<int>& l32) {
        long long at = 0;
        for (long long n : len) {
            off.push_back(at);
            l32.push_back((int)n);
            at += n > 0 ? n : 0;
        }
    };
    std::vector<long long> offsets, noffsets;
    std::vector<int> len32, nlen32;
    offsets_of(lengths, offsets, len32);
    offsets_of(nlengths, noffsets, nlen32);
    p.offsets = offsets.data(); p.lengths = len32.data(); p.R = (int)len32.size();
    const bool noise = !nlengths.empty(), gauss = p.k.gauss_prob > 0.0;
    if (noise) { p.noise_offsets = noffsets.data(); p.noise_lengths = nlen32.data(); p.Rn = (int)nlen32.size(); }
    if (!index.empty()) p.index = index.data();
    else { p.order = order.data(); p.N = (long long)order.size(); }
    std::vector<long long> rec_off(B), noise_off(B), stream(B), index_out(B);
    std::vector<int> rec_len(B), start(B), pad_mode(B), rec(B), masks(2 * (size_t)B * M), noise_len(B), noise_start(B), noise_mode(B);
    std::vector<float> gain(B), coeff(2 * (size_t)B), amp(B);
    p.rec_off = rec_off.data(); p.rec_len = rec_len.data(); p.start = start.data(); p.pad_mode = pad_mode.data();
    p.gain = gain.data(); p.masks = M > 0 ? masks.data() : nullptr; p.rec = rec.data(); p.index_out = index_out.data();
    if (noise) {
        p.noise_off = noise_off.data(); p.noise_len = noise_len.data(); p.noise_start = noise_start.data();
        p.noise_pad_mode = noise_mode.data(); p.noise_coeff = coeff.data();
    }
    if (gauss) { p.gauss_amp = amp.data(); p.gauss_stream = stream.data(); }
    for (int b = 0; b < B; ++b) draw_plan_clip(p, step, b);
    for (int b = 0; b < B; ++b) {
        if (rec[b] != index_out[b]) return 4;
        std::printf("%d %lld %lld %d %d %d %08x |", b, index_out[b], rec_off[b], rec_len[b], start[b], pad_mode[b], bits(gain[b]));
        for (int m = 0; m < M; ++m) std::printf(" %d %d", masks[2 * ((size_t)b * M + m)], masks[2 * ((size_t)b * M + m) + 1]);
        std::printf(" |");
        if (noise) std::printf(" %lld %d %d %d %08x %08x", noise_off[b], noise_len[b], noise_start[b], noise_mode[b], bits(coeff[2 * b]), bits(coeff[2 * b + 1]));
        std::printf(" |");
        if (gauss) std::printf(" %08x %lld", bits(amp[b]), stream[b]);
        std::printf("\n");
    }
    return 0;
}
