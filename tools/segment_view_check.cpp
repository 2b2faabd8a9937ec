// segment_view_check.cpp -- the clamped row view of leaf_assemble_segments_f32 (csrc/leaf_segments_view.hpp, the very functions the
// kernels call) over hostile plans, on the CPU: an integer overflow or an index outside the buffers is found here, under
// -fsanitize=undefined, and not on a GPU.  Host only, no HIP:
//
//     c++ -std=c++17 -O1 -g -fsanitize=undefined -fno-sanitize-recover=undefined -I leaf_pytorch_amd/csrc \
//         tools/segment_view_check.cpp -o /tmp/segment_view_check && /tmp/segment_view_check
//
// Every combination of the values below goes through segment_view / segment_source / segment_peak_index, and what comes back is
// checked against the contract of include/leaf_hip.h: the recording inside store[0, store_len), every source index inside the
// recording, the peak index inside peaks[0, R) (the same clamp picks a clip's row of moments[0, R)), and the value the closed form
// clamp(win + t, 0, L - 1) gives in wide arithmetic.  The spans of leaf_clip_moments_f32 (moment_span) go through it too: for any
// length they follow each other, begin at whole tiles and cover [0, L) exactly.
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "leaf_segments_view.hpp"

static long long fails = 0;

static void expect(bool ok, const char* what, long long a, long long b, long long c, long long d, long long e) {
    if (ok) return;
    if (fails++ < 20) std::fprintf(stderr, "FAIL %s: rec_off=%lld rec_len=%lld win=%lld store_len=%lld S=%lld\n", what, a, b, c, d, e);
}

int main() {
    const long long store_lens[] = {0, 1, 7, 1000, (1ll << 31) - 1, 1ll << 31, 1ll << 40, LLONG_MAX};
    const long long offs[] = {LLONG_MIN, -(1ll << 62), -5, -1, 0, 1, 6, 7, 999, 1000, 1001, (1ll << 31), (1ll << 40), 1ll << 62, LLONG_MAX};
    const int lens[] = {INT_MIN, -3, -1, 0, 1, 2, 3, 4, 5, 7, 1000, INT_MAX - 1, INT_MAX};
    const long long wins[] = {LLONG_MIN, -(1ll << 62), -(1ll << 31) - 1, -(1ll << 31), -1001, -1000, -17, -16, -5, -4, -1, 0, 1, 3, 4, 6, 7,
                              15, 16, 999, 1000, (1ll << 31) - 1, 1ll << 31, 1ll << 62, LLONG_MAX};
    const int sizes[] = {1, 4, 5, 13, 16, 1000, 40000, INT_MAX - 3, INT_MAX};
    long long cases = 0;
    for (long long N : store_lens)
        for (long long off : offs)
            for (int len : lens)
                for (long long win : wins)
                    for (int S : sizes) {
                        ++cases;
                        const SegmentView v = segment_view(off, len, win, N, S);
                        expect(v.off >= 0 && v.off <= N, "off outside [0, store_len]", off, len, win, N, S);
                        expect(v.L >= 0 && v.L <= N - v.off, "L outside [0, store_len - off]", off, len, win, N, S);
                        expect(v.L <= (len < 0 ? 0 : len), "L beyond rec_len", off, len, win, N, S);
                        expect(-(long long)v.left >= -(long long)S && -(long long)v.left <= v.L, "win outside [-S, L]", off, len, win, N, S);
                        const SegmentView r = recording_view(off, len, N);
                        expect(r.off == v.off && r.L == v.L && r.left == 0, "recording_view differs", off, len, win, N, S);
                        if (v.L == 0) continue;                           // zeros: no sample is read
                        // the row's ends, its middle, and the chunk grid's overhang (t in [-3, S + 3) is formed, [0, S) is read)
                        const long long ts[] = {-3, 0, 1, (long long)S / 2, (long long)S - 1, (long long)S + 2};
                        for (long long t : ts) {
                            const long long j = segment_source(v, t);
                            expect(j >= 0 && j < v.L && v.off + j < N, "source outside the recording", off, len, win, N, S);
                            const __int128 wide = (__int128)win + t;      // the closed form, where it cannot overflow
                            const long long want = wide < 0 ? 0 : (wide > v.L - 1 ? v.L - 1 : (long long)wide);
                            if (t >= 0 && t < S) expect(j == want, "source is not clamp(win + t, 0, L - 1)", off, len, win, N, S);
                        }
                    }
    const int recs[] = {INT_MIN, -1, 0, 1, 5, 6, INT_MAX - 1, INT_MAX};
    const int Rs[] = {1, 2, 6, INT_MAX};
    for (int rec : recs)
        for (int R : Rs) {
            ++cases;
            const int i = segment_peak_index(rec, R);
            expect(i >= 0 && i < R && (rec < 0 || rec >= R || i == rec), "peak index outside [0, R)", rec, R, 0, 0, 0);
        }
    // leaf_clip_moments_f32: the spans of a recording of any length tile [0, L) in order, in whole tiles, for any (clamped) k
    const int Ls[] = {INT_MIN, -1, 0, 1, 2, 1023, 1024, 1025, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1, 300001, INT_MAX - 1024, INT_MAX - 1, INT_MAX};
    for (int L : Ls) {
        const long long len = L < 0 ? 0 : L;
        long long at = 0;
        for (int k = 0; k < kMomentSpans; ++k) {
            ++cases;
            const MomentSpan s = moment_span(L, k);
            expect(s.begin == at && s.end >= s.begin && s.end <= len, "spans do not follow each other inside [0, L)", L, k, s.begin, s.end, 0);
            expect(s.begin == s.end || s.begin % kMomentTile == 0, "a span does not begin at a tile", L, k, s.begin, s.end, 0);
            at = s.end;
        }
        expect(at == len, "the spans do not cover the recording", L, at, 0, 0, 0);
        const int ks[] = {INT_MIN, -1, kMomentSpans, INT_MAX};
        for (int k : ks) {
            ++cases;
            const MomentSpan s = moment_span(L, k), edge = moment_span(L, k < 0 ? 0 : kMomentSpans - 1);
            expect(s.begin == edge.begin && s.end == edge.end, "a span index outside is not clamped", L, k, s.begin, s.end, 0);
        }
    }
    std::printf("%lld cases, %lld failures\n", cases, fails);
    return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
