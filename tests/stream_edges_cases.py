"""Cases of tests/test_gpu_stream_edges.py and tests/test_host_stream_edges.py: the streaming family's geometries, recording-length
lattices, chunkings, parameter sets, an fp64 twin of the stream, and the integer model the coverage list is computed on.  Plain module,
no fixtures.  Of the product it imports the integer functions alone (streaming._geometry, stream_plan, stream_capacity and the
library's leaf_stream_history_samples): the geometry is taken from them, not restated; the host test holds it to the figures of the two fused geometries.

A recording of T samples (N(0,1), seeded by the geometry and T, three rows) is cut by a CHUNKING -- a list of chunk sizes that sum to T --
fed to a stream and flushed.  The lattice of T, per geometry (h the hop, r = reach, H the history, LS the block, cap the capacity):

    1, 2, h-1, h, h+1, padL, padL+1, r, r+1, r+2, K-1, K, K+1, H-1, H, H+1, LS-1, LS, LS+1, 2LS+1,
    r+1+62h, r+1+63h, r+1+64h  (one chunk emits 63, 64, 65 frames),  cap-1, cap, cap+1, cap+H+1,
    at 201 / 80 also r+1+126h, r+1+127h, r+1+128h  (127, 128, 129 frames in one step)

and the chunkings of a T: (a) one chunk; (b) one-sample chunks (T <= K + 1); (c) chunks of h, h-1, h+1; (d) [p, T-p] for every lattice
value p < T; (e) three seeded sequences from {1, 2, h-1, h, h+1, padL, r, r+1, K, H, LS-1, LS, LS+1, cap - hist_len, a random size};
(f) the explicit lists of FOUND.

n = 128 and 129 ARE reachable from the Python layer at 201 / 80 (a first chunk of r + 1 + 127 h = 10361 samples completes 128 frames:
(10361 - 1 - 200) // 80 + 1), so their lengths are lattice members; the raw-ABI windows run them as well.  c_lo > 0 is not reachable:
a stream's first frame of a step is at most `lead` = 3, and 3 h - padL < LS (the host test shows it over every position)."""
import functools
import random
from collections import namedtuple

import torch

import forward_edges_cases as fe
from leaf_pytorch_amd import _native
from leaf_pytorch_amd.streaming import _geometry, stream_capacity, stream_plan
from oracle import leaf_oracle as lo

F = 6
SAMPLE_RATE = {(401, 160): 16000, (201, 80): 8000, (552, 220): 22050, (801, 320): 32000, (1103, 441): 44100}
FUSED = ((401, 160), (201, 80))                                 # the one-launch kernel's geometries
TWO_LAUNCH_ONLY = ((552, 220), (801, 320), (1103, 441))
Geo = namedtuple("Geo", "K hop padL lead reach H LS cap sr")


@functools.lru_cache(maxsize=None)
def geo(K, hop):
    lead, reach = _geometry(K, hop)
    return Geo(K, hop, fe.pad_left(K), lead, reach, _native.load().leaf_stream_history_samples(K, hop),
               fe.fft_block_len(K, hop, (K, hop) in fe.STATIC), stream_capacity(K, hop), SAMPLE_RATE[(K, hop)])


def gid(g):
    return f"{g.K}-{g.hop}"


# ---- recording lengths
def lattice(g):
    K, h, r, H, LS, cap = g.K, g.hop, g.reach, g.H, g.LS, g.cap
    ts = {1, 2, h - 1, h, h + 1, g.padL, g.padL + 1, r, r + 1, r + 2, K - 1, K, K + 1, H - 1, H, H + 1, LS - 1, LS, LS + 1, 2 * LS + 1,
          r + 1 + 62 * h, r + 1 + 63 * h, r + 1 + 64 * h, cap - 1, cap, cap + 1, cap + H + 1}
    if (K, h) == (201, 80):
        ts |= {r + 1 + 126 * h, r + 1 + 127 * h, r + 1 + 128 * h}
    return sorted(ts)


def reduced_lattice(g):
    return sorted({1, g.hop, g.reach, g.reach + 1, g.K, g.LS + 1, 2 * g.LS + 1})


# ---- the integer model: what the Python layer does with a chunking
Step = namedtuple("Step", "chunk piece hist_len next started Tc first n drop final")


def plan_steps(g, sizes):
    """The launches of LeafStream(fused=True) fed `sizes` and flushed: a chunk beyond capacity - hist_len goes in pieces.  (A geometry
    the one-launch kernel does not serve has no capacity: the two-launch stream takes every chunk whole.)"""
    cap = g.cap if (g.K, g.hop) in FUSED else 1 << 30
    hist = nxt = 0
    started, out = False, []
    for ci, size in enumerate(sizes):
        at = 0
        while at < size:
            take = min(size - at, cap - hist)
            first, n, drop, hist2, nxt2 = stream_plan(hist, nxt, take, g.K, g.hop, False)
            out.append(Step(ci, at > 0, hist, nxt, started, take, first, n, drop, False))
            hist, nxt, started, at = hist2, nxt2, started or n > 0, at + take
    first, n, drop, _, _ = stream_plan(hist, nxt, 0, g.K, g.hop, True)
    out.append(Step(len(sizes), False, hist, nxt, started, 0, first, n, drop, True))
    return out


def counts_per_chunk(g, sizes):
    """Frames every step() call returns, then flush()."""
    out = [0] * (len(sizes) + 1)
    for s in plan_steps(g, sizes):
        out[s.chunk] += s.n
    return out


def stream_blocks(g, first, n, T):
    """csrc/leaf_kernels.hip, stream_blocks, restated: (c_lo, nb) of frames first .. first + n - 1 (n > 0) of a buffer of T samples."""
    c_lo = max(0, first * g.hop - g.padL) // g.LS
    return c_lo, min(T - 1, (first + n - 1) * g.hop - g.padL + g.K - 1) // g.LS - c_lo + 1


def stream_frames_ok(g, first, n, T):
    TPv = (T - 1) // g.hop + 1 if T > 0 else 0
    return first >= 0 and n >= 0 and first <= TPv and n <= TPv - first


STREAM_EVENTS = ("n==0", "n==1", "n==63", "n==64", "n==65", "first step n>64", "nb==1", "nb==10", "buffer==capacity", "hist_len==H",
                 "drop==0 with n>0", "chunk in pieces", "never a frame", "started n>64")
EVENTS_8K = ("n==127 first step", "n==128 first step", "n==129 first step")


def events(g, sizes):
    """The events of the coverage list a chunking reaches, on integers."""
    ev, steps = set(), plan_steps(g, sizes)
    for s in steps:
        T = s.hist_len + s.Tc
        if s.n == 0 and not s.final:
            ev.add("n==0")
        if s.n in (1, 63, 64, 65):
            ev.add(f"n=={s.n}")
        if s.n > 64 and s.hist_len == 0 and s.chunk == 0 and not s.piece:
            ev.add("first step n>64")
            if s.n in (127, 128, 129):
                ev.add(f"n=={s.n} first step")
        if s.n > 64 and s.started:
            ev.add("started n>64")
        if s.n > 0:
            c_lo, nb = stream_blocks(g, s.first, s.n, T)
            assert 1 <= nb <= 10
            ev |= {f"nb=={nb}"} & {"nb==1", "nb==10"}
            if c_lo > 0:
                ev.add("c_lo>0")
        if T == g.cap:
            ev.add("buffer==capacity")
        if s.hist_len == g.H:
            ev.add("hist_len==H")
        if s.drop == 0 and s.n > 0 and not s.final:
            ev.add("drop==0 with n>0")
        if s.piece:
            ev.add("chunk in pieces")
    if not any(s.n for s in steps[:-1]):
        ev.add("never a frame")
    return ev


# ---- chunkings
def _cut(T, size):
    return [size] * (T // size) + ([T % size] if T % size else [])


def random_sizes(g, T, i):
    """Chunking (e): sizes drawn until T is used up; `cap - hist_len` fills the virtual buffer to exactly the capacity.  (A draw of
    it late in a recording is cut to what is left, so the third sequence of a T >= cap takes it as its second size: the member is live.)"""
    rng = random.Random(7919 * g.K + 31 * T + i)
    fixed = [1, 2, g.hop - 1, g.hop, g.hop + 1, g.padL, g.reach, g.reach + 1, g.K, g.H, g.LS - 1, g.LS, g.LS + 1, "fill", "random"]
    sizes, hist, nxt = [], 0, 0
    while sum(sizes) < T:
        pick = rng.choice(fixed)
        pick = "fill" if (i == 2 and T >= g.cap and len(sizes) == 1) else pick
        pick = g.cap - hist if pick == "fill" else rng.randrange(1, 4000) if pick == "random" else pick
        size = min(pick, T - sum(sizes))
        sizes.append(size)
        at = 0
        while at < size:
            take = min(size - at, g.cap - hist)
            _, _, _, hist, nxt = stream_plan(hist, nxt, take, g.K, g.hop, False)
            at += take
    return sizes


# (f) Explicit chunkings, written down from an integer search over stream_plan for what (a) - (e) reach only by the luck of a seed or
# not at all: a buffer filled to exactly the capacity on top of a full history; more than 64 frames on a stream that HAS started (the
# carried state and the inter-group carry in one launch); n = 63 .. 65 and 127 .. 129 on a started stream; and every step ending ON a
# frame's reach (one sample short of completing it) or one sample behind it -- the chunking at which a stream that takes the reach one
# sample short emits EVERY frame early, which is what lifts that defect over the GPU bound (the host test's mutations).
FOUND = {
    (401, 160): {
        16000: [("f-fill-on-H", [880, 15120])],
        16881: [("f-fill-then-rest", [880, 15120, 881]), ("f-started-65", [401, 10400, 6080])],
        10641: [("f-started-64", [401, 10240]), ("f-started-63", [561, 10080]), ("f-ends-on-every-reach", [400] + [160] * 64 + [1])],
        3201: [("f-hops-then-block", [160] * 10 + [1601]), ("f-ends-on-every-reach", [400] + [160] * 17 + [81]),
               ("f-completes-one-frame-each", [401] + [160] * 17 + [80])],
    },
    (201, 80): {
        16000: [("f-fill-on-H", [440, 15560])],
        16441: [("f-fill-then-rest", [440, 15560, 441]), ("f-started-65", [201, 5200, 11040]), ("f-started-129", [201, 10320, 5920])],
        10441: [("f-started-128", [201, 10240]), ("f-started-127", [281, 10160])],
        5321: [("f-started-64", [201, 5120]), ("f-started-63", [281, 5040]), ("f-ends-on-every-reach", [200] + [80] * 64 + [1])],
        3201: [("f-hops-then-block", [80] * 20 + [1601]), ("f-ends-on-every-reach", [200] + [80] * 37 + [41]),
               ("f-completes-one-frame-each", [201] + [80] * 37 + [40])],
    },
}


def chunkings(g, T, kinds="abcdef", points=None):
    """[(name, sizes)] of one recording length, duplicates (as size lists) dropped, every list summing to T.  `points`: the lattice
    whose members p < T split (d) (default: the geometry's full lattice; the reduced lattice splits at its own members)."""
    out = []
    if "a" in kinds:
        out.append(("a", [T]))
    if "b" in kinds and T <= g.K + 1:
        out.append(("b", [1] * T))
    if "c" in kinds:
        out += [(f"c{s}", _cut(T, s)) for s in (g.hop, g.hop - 1, g.hop + 1)]
    if "d" in kinds:
        out += [(f"d{p}", [p, T - p]) for p in (lattice(g) if points is None else points) if p < T]
    if "e" in kinds:
        out += [(f"e{i}", random_sizes(g, T, i)) for i in range(3)]
    if "f" in kinds:
        out += FOUND.get((g.K, g.hop), {}).get(T, [])
    seen, kept = set(), []
    for name, sizes in out:
        sizes = [s for s in sizes if s > 0]
        assert sum(sizes) == T and sizes, (gid(g), T, name, sizes)
        if tuple(sizes) not in seen:
            seen.add(tuple(sizes))
            kept.append((name, sizes))
    return kept


def all_cases(g, kinds="abcdef", ts=None):
    return [(T, name, sizes) for T in (lattice(g) if ts is None else ts) for name, sizes in chunkings(g, T, kinds)]


def bitwise_subset(g, T):
    """The chunkings the bit-for-bit properties (rows alone, int16, bfloat16, a poisoned second stream) run at: (a), (c) hop + 1, (e) 0, (f)."""
    return [(n, s) for n, s in chunkings(g, T) if n in ("a", f"c{g.hop + 1}", "e0") or n.startswith("f")]


# ---- signals and parameters
@functools.lru_cache(maxsize=None)
def signal(K, hop, T):
    """(3, 1, T) float32, N(0,1): rows of a B = 3 stream; B = 1 takes row 0."""
    return torch.randn(3, 1, T, generator=torch.Generator().manual_seed(1000 * K + hop + 7 * T))


def pcm16(x):
    return (x.clamp(-4, 4) * 8000).round().to(torch.int16)


PSETS = ("defaults", "away", "wide")
_AWAY = {"_compression.ema._weights": [0.0, 1.0, -0.2, 1.5, 0.04, 0.5], "_compression.alpha": [0.96, 0.96, 0.96, 0.96, 1.2, 0.8],
         "_compression.delta": [2.0, 2.0, 2.0, 2.0, 0.5, 3.0], "_compression.root": [2.0, 2.0, 2.0, 2.0, 1.0, 3.0]}
# "wide": filters as long as the window (sigma up to its clamp, K sqrt(2 ln 2) / pi = 0.375 K) and the widest pooling windows, so that
# the samples and frames at the very edge of a receptive field carry weight: the default bank at F = 6 has sigma <= 11 samples, and a
# stream that emits a frame one sample early, or drops one hop too many, computes the same numbers with it.  PCEN as "away".
_WIDE_MU = [0.0, 0.3, 0.8, 1.5, 0.02, 3.1]
_WIDE_SIGMA = [0.4, 0.3, 0.22, 0.375, 0.4, 0.35]             # in units of K
_WIDE_POOL = [0.5, 0.5, 0.45, 0.4, 0.5, 0.3]


@functools.lru_cache(maxsize=None)
def _params(K, hop, pset, n_filters):
    g = geo(K, hop)
    p = lo.default_params(lo.geometry(F, g.sr))
    if pset in ("away", "wide"):
        p.update({k: torch.tensor(v) for k, v in _AWAY.items()})
    if pset == "wide":
        p["_complex_conv._kernel"] = torch.tensor([[m, s * K] for m, s in zip(_WIDE_MU, _WIDE_SIGMA)])
        p["_pooling.weights"] = torch.tensor(_WIDE_POOL).reshape(1, 1, F, 1)
    if n_filters != F:
        p = {k: (v[:, :, :n_filters] if v.dim() == 4 else v[:n_filters]).clone() for k, v in p.items()}
    return p


def params(g, pset, n_filters=F):
    """The state dict (float32, CPU) of a parameter set; n_filters = 1: its row 0 (the "away" set's: a smoother clamped to 0)."""
    assert pset in PSETS
    return {k: v.clone() for k, v in _params(g.K, g.hop, pset, n_filters).items()}


def lgeo(g, n_filters=F):
    return lo.LeafGeometry(n_filters, g.sr, g.K, g.hop, *lo.same_padding(g.K))


# ---- fp64 references
def pcen_point(p, m, prm):
    """oracle.leaf_oracle.pcen's point function with the smoother given (the host test holds it to lo.pcen with lo.ema_scan's)."""
    a = prm["_compression.alpha"].clamp(max=1.0).reshape(1, -1, 1)
    inv_r = (1.0 / prm["_compression.root"].clamp(min=1.0)).reshape(1, -1, 1)
    d = prm["_compression.delta"].reshape(1, -1, 1)
    return (p / (lo.PCEN_FLOOR + m) ** a + d) ** inv_r - d ** inv_r


@functools.lru_cache(maxsize=None)
def _pooled64(K, hop, T, wide):
    g = geo(K, hop)
    prm = {k: v.double() for k, v in params(g, "wide" if wide else "defaults").items()}
    return lo.leaf_forward(signal(K, hop, T).double(), prm, lgeo(g), False, torch.float64)


def pooled64(g, pset, T):
    """(3, F, frames) floored pooled frames of the whole recording, fp64 ("defaults" and "away" share filters and pooling)."""
    return _pooled64(g.K, g.hop, T, pset == "wide")


@functools.lru_cache(maxsize=None)
def _oracle(K, hop, pset, T):
    g = geo(K, hop)
    prm = {k: v.double() for k, v in params(g, pset).items()}
    return lo.pcen(pooled64(g, pset, T), prm["_compression.alpha"], prm["_compression.delta"], prm["_compression.root"],
                   prm["_compression.ema._weights"])


def oracle(g, pset, T, n_filters=F):
    """The fp64 whole-clip oracle (3, n_filters, frames), PCEN on; never modified."""
    return _oracle(g.K, g.hop, pset, T)[:, :n_filters]


def window_oracle(g, pset, T, first, n, mode):
    """Frames first .. first + n - 1 of the whole clip as a raw step emits them: mode "log1p" the oracle's own pooled frames through
    log1p, mode "pcen" the oracle's PCEN with the smoother started at frame `first`."""
    p = pooled64(g, pset, T)[:, :, first:first + n]
    if mode == "log1p":
        return torch.log1p(p)
    prm = {k: v.double() for k, v in params(g, pset).items()}
    return lo.pcen(p, prm["_compression.alpha"], prm["_compression.delta"], prm["_compression.root"], prm["_compression.ema._weights"])


MUTATIONS = ("reach-1", "drop+1", "seam", "carry-step", "carry-group", "pad")


class Twin:
    """The stream in fp64 on the CPU: step() and flush() driven by stream_plan, the pooled frames of [history | chunk] from the oracle
    without compression, a five-line smoother whose state is carried from step to step and starts at the first emitted frame, and the
    oracle's PCEN point function.

    `mutation` breaks it the way a kernel or host defect would (`at`: the step index the one-step mutations strike at, default any):
      reach-1      a frame leaves one sample before its receptive field is complete (the sample counts as zero)
      drop+1       one hop too many is dropped in front of the next frame
      seam         the last sample of the history is lost (zero) where the chunk is joined to it
      carry-step   the smoother's carry is forgotten at step `at`: it restarts from that step's first frame
      carry-group  the carry is forgotten between two groups of 64 frames of one step
      pad          a non-final step zeroes the energy one sample early, as the clip-end padding would at a final one"""

    def __init__(self, g, prm, mutation=None, at=None):
        assert mutation is None or mutation in MUTATIONS
        self.g, self.mutation, self.at = g, mutation, at
        self.prm = {k: v.double() for k, v in prm.items()}
        self.lgeo = lgeo(g, self.prm["_pooling._bias"].numel())
        self.w = self.prm["_compression.ema._weights"].clamp(0.0, 1.0).reshape(1, -1)
        self.buf, self.next, self.M, self.i = None, 0, None, 0

    def _plan(self, hist_len, Tc, final):
        g = self.g
        if self.mutation not in ("reach-1", "drop+1"):
            return stream_plan(hist_len, self.next, Tc, g.K, g.hop, final)
        # stream_plan restated, with the defect
        L = hist_len + Tc
        reach = g.reach - (self.mutation == "reach-1")
        last = (L - 1) // g.hop if final else (L - 1 - reach) // g.hop
        n = max(0, last - self.next + 1)
        if final:
            return self.next, n, L, 0, 0
        if n == 0:
            return self.next, 0, 0, L, self.next
        drop = max(0, last + 1 - g.lead)
        if self.mutation == "drop+1" and drop > 0:
            # the buffer starts one hop later; the frames keep their place in the recording, the samples in front are gone
            return self.next, n, (drop + 1) * g.hop, L - (drop + 1) * g.hop, last + 1 - drop - 1
        return self.next, n, drop * g.hop, L - drop * g.hop, last + 1 - drop

    def _smooth(self, p):
        out = torch.empty_like(p)
        for k in range(p.shape[-1]):
            forget = self.M is None or (self.mutation == "carry-group" and k > 0 and k % 64 == 0)
            self.M = p[:, :, k] if forget else self.M
            self.M = self.w * p[:, :, k] + (1.0 - self.w) * self.M
            out[:, :, k] = self.M
        return out

    def _emit(self, Tc, final):
        g, L = self.g, self.buf.shape[-1]
        first, n, drop, hist2, nxt2 = self._plan(L - Tc, Tc, final)
        B, nf = self.buf.shape[0], self.lgeo.n_filters
        out = torch.empty(B, nf, 0, dtype=torch.float64)
        if n > 0:
            buf = self.buf
            if self.mutation == "drop+1" and first < 0:            # frames in front of the buffer: the samples they need are zeros
                buf = torch.cat([torch.zeros(B, -first * g.hop, dtype=torch.float64), buf], dim=-1)
                first = 0
            _, st = lo.leaf_forward(buf.unsqueeze(1), self.prm, self.lgeo, False, torch.float64, True)
            e = st["energy"]
            if self.mutation == "pad" and not final:
                e = e.clone()
                e[:, :, buf.shape[-1] - 1 - (g.K - 1 - g.padL):] = 0.0
            p = lo.gaussian_pool(e, st["lowpass"], self.prm["_pooling._bias"], g.hop).clamp_min(lo.FLOOR_POOLED)[:, :, first:first + n]
            if self.mutation == "carry-step" and self.at in (None, self.i) and self.M is not None:
                self.M = None
            out = pcen_point(p, self._smooth(p), self.prm)
        self.buf, self.next = self.buf[:, drop:], nxt2
        assert final or self.buf.shape[-1] == hist2
        self.i += 1
        return out

    def step(self, chunk):
        """chunk (B, Tc) -> (B, F, n) float64."""
        chunk = chunk.double()
        hist = chunk[:, :0] if self.buf is None else self.buf
        if self.mutation == "seam" and hist.shape[-1] and self.at in (None, self.i):
            hist = hist.clone()
            hist[:, -1] = 0.0
        self.buf = torch.cat([hist, chunk], dim=-1)
        return self._emit(chunk.shape[-1], False)

    def flush(self):
        if self.buf is None:
            return torch.empty(0, self.lgeo.n_filters, 0, dtype=torch.float64)
        out = self._emit(0, True)
        self.buf, self.next, self.M = None, 0, None
        return out

    def run(self, x, sizes):
        """x (B, 1, T) cut by `sizes`, flushed: ([frames per step() and flush()], concatenated)."""
        outs, pos = [], 0
        for s in sizes:
            outs.append(self.step(x[:, 0, pos:pos + s]))
            pos += s
        outs.append(self.flush())
        return outs, torch.cat(outs, dim=-1)


# ---- raw windows (part 2 of the GPU file): (first, n) of leaf_stream_step_f32 with hist_len = 0, started = 0, Tc = T
WINDOW_N = (1, 2, 63, 64, 65)


def window_lengths(g):
    return (g.LS + 1, 5 * g.LS + 3, g.cap)


def edge_frames(g, T):
    """Frames 0, 1, the last, and around every block boundary c LS the frames whose windows [m h - padL, m h - padL + K - 1] start or
    end nearest to it, with their neighbours."""
    TPv = (T - 1) // g.hop + 1
    ms = {0, 1, TPv - 1}
    for c in range(1, -(-T // g.LS)):
        start, end = (c * g.LS + g.padL) // g.hop, (c * g.LS + g.padL - g.K + 1) // g.hop
        ms |= {start - 1, start, start + 1, end - 1, end, end + 1}
    return sorted(m for m in ms if 0 <= m < TPv)


def windows(g, T):
    """[(first, n)]: every n of WINDOW_N (and 128, 129 at 201 / 80 with T = cap) with `first` or the last frame on an edge frame."""
    TPv, out = (T - 1) // g.hop + 1, set()
    ns = WINDOW_N + ((128, 129) if (g.K, g.hop, T) == (201, 80, g.cap) else ())
    for n in ns:
        for m in edge_frames(g, T):
            for first in (m, m - n + 1):
                if first >= 0 and first + n <= TPv:
                    out.add((first, n))
    return sorted(out)


# ---- the bank: three slots, every slot a sequence of lattice streams.  An entry is (T, chunking name, how it ends, idle steps
# before it): "last" ends on the last chunk (one step with samples and `end`), "empty" ends in a step of its own without samples.
# max_chunk = cap - H bounds a bank's chunk, so the chunkings here have none longer.
BANK_STREAMS = {
    (401, 160): [
        [(1601, "c160", "last", 0), (3201, "c161", "last", 2), (401, "a", "last", 0), (1, "a", "last", 1), (880, "d400", "empty", 0)],
        [(10641, "a", "last", 1), (2321, "f-bank-eq", "last", 0), (160, "a", "empty", 3), (3201, "e1", "last", 0)],
        [(402, "b", "last", 5), (10481, "d1600", "last", 0), (1600, "c159", "empty", 2)],
    ],
    (201, 80): [
        [(1601, "c80", "last", 0), (3201, "c81", "last", 2), (201, "a", "last", 0), (1, "a", "last", 1), (440, "d200", "empty", 0)],
        [(10441, "a", "last", 1), (1161, "f-bank-eq", "last", 0), (80, "a", "empty", 3), (3201, "e1", "last", 0)],
        [(202, "b", "last", 5), (5321, "d1600", "last", 0), (1600, "c79", "empty", 2)],
    ],
}
# the ending pass with drop == hist_len: the history entering the last chunk is a whole number of hops, all of it dropped
BANK_FOUND = {(401, 160): {2321: ("f-bank-eq", [1600, 721])}, (201, 80): {1161: ("f-bank-eq", [800, 361])}}
BANK_EVENTS = ("end drop<hist_len", "end drop==hist_len", "end drop>hist_len", "end n==0", "end without samples", "slot reused", "idle between")


def bank_sizes(g, T, name):
    if name.startswith("f-bank"):
        found = BANK_FOUND[(g.K, g.hop)][T]
        assert found[0] == name and sum(found[1]) == T
        return found[1]
    return dict(chunkings(g, T))[name]


def bank_script(g, streams=None):
    """(script, order): the rows [(length, end)] * slots of LeafStreamBank.step, and per slot its streams [(T, sizes)] in order."""
    streams = BANK_STREAMS[(g.K, g.hop)] if streams is None else streams
    ops, order = [], []
    for slot in streams:
        col, mine = [], []
        for T, name, how, idle in slot:
            sizes = bank_sizes(g, T, name)
            assert max(sizes) <= g.cap - g.H, (T, name)
            col += [(0, 0)] * idle + [(s, 0) for s in sizes[:-1]]
            col += [(sizes[-1], 1)] if how == "last" else [(sizes[-1], 0), (0, 1)]
            mine.append((T, sizes))
        ops.append(col)
        order.append(mine)
    rows = max(len(c) for c in ops)
    return [[c[i] if i < len(c) else (0, 0) for c in ops] for i in range(rows)], order


def bank_events(g, script, plan):
    """The bank's events of the coverage list, from the records `plan` (LeafStreamBank._plan of a bank of len(script[0]) slots) makes."""
    ev, B = set(), len(script[0])
    running, used, was_idle = [False] * B, [False] * B, [False] * B
    for row in script:
        recs, _ = plan([r[0] for r in row], [bool(r[1]) for r in row])
        for b, (Tc, end) in enumerate(row):
            r = recs[b]
            if r.idle:
                was_idle[b] = was_idle[b] or used[b]
                continue
            if not running[b] and used[b]:
                ev.add("slot reused")
                if was_idle[b]:
                    ev.add("idle between")
            running[b], used[b] = True, True
            if end:
                running[b], was_idle[b] = False, False
                if Tc == 0:
                    ev.add("end without samples")
                elif r.end_n == 0:
                    ev.add("end n==0")                          # the chunk completes no frame: one pass serves
                else:
                    ev.add("end drop" + ("<" if r.drop_samples < r.hist_len else "==" if r.drop_samples == r.hist_len else ">") + "hist_len")
    return ev


def wide_bank_script(g):
    """A bank of 130 slots -- two launches (a launch holds 128) -- in a handful of steps: slots 0 .. 126 carry one short one-chunk
    stream each, beginning at different steps and ending both ways; slots 127 .. 129, behind the split, carry lattice streams.
    Returns (script, {slot: (T, sizes)} of those three)."""
    lat = {127: (g.LS + 1, f"d{g.LS}", "last", 0), 128: (g.H + 1, f"d{g.H}", "empty", 0), 129: (2 * g.LS + 1, f"d{g.LS + 1}", "last", 1)}
    streams = [[(300 + 3 * b, "a", "last" if b % 2 else "empty", b % 3)] for b in range(127)] + [[lat[b]] for b in (127, 128, 129)]
    script, order = bank_script(g, streams)
    return script, {b: order[b][0] for b in lat}
