"""The plan drawn on the device, the host side (no GPU): the oracle of leaf_draw_clip_plan -- Philox4x32-10 over NumPy integers and
the formulas of include/leaf_hip.h in float64 -- pinned against the library's existing stream, then compared with the draw header
itself (csrc/leaf_clip_draws.hpp, through tools/clip_draws_check.cpp compiled with plain g++); the distributions; the C entry as
declared and exported, and its argument checks.  tests/test_gpu_clip_draws.py compares the kernel with the oracle defined here."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from leaf_pytorch_amd import DeviceClipSampler, PackedClips, _native
from test_host_clip_noise import MASK32, PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1, philox4x32_10, philox_groups

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, ALIGNMENT = -1, -2, -7
LN10 = 2.302585092994045684                            # the constant of the header (the double next to ln 10)
NOISE_COUNTER, GAUSS_COUNTER = 64, 65
DEFAULTS = dict(pad_modes=(2, 1), wrap_pad_prob=0.5, gain_prob=0.25, gain_db=(-18.0, 6.0), num_masks=0, time_perc=0.0, noise_prob=0.5,
                snr_range=(10.0, 25.0), gaussian_prob=0.0, gaussian_amplitude=(0.001, 0.015))


def consts(**kw):
    assert set(kw) <= set(DEFAULTS)
    return {**DEFAULTS, **kw}


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def philox_words(seed: int, ids: np.ndarray, q: int, word1: int = 1) -> np.ndarray:
    """Philox4x32-10 under the key (lo32(seed), hi32(seed)) on the counters (q, word1, lo32(id), hi32(id)), one per entry of ``ids``
    (uint64): (n, 4) uint64 holding 32-bit words.  Integers only."""
    ids = np.asarray(ids, dtype=np.uint64)
    m, s32 = np.uint64(MASK32), np.uint64(32)
    c0, c1 = np.full(ids.shape, q, dtype=np.uint64), np.full(ids.shape, word1, dtype=np.uint64)
    c2, c3 = ids & m, ids >> s32
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return np.stack((c0, c1, c2, c3), axis=1)


def unit(r: np.ndarray) -> np.ndarray:
    """u(r) = r 2^-32 in float64 (exact)."""
    return r.astype(np.float64) * 2.0 ** -32


def below(r: np.ndarray, n) -> np.ndarray:
    """(uint64(r) n) >> 32, a uniform integer in [0, n): r < 2^32 and n <= 2^32, so the product fits 64 bits."""
    return ((r * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def plan_ref(k: dict, size: int, train: bool, seed: int, stream_base: int, step: int, B: int, lengths, index=None, order=None,
             noise_lengths=None) -> dict:
    """The plan of leaf_draw_clip_plan by the definition in include/leaf_hip.h.  ``lengths`` / ``noise_lengths``: the stores'
    recordings, lying back to back.  Integer fields are int64 arrays; gain, coeff and gauss_amp are float64 BEFORE their one rounding
    (``compare`` rounds them).  Every group is computed, whatever the call under test asks for."""
    S, M = int(size), int(k["num_masks"])
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.cumsum(np.maximum(lengths, 0)) - np.maximum(lengths, 0)
    R = lengths.size
    ids = np.array([(stream_base + step * B + b) % 2 ** 64 for b in range(B)], dtype=np.uint64)
    if index is not None:
        raw = np.asarray(index, dtype=np.int64)
    else:
        order = np.asarray(order, dtype=np.int64)
        raw = order[[((step * B + b) % 2 ** 64) % order.size for b in range(B)]]
    i = np.clip(raw, 0, R - 1)
    L = lengths[i]
    out = dict(index=i, rec=i, rec_off=offsets[i], rec_len=L)
    w = philox_words(seed, ids, 0)
    out["pad_mode"] = np.where(unit(w[:, 0]) < k["wrap_pad_prob"], k["pad_modes"][0], k["pad_modes"][1]).astype(np.int64)
    span = np.maximum(L - S, 0)
    out["start"] = below(w[:, 1], span + 1) if train else span // 2
    lo, hi = k["gain_db"]
    db = lo + (hi - lo) * unit(w[:, 3])
    out["gain"] = np.where(unit(w[:, 2]) < k["gain_prob"], np.exp(db * (LN10 / 20.0)), 1.0)
    if M > 0:
        used = 1 + below(philox_words(seed, ids, 1)[:, 0], M)
        masks = np.zeros((B, M, 2), dtype=np.int64)
        for m in range(M):
            w = philox_words(seed, ids, 2 + m)
            v = (unit(w[:, 0]) * k["time_perc"]) * float(S)
            n = np.where(m < used, np.clip(np.floor(np.nan_to_num(v, nan=0.0)), 0, S), 0).astype(np.int64)
            masks[:, m, 0] = np.floor(unit(w[:, 1]) * (S - n).astype(np.float64)).astype(np.int64)
            masks[:, m, 1] = n
        out["masks"] = masks
    if noise_lengths is not None:
        nl = np.asarray(noise_lengths, dtype=np.int64)
        noff = np.cumsum(np.maximum(nl, 0)) - np.maximum(nl, 0)
        w = philox_words(seed, ids, NOISE_COUNTER)
        apply = unit(w[:, 0]) < k["noise_prob"]
        lo, hi = k["snr_range"]
        snr = lo + (hi + 1.0 - lo) * unit(w[:, 1])
        j = below(w[:, 2], nl.size)
        nstart = below(w[:, 3], np.maximum(nl[j] - S, 0) + 1)
        ratio = np.exp(snr * (LN10 / 10.0))
        c = ratio / (1.0 + ratio)
        out.update(noise_off=noff[j], noise_len=np.where(apply, nl[j], 0), noise_start=np.where(apply, nstart, 0),
                   noise_pad_mode=np.full(B, 2, dtype=np.int64), coeff=np.stack((c, 1.0 - c), axis=1))
    w = philox_words(seed, ids, GAUSS_COUNTER)
    lo, hi = k["gaussian_amplitude"]
    out["gauss_amp"] = np.where(unit(w[:, 0]) < k["gaussian_prob"], (lo + (hi - lo) * unit(w[:, 1])).astype(np.float32).astype(np.float64), 0.0)
    out["gauss_stream"] = ids.astype(np.int64)          # the id's 64 bits as an int64
    return out


INT_FIELDS = ("index", "rec", "rec_off", "rec_len", "start", "pad_mode", "masks", "noise_off", "noise_len", "noise_start", "noise_pad_mode",
              "gauss_stream")


def f32_bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32).astype(np.int64)


def compare(got: dict, want: dict) -> None:
    """``got`` (whatever groups the call under test produced; floats as float32) against the oracle: every integer field equal,
    gauss_amp bit-equal (IEEE add and multiply only), gain and both coefficients within ONE float32 ulp -- the only inexact operation
    behind them is a double-precision exp (relative error about 2^-52), so the two float32 roundings differ only where the double
    sits on a rounding boundary, and then by one ulp.  All three are positive, so the ulp distance is the distance of the bit patterns."""
    assert set(got) <= set(want), set(got) - set(want)
    for name, g in got.items():
        g = np.asarray(g)
        if name in INT_FIELDS:
            assert np.array_equal(g.astype(np.int64), want[name]), name
        elif name == "gauss_amp":
            assert np.array_equal(f32_bits(g), f32_bits(want[name])), name
        else:
            assert name in ("gain", "coeff")
            d = np.abs(f32_bits(g) - f32_bits(want[name]))
            assert d.shape == np.asarray(want[name]).shape and int(d.max()) <= 1, (name, int(d.max()))


# ---- the oracle is the library's generator ---------------------------------------------------------------------------------------------

def test_the_oracle_is_the_stream_generator_with_counter_word_1_set():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((MASK32,) * 4, (MASK32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for (c0, c1, c2, c3), (k0, k1), want in kat:        # the known answers of tests/test_host_clip_noise.py, through this file's rounds
        got = philox_words(k0 | (k1 << 32), np.array([c2 | (c3 << 32)], dtype=np.uint64), c0, word1=c1)[0]
        assert " ".join(f"{int(w):08x}" for w in got) == want
    # with word 1 at 0 the words are those behind _native.gaussian_noise's documented stream: counter (g, 0, stream), key = seed
    seed, stream = 0xa4093822_299f31d0, 2 ** 40 + 5
    groups = philox_groups(seed, stream, 7)
    for g in (0, 3, 6):
        assert np.array_equal(philox_words(seed, np.array([stream], dtype=np.uint64), g, word1=0)[0], groups[g])
    # ... and with word 1 at 1, the plan's domain, they are the plain rounds on (q, 1, id): never a counter of the Gaussian stream
    ids = np.array([0, 5, 2 ** 64 - 1], dtype=np.uint64)
    for q in (0, 1, 33, 64, 65):
        w = philox_words(seed, ids, q)
        for n, i in enumerate(ids.tolist()):
            assert tuple(int(x) for x in w[n]) == philox4x32_10((q, 1, i & MASK32, i >> 32), (seed & MASK32, seed >> 32))
    assert not np.array_equal(philox_words(seed, ids, 0), philox_words(seed, ids, 0, word1=0))
    assert LN10 == math.log(10.0) and np.log(10.0) == LN10


def test_the_integer_rules():
    r = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    assert below(r, 1).tolist() == [0, 0, 0, 0] and below(r, 11).tolist() == [0, 0, 5, 10] and below(r, 2 ** 31).tolist() == [0, 0, 2 ** 30, 2 ** 31 - 1]
    assert unit(r).tolist() == [0.0, 2.0 ** -32, 0.5, 1 - 2.0 ** -32]


# ---- the draw header, through tools/clip_draws_check.cpp ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path_factory.mktemp("clip_draws") / "clip_draws_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(REPO, "leaf_pytorch_amd", "csrc"),
                    os.path.join(REPO, "tools", "clip_draws_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, k, size, train, seed, stream_base, step, B, lengths, index=None, order=None, noise_lengths=None, expect=0):
    lst = lambda v: ",".join(str(int(x)) for x in v)
    args = [f"B={B}", f"S={size}", f"train={int(train)}", f"mode0={k['pad_modes'][0]}", f"mode1={k['pad_modes'][1]}", f"M={k['num_masks']}",
            f"wrap={k['wrap_pad_prob']!r}", f"gainp={k['gain_prob']!r}", f"glo={k['gain_db'][0]!r}", f"ghi={k['gain_db'][1]!r}",
            f"tperc={k['time_perc']!r}", f"noisep={k['noise_prob']!r}", f"snrlo={k['snr_range'][0]!r}", f"snrhi={k['snr_range'][1]!r}",
            f"gaussp={k['gaussian_prob']!r}", f"alo={k['gaussian_amplitude'][0]!r}", f"ahi={k['gaussian_amplitude'][1]!r}",
            f"seed={seed}", f"base={stream_base}", f"step={step}", f"lengths={lst(lengths)}"]
    if noise_lengths is not None:
        args.append(f"nlengths={lst(noise_lengths)}")
    args.append(f"index={lst(index)}" if index is not None else f"order={lst(order)}")
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == expect, (run.returncode, run.stderr)
    if expect:
        return None
    M = k["num_masks"]
    cols = {n: [] for n in ("index", "rec_off", "rec_len", "start", "pad_mode", "gain", "masks", "noise_off", "noise_len", "noise_start",
                            "noise_pad_mode", "coeff", "gauss_amp", "gauss_stream")}
    unbits = lambda h: np.array([int(h, 16)], dtype=np.uint32).view(np.float32)[0]
    lines = run.stdout.splitlines()
    assert len(lines) == B
    for b, line in enumerate(lines):
        head, masks, noise, gauss = (part.split() for part in line.split("|"))
        assert int(head[0]) == b and len(masks) == 2 * M
        for name, v in zip(("index", "rec_off", "rec_len", "start", "pad_mode"), head[1:6]):
            cols[name].append(int(v))
        cols["gain"].append(unbits(head[6]))
        cols["masks"].append(np.array(masks, dtype=np.int64).reshape(M, 2))
        if noise:
            for name, v in zip(("noise_off", "noise_len", "noise_start", "noise_pad_mode"), noise[:4]):
                cols[name].append(int(v))
            cols["coeff"].append([unbits(noise[4]), unbits(noise[5])])
        if gauss:
            cols["gauss_amp"].append(unbits(gauss[0]))
            cols["gauss_stream"].append(int(gauss[1]))
    return {n: np.array(v) for n, v in cols.items() if len(v) == B and not (n == "masks" and M == 0)}


S = 64
LENGTHS = (1, 7, S - 1, S, S + 1, 3 * S + 5)
NOISE_LENGTHS = (5, S, 2 * S + 1)
FULL = consts(num_masks=3, time_perc=0.3, gain_prob=0.5, noise_prob=0.6, gaussian_prob=0.5)


@pytest.mark.parametrize("case", [
    dict(B=1, index=[5]), dict(B=5, index=[0, 1, 2, 3, 5], step=2), dict(B=300, index=list(range(6)) * 50, step=7, stream_base=2 ** 40),
    dict(B=6, index=list(range(6)), train=False), dict(B=7, order=[3, 5, 5, 0], step=3), dict(B=7, order=[-5, 15, 5, 2], step=1),
    dict(B=5, index=[5] * 5, step=2 ** 64 - 1, stream_base=2 ** 64 - 3), dict(B=5, order=[5, 4], step=2 ** 63 + 11, seed=2 ** 64 - 1),
    dict(B=4, index=[5, 4, 3, 2], k=consts(num_masks=32, time_perc=1.0, gaussian_prob=1.0)),
    dict(B=4, index=[5, 4, 3, 2], k=consts(num_masks=2, time_perc=7.5, gain_prob=1.0, gain_db=(-60.0, 40.0), pad_modes=(3, 0), wrap_pad_prob=0.9)),
    dict(B=3, index=[5, 5, 5], noise=None), dict(B=3, index=[5, 5, 5], k=consts()),
])
def test_the_header_draws_what_the_oracle_draws(tool, case):
    case = dict(case)
    k, noise = case.pop("k", FULL), case.pop("noise", NOISE_LENGTHS)
    args = dict(size=S, train=case.pop("train", True), seed=case.pop("seed", 0x1234_5678_9abc_def0), stream_base=case.pop("stream_base", 0),
                step=case.pop("step", 0), B=case.pop("B"), lengths=LENGTHS, index=case.pop("index", None), order=case.pop("order", None),
                noise_lengths=noise)
    assert not case
    got, want = run_tool(tool, k, **args), plan_ref(k, **args)
    assert {"index", "rec_off", "rec_len", "start", "pad_mode", "gain"} <= set(got)
    assert ("masks" in got) == (k["num_masks"] > 0) and ("coeff" in got) == (noise is not None) and ("gauss_amp" in got) == (k["gaussian_prob"] > 0)
    compare(got, want)
    # ... and the plan is one `clip_plan` / `noise_plan` accept: inside the store, start inside its span, coefficients in [0, 1]
    store_len = int(sum(LENGTHS))
    B = args["B"]
    t = lambda name: torch.from_numpy(np.asarray(got[name]))
    _native.clip_plan(store_len, t("rec_off"), t("rec_len"), t("start"), t("pad_mode"), S, t("gain"), t("masks") if "masks" in got else None)
    if noise is not None:
        _native.noise_plan(int(sum(noise)), t("noise_off"), t("noise_len"), t("noise_start"), t("noise_pad_mode"), t("coeff"), S, B)
    if "masks" in got:
        m = got["masks"]
        assert bool(((m[..., 1] >= 0) & (m[..., 0] >= 0) & (m[..., 0] + m[..., 1] <= S)).all())


def test_the_tool_refuses_what_the_entry_refuses(tool):
    for bad in (dict(B=0, index=[]), dict(B=2, index=[0]), dict(B=1, index=[0], k=consts(num_masks=33)), dict(B=1, index=[0], size=0),
                dict(B=1, index=[0], k=consts(pad_modes=(4, 0)))):
        run_tool(tool, bad.pop("k", FULL), bad.pop("size", S), True, 1, 0, 0, bad.pop("B"), LENGTHS, index=bad.pop("index"), expect=3)


# ---- the distributions ----------------------------------------------------------------------------------------------------------------

N_CLIPS = 20000
DIST_SEED = 2024                                        # fixed: the checks below are deterministic, and pass with this seed


@pytest.fixture(scope="module")
def many(tool):
    k = consts(wrap_pad_prob=0.5, gain_prob=0.25, noise_prob=0.6, gaussian_prob=0.3, num_masks=3, time_perc=0.2)
    args = dict(size=S, train=True, seed=DIST_SEED, stream_base=0, step=0, B=N_CLIPS, lengths=(S + 10,), order=[0], noise_lengths=(S + 3, 2 * S))
    got = run_tool(tool, k, **args)
    compare(got, plan_ref(k, **args))                   # 20 000 clips of the header against the oracle, field by field
    return k, got


def test_frequencies_are_binomial(many):
    k, got = many
    n = N_CLIPS
    for name, count, p in (("pad mode", int((got["pad_mode"] == k["pad_modes"][0]).sum()), k["wrap_pad_prob"]),
                           ("gain", int((got["gain"] != 1.0).sum()), k["gain_prob"]),
                           ("noise", int((got["noise_len"] > 0).sum()), k["noise_prob"]),
                           ("gaussian", int((got["gauss_amp"] != 0.0).sum()), k["gaussian_prob"])):
        assert abs(count - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (name, count, n * p)


def test_start_is_uniform_over_its_span(many):
    _, got = many
    counts = np.bincount(got["start"], minlength=11)
    assert counts.size == 11 and int(counts.min()) > 0                       # a span of 10: the values 0 .. 10, every one hit
    expected = N_CLIPS / 11
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert chi2 < 29.588, chi2                                               # the 99.9 % quantile of chi-square with 10 degrees of freedom


def test_the_other_draws_stay_in_their_ranges(many):
    k, got = many
    g = got["gain"][got["gain"] != 1.0].astype(np.float64)
    assert 10 ** (-18 / 20) * (1 - 1e-6) <= g.min() and g.max() <= 10 ** (6 / 20) * (1 + 1e-6)
    a = got["gauss_amp"][got["gauss_amp"] != 0]
    assert 0.001 <= a.min() and a.max() <= np.float32(0.015)
    c = got["coeff"].astype(np.float64)
    snr = 10 * np.log10(c[:, 0] / c[:, 1])
    assert snr.min() >= 10 - 1e-3 and snr.max() <= 26 + 1e-3 and abs(snr.mean() - 18.0) < 5 * 16 / math.sqrt(12 * N_CLIPS)
    assert set(np.unique(got["noise_off"]).tolist()) == {0, S + 3}            # both noise recordings are chosen
    long = got["noise_len"] == 2 * S
    assert got["noise_start"][long].min() == 0 and got["noise_start"][long].max() == S and set(got["noise_pad_mode"].tolist()) == {2}
    m = got["masks"]
    used = (m[..., 1] > 0).sum(axis=1)
    assert m[..., 1].max() <= int(0.2 * S) and used.max() == 3 and bool((m[..., 0] + m[..., 1] <= S).all())
    assert np.array_equal(got["gauss_stream"], np.arange(N_CLIPS))            # the id of clip b at step 0, base 0


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------

CTYPE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "double": ctypes.c_double}


def test_the_entry_is_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    m = re.search(r"int leaf_draw_clip_plan\(([^)]*)\);", flat)
    assert m
    declared = [ctypes.c_void_p if "*" in a else CTYPE[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(1).split(",")]
    i, v, ll, ull, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double
    want = [i, i, i, v, v, i, v, v, i, v, v, ll, v, i, ull, ull, i, i, d, d, d, d, i, d, d, d, d, d, d, d] + [v] * 15 + [v]
    assert declared == want == _native._SIGNATURES["leaf_draw_clip_plan"][1] and _native._SIGNATURES["leaf_draw_clip_plan"][0] == i
    assert "leaf_draw_clip_plan" in _native.EXPORTED_SYMBOLS and "leaf_draw_clip_plan" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    lib = _native.load()
    fn = lib.leaf_draw_clip_plan
    assert fn.restype == i and fn.argtypes == want and lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "leaf_draw_clip_plan" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    src = open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_clip_draws.hpp")).read()
    assert f"kDrawMaxMasks = {_native.DRAW_MAX_MASKS};" in src and "kDrawNoiseCounter = 64u, kDrawGaussCounter = 65u" in src
    assert "kDrawLn10 = 2.302585092994045684;" in src
    assert callable(_native.draw_clip_plan) and leaf_pytorch_amd.DeviceClipSampler is DeviceClipSampler


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch
    outs = ("rec_off", "rec_len", "start", "pad_mode", "gain", "masks", "rec", "noise_off", "noise_len", "noise_start", "noise_pad_mode",
            "noise_coeff", "gauss_amp", "gauss_stream", "index_out")

    def call(B=4, size=16, train=1, offsets=p, lengths=p, R=3, noise_offsets=p, noise_lengths=p, Rn=2, index=p, order=None, N=0, state=p,
             advance=1, seed=1, stream_base=0, mode_a=2, mode_b=1, M=2, **kw):
        ptrs = [kw.pop(name, p) for name in outs]
        assert not kw
        return lib.leaf_draw_clip_plan(B, size, train, offsets, lengths, R, noise_offsets, noise_lengths, Rn, index, order, N, state, advance,
                                       seed, stream_base, mode_a, mode_b, 0.5, 0.25, -18.0, 6.0, M, 0.1, 0.5, 10.0, 25.0, 0.5, 0.001, 0.015,
                                       *ptrs, None)

    noise_group = ("noise_offsets", "noise_lengths", "noise_off", "noise_len", "noise_start", "noise_pad_mode", "noise_coeff")
    for name in ("offsets", "lengths", "state", "rec_off", "rec_len", "start", "pad_mode") + noise_group + ("gauss_amp", "gauss_stream"):
        assert call(**{name: None}) == NULL_POINTER, name                                  # required, or a group given in part
    assert call(index=None) == NULL_POINTER and call(order=p, N=5) == NULL_POINTER         # neither, and both
    assert call(index=None, order=p, N=5, B=0) == BAD_SHAPE                                # (the order form is taken)
    for kw in (dict(B=0), dict(B=-1), dict(size=0), dict(size=-5), dict(R=0), dict(M=-1), dict(M=33), dict(M=2, masks=None), dict(Rn=0),
               dict(index=None, order=p, N=0), dict(index=None, order=p, N=-1), dict(mode_a=4), dict(mode_b=-1)):
        assert call(**kw) == BAD_SHAPE, kw
    assert call(B=0, state=None) == NULL_POINTER and call(B=0, state=p + 4) == BAD_SHAPE   # the order of the checks
    no_noise = {k: None for k in noise_group}
    assert call(Rn=0, state=p + 4, **no_noise) == ALIGNMENT                                # without the group Rn is not looked at
    for name in ("offsets", "noise_offsets", "index", "state", "rec_off", "noise_off", "gauss_stream", "index_out"):
        assert call(**{name: p + 4}) == ALIGNMENT, name
    assert call(index=None, order=p + 4, N=3) == ALIGNMENT
    for name in ("lengths", "noise_lengths", "rec_len", "start", "pad_mode", "gain", "masks", "rec", "noise_len", "noise_start", "noise_pad_mode",
                 "noise_coeff", "gauss_amp"):
        assert call(**{name: p + 2}) == ALIGNMENT, name


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_the_sampler_needs_the_device_and_checks_its_constants_first():
    clips = PackedClips([torch.zeros(n, dtype=torch.int16) for n in LENGTHS])
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        DeviceClipSampler(clips, S, seed=3)
    for bad in (dict(num_masks=33), dict(num_masks=-1), dict(pad_modes=("replicate",)), dict(pad_modes=("replicate", 7))):
        with pytest.raises(ValueError):
            DeviceClipSampler(clips, S, seed=3, **bad)
    with pytest.raises(ValueError):
        DeviceClipSampler(clips, 0, seed=3)
    with pytest.raises(TypeError):
        DeviceClipSampler(clips, S, noise_clips=PackedClips([torch.zeros(8)]), seed=3)
    # the keywords and defaults the two samplers share are the same
    import inspect
    a, b = (inspect.signature(c.__init__).parameters for c in (leaf_pytorch_amd.ClipSampler, DeviceClipSampler))
    shared = [n for n in a if n in b and n != "self"]
    assert set(a) - set(b) == {"generator"} and set(b) - set(a) == {"seed", "stream_base", "order", "batch_size"}
    assert all(a[n].default == b[n].default for n in shared)
    assert "32-bit" in DeviceClipSampler.__doc__
