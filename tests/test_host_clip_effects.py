"""ClipValue and the sox-style reverb (leaf_clip_effects_f32), the host side (no GPU): a NumPy oracle written from the definition in
include/leaf_hip.h -- ``np.float32`` scalars and plain Python loops, every operation rounded on its own -- compared bit for bit with
the sequential definition in csrc/leaf_clip_effects.hpp (through tools/clip_effects_check.cpp compiled with plain g++); the plan
arithmetic of ``_native.reverb_plan``; the C entry as declared and exported, and its argument checks; the validation of a plan that
arrives on the CPU; ``EffectsClipSampler``'s draws.  tests/test_gpu_clip_effects.py compares the kernel with the oracle and the
cases defined here."""
import ctypes
import functools
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import leaf_pytorch_amd
from leaf_pytorch_amd import ClipSampler, EffectsClipSampler, PackedClips, _native, transforms

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_SHAPE, ALIGNMENT, UNSUPPORTED = -1, -2, -7, -8
F = np.float32
WET = 0.015
COMB_TUNING = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_TUNING = (225, 341, 441, 556)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------

def lengths_ref(sample_rate, room_scale):
    """(comb, allpass) by the header's formulas, in double."""
    r = sample_rate / 44100
    scale = room_scale / 100 * 0.9 + 0.1
    return [int(scale * r * c + 0.5) for c in COMB_TUNING], [int(r * a + 0.5) for a in ALLPASS_TUNING]


def feedback_ref(reverberance):
    a = -1 / math.log(1 - 0.3)
    b = 100 / (math.log(1 - 0.98) * a + 1)
    return 1 - math.exp((reverberance - b) / (a * b))


def clip_value_ref(x, factor):
    """ClipValue on one clip: bounds from the exact minimum and maximum (a zero counting as +0), then min(max(x, lo), hi)."""
    factor = F(factor)
    if factor < 0:
        return np.array(x, dtype=np.float32)
    lo, hi = (F(x.min()) + F(0)) * factor, (F(x.max()) + F(0)) * factor
    y = np.empty(len(x), dtype=np.float32)
    for n in range(len(x)):
        m = lo if x[n] < lo else x[n]
        y[n] = hi if hi < m else m
    return y


def reverb_ref(x, feedback, damp, comb, allpass, wet=WET):
    """The reverb on one clip, sample after sample as the header writes it."""
    fb, dp, wet, half, zero = F(feedback), F(damp), F(wet), F(0.5), F(0)
    cb, ap = [[zero] * int(n) for n in comb], [[zero] * int(n) for n in allpass]
    p, q, store = [0] * 8, [0] * 4, [zero] * 8
    y = np.empty(len(x), dtype=np.float32)
    for n in range(len(x)):
        inp, out = F(x[n]), zero
        for i in range(7, -1, -1):
            line, at = cb[i], p[i]
            o = line[at]
            s = o + (store[i] - o) * dp
            store[i] = s
            line[at] = inp + s * fb
            p[i] = at + 1 if at + 1 < len(line) else 0
            out = out + o
        for j in range(3, -1, -1):
            line, at = ap[j], q[j]
            o = line[at]
            line[at] = out + o * half
            q[j] = at + 1 if at + 1 < len(line) else 0
            out = o - out
        y[n] = inp + out * wet
    return y


def effects_ref(x, factor, feedback, damp, comb, sample_rate, wet=WET):
    """(B, S) float32: both steps per clip.  ``comb`` rows with comb[0] <= 0 skip the reverb; the other lengths are clamped into
    [1, cap] as the kernel clamps them (a validated plan is inside already)."""
    caps, allpass = lengths_ref(sample_rate, 100)
    y = np.empty(x.shape, dtype=np.float32)
    for b in range(x.shape[0]):
        v = clip_value_ref(x[b], -1.0 if factor is None else factor[b])
        if comb is not None and comb[b][0] > 0:
            v = reverb_ref(v, feedback[b], damp[b], [min(max(int(c), 1), cap) for c, cap in zip(comb[b], caps)], allpass, wet)
        y[b] = v
    return y


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- the cases (tests/test_gpu_clip_effects.py runs the kernel on the same ones) ---------------------------------------------------------

S_LIST = (1, 19, 20, 21, 63, 64, 65, 587, 588, 1500)
RATES = (8000, 16000, 48000)
SKIP = None


def signal(kind, S, seed):
    if kind == "noise":
        return np.random.RandomState(seed).uniform(-1.0, 1.0, S).astype(np.float32)
    x = np.zeros(S, dtype=np.float32)
    x[{"impulse": 0, "late": S // 2}[kind]] = 1.0
    return x


def _cases():
    """id -> (sample_rate, S, clips): a clip is (signal kind, factor, (reverberance, damping, room_scale) or SKIP)."""
    cases = {}
    for rate in RATES:
        for room in (0, 100):
            for S in S_LIST:                                                    # one clip, uniform noise
                cases[f"{rate}-room{room}-S{S}-B1"] = (rate, S, [("noise", -1.0, (50, 30, room))])
            cases[f"{rate}-room{room}-S1500-impulse"] = (rate, 1500, [("impulse", -1.0, (50, 30, room))])
        for S in S_LIST if rate == 16000 else (65, 588):                        # five clips, every one its own plan, one skipped
            cases[f"{rate}-S{S}-B5"] = (rate, S, [("impulse", -1.0, (10, 10, 0)), ("noise", -1.0, (50, 50, 100)), ("noise", -1.0, SKIP),
                                                  ("noise", -1.0, (100, 0, 37)), ("late", -1.0, (0, 100, 0))])
    cases["16000-S16000"] = (16000, 16000, [("noise", -1.0, (50, 50, 50))])
    cases["8000-subnormal-tail"] = (8000, 16000, [("impulse", -1.0, (10, 50, 0))])
    # ClipValue alone: extremes at the first and last sample, a non-negative clip, factor 0, a skipped clip; one sample
    cases["clipvalue-S37"] = (16000, 37, [("edges", 0.5, SKIP), ("positive", 0.25, SKIP), ("noise", 0.0, SKIP), ("noise", -1.0, SKIP),
                                          ("noise", 0.1, SKIP), ("noise", 1.0, SKIP)])
    cases["clipvalue-S1"] = (16000, 1, [("noise", 0.5, SKIP), ("noise", -2.0, SKIP), ("noise", 0.0, SKIP)])
    # both steps in one call
    cases["both-S588"] = (16000, 588, [("noise", 0.15, (50, 50, 100)), ("noise", 0.05, SKIP), ("noise", -1.0, (30, 20, 0)), ("noise", 0.2, (10, 10, 50))])
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=None)
def build(case_id):
    """(sample_rate, x (B, S), factor (B,), feedback (B,), damp (B,), comb (B, 8)) of a case, NumPy arrays; a skipped reverb is a row
    of zeros."""
    rate, S, clips = CASES[case_id]
    B = len(clips)
    x = np.empty((B, S), dtype=np.float32)
    factor, feedback, damp = np.empty(B, dtype=np.float32), np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
    comb = np.zeros((B, 8), dtype=np.int32)
    for b, (kind, f, rev) in enumerate(clips):
        seed = 1000 * b + S
        if kind == "edges":                                                     # the minimum is the first sample, the maximum the last
            x[b] = signal("noise", S, seed) * 0.5
            x[b, 0], x[b, -1] = -0.9, 0.8
        elif kind == "positive":
            x[b] = np.abs(signal("noise", S, seed)) + np.float32(0.125)
        else:
            x[b] = signal(kind, S, seed)
        factor[b] = f
        if rev is not SKIP:
            fb, dp, cm = _native.reverb_plan([rev[0]], [rev[1]], [rev[2]], rate)
            feedback[b], damp[b], comb[b] = fb.numpy()[0], dp.numpy()[0], cm.numpy()[0]
    return rate, x, factor, feedback, damp, comb


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    rate, x, factor, feedback, damp, comb = build(case_id)
    return effects_ref(x, factor, feedback, damp, comb, rate)


def test_the_cases_cover_what_they_claim():
    assert lengths_ref(8000, 0)[0][0] == 20 and min(lengths_ref(8000, 0)[0] + lengths_ref(8000, 0)[1]) == 20     # the shortest line
    caps, allpass = lengths_ref(48000, 100)
    assert 54000 < 4 * (sum(caps) + sum(allpass)) < 56000                      # the largest layout, about 55 KB
    tail = oracle("8000-subnormal-tail")[0]
    mag = np.abs(tail[tail != 0])
    assert mag.min() < np.finfo(np.float32).tiny and (mag < np.finfo(np.float32).tiny).sum() > 100             # it decays into subnormals
    assert not np.array_equal(oracle("16000-room0-S1500-B1"), build("16000-room0-S1500-B1")[1])
    y = oracle("clipvalue-S37")
    x = build("clipvalue-S37")[1]
    assert y[0].min() == F(-0.45) and y[0].max() == F(0.4) and y[1].min() > 0 and not y[2].any() and np.array_equal(bits(y[3]), bits(x[3]))


# ---- the header's sequential definition, through tools/clip_effects_check.cpp -----------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path_factory.mktemp("clip_effects") / "clip_effects_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(REPO, "leaf_pytorch_amd", "csrc"),
                    os.path.join(REPO, "tools", "clip_effects_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, path, rate, x, factor, feedback, damp, comb, wet=WET, expect=0):
    B, S = x.shape
    with open(path, "w") as fh:
        fh.write(f"{rate} {int(bits(F(wet)).reshape(-1)[0]):08x} {B} {S}\n")
        for b in range(B):
            head = " ".join(f"{int(w):08x}" for w in bits([factor[b], feedback[b], damp[b]]))
            fh.write(head + " " + " ".join(str(int(c)) for c in comb[b]) + "\n" + " ".join(f"{int(w):08x}" for w in bits(x[b])) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == expect, (run.returncode, run.stderr)
    if expect:
        return None
    lines = run.stdout.splitlines()
    assert len(lines) == B
    return np.array([[int(w, 16) for w in line.split()] for line in lines], dtype=np.uint32).reshape(B, S)


@pytest.mark.parametrize("case_id", sorted(CASES))
def test_the_header_computes_what_the_oracle_computes(tool, tmp_path, case_id):
    got = run_tool(tool, tmp_path / "plan.txt", *build(case_id))
    want = bits(oracle(case_id))
    assert np.array_equal(got, want), (case_id, int((got != want).sum()))


def test_the_tool_clamps_hostile_lengths_and_refuses_what_the_entry_refuses(tool, tmp_path):
    run = subprocess.run([tool, "hostile"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("hostile ok"), (run.returncode, run.stdout, run.stderr)
    x = signal("noise", 200, 3).reshape(1, 200)
    one = np.ones(1, dtype=np.float32)
    comb = np.array([[10 ** 9, 0, -7, 10 ** 9, 3, 0, -7, 10 ** 9]], dtype=np.int32)
    got = run_tool(tool, tmp_path / "hostile.txt", 16000, x, -one, one * F(0.5), one * F(0.3), comb)
    assert np.array_equal(got, bits(effects_ref(x, -one, one * F(0.5), one * F(0.3), comb, 16000)))
    for rate in (50, 96000):                                                    # an all-pass of 0 samples; lines beyond the LDS budget
        run_tool(tool, tmp_path / "refused.txt", rate, x, -one, one, one, comb, expect=3)


# ---- the plan arithmetic ---------------------------------------------------------------------------------------------------------------

def test_reverb_plan_is_the_formulas_in_double():
    assert feedback_ref(0) == pytest.approx(0.30, abs=1e-12) and feedback_ref(100) == pytest.approx(0.98, abs=1e-12)
    assert feedback_ref(50) == pytest.approx(0.8816, abs=1e-4)                   # 0.88168
    for rate in (8000, 16000, 44100, 48000):
        for room in (0, 37, 100):
            fb, dp, comb = _native.reverb_plan([0, 50, 100], [0, 50, 100], [room] * 3, rate)
            assert fb.dtype == torch.float32 and dp.dtype == torch.float32 and comb.dtype == torch.int32 and tuple(comb.shape) == (3, 8)
            assert np.array_equal(bits(fb.numpy()), bits([F(feedback_ref(v)) for v in (0, 50, 100)]))
            assert np.array_equal(bits(dp.numpy()), bits([F(v / 100 * 0.3 + 0.2) for v in (0, 50, 100)]))
            want_comb, want_allpass = lengths_ref(rate, room)
            assert comb.tolist() == [want_comb] * 3
            assert _native.reverb_lengths(rate, room) == (want_comb, want_allpass)
    assert lengths_ref(44100, 100) == (list(COMB_TUNING), list(ALLPASS_TUNING))
    assert _native.reverb_lengths(16000, 0)[0] == [40, 43, 46, 49, 52, 54, 56, 59] and _native.reverb_lengths(16000)[1] == [82, 124, 160, 202]
    fb, dp, comb = _native.reverb_plan(torch.tensor([10, 50]), torch.tensor([10, 50]), torch.tensor([0, 100]), 16000)     # tensors; per clip
    assert comb.tolist() == [lengths_ref(16000, 0)[0], lengths_ref(16000, 100)[0]]
    assert tuple(t.numel() for t in _native.reverb_plan(50, 50, 50, 16000)) == (1, 1, 8)
    assert _native.reverb_plan([50], [50], [100], 150)[2][0, 0] == 4            # 1116 * 150 / 44100 + 0.5 = 4.29
    with pytest.raises(ValueError):
        _native.reverb_plan([50], [50], [0], 150)                               # ... and a tenth of it: comb 0 would have 0 samples
    with pytest.raises(ValueError):
        _native.reverb_plan([50], [50], [100], 50)                              # all-pass 0: 225 * 50 / 44100 + 0.5 < 1
    for bad in (([50, 50], [50], [50]), ([101], [50], [50]), ([50], [-1], [50]), ([50], [50], [float("nan")])):
        with pytest.raises(ValueError):
            _native.reverb_plan(*bad, 16000)


# ---- the C entry -------------------------------------------------------------------------------------------------------------------------

def test_the_entry_is_declared_as_exported():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    m = re.search(r"int leaf_clip_effects_f32\(([^)]*)\);", flat)
    assert m
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    declared = [ctypes.c_void_p if "*" in a else ctype[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(1).split(",")]
    i, v, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    want = [v, v, i, i, v, v, v, v, i, f, v]
    assert declared == want == _native._SIGNATURES["leaf_clip_effects_f32"][1] and _native._SIGNATURES["leaf_clip_effects_f32"][0] == i
    assert "leaf_clip_effects_f32" in _native.EXPORTED_SYMBOLS
    assert "leaf_clip_effects_f32" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6          # additive: the version stays
    lib = _native.load()
    fn = lib.leaf_clip_effects_f32
    assert fn.restype == i and fn.argtypes == want and lib.leaf_abi_version() == 6 and _native.ABI_VERSION == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "leaf_clip_effects_f32" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    src = open(os.path.join(REPO, "leaf_pytorch_amd", "csrc", "leaf_clip_effects.hpp")).read()
    assert "{" + ", ".join(str(c) for c in _native.REVERB_COMB_TUNING) + "}" in src
    assert "{" + ", ".join(str(a) for a in _native.REVERB_ALLPASS_TUNING) + "}" in src and "kFxLdsBudget = 64 * 1024;" in src
    assert _native.REVERB_LDS_BUDGET == 64 * 1024 and _native.REVERB_COMB_TUNING == COMB_TUNING and _native.REVERB_ALLPASS_TUNING == ALLPASS_TUNING
    assert leaf_pytorch_amd.clip_effects is _native.clip_effects and transforms.clip_effects is _native.clip_effects
    assert leaf_pytorch_amd.reverb_plan is _native.reverb_plan and leaf_pytorch_amd.EffectsClipSampler is EffectsClipSampler


def test_argument_checks_are_answered_without_a_device():
    lib = _native.load()
    p = 0x10000                                        # never dereferenced: every call below is refused before the launch
    far = p + (1 << 24)

    def call(x=p, y=far, B=2, S=100, factor=p, feedback=p, damp=p, comb=p, rate=16000, wet=WET):
        return lib.leaf_clip_effects_f32(x, y, B, S, factor, feedback, damp, comb, rate, wet, None)

    assert call(x=None) == NULL_POINTER and call(y=None) == NULL_POINTER
    for part in ("feedback", "damp", "comb"):          # the reverb group given in part
        assert call(**{part: None}) == NULL_POINTER, part
    for kw in (dict(B=0), dict(B=-1), dict(S=0), dict(S=-3), dict(B=1 << 16, S=1 << 15), dict(y=p), dict(y=p + 400), dict(x=far, y=far - 796),
               dict(rate=0), dict(rate=-16000), dict(rate=50)):
        assert call(**kw) == BAD_SHAPE, kw
    for name in ("x", "y", "factor", "feedback", "damp", "comb"):
        base = far if name == "y" else p
        assert call(**{name: base + 2}) == ALIGNMENT, name
    assert call(rate=96000) == UNSUPPORTED and call(rate=60000) == UNSUPPORTED            # the lines do not fit 64 KB
    assert call(rate=0, feedback=None, damp=None, comb=None, x=p + 2) == ALIGNMENT         # without the group the rate is not looked at
    assert call(B=0, x=None) == NULL_POINTER           # the order of the checks


# ---- the Python layer: validation of a plan on the CPU ----------------------------------------------------------------------------------

def test_a_bad_cpu_plan_raises_before_the_device_is_looked_at():
    x = torch.zeros(2, 1, 64)                          # a CPU batch: a valid plan gets as far as require_hip and no further
    fb, dp, comb = _native.reverb_plan([50, 50], [50, 50], [0, 100], 16000)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.clip_effects(x, [0.1, -1.0], (fb, dp, comb))
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
        _native.clip_effects(x[:, 0], None, (fb * 0, dp * 0, comb * 0))         # all skipped: nothing to validate in the rows
    bad_comb = comb.clone()
    bad_comb[1, 7] += 1                                # one past its cap
    neg = comb.clone()
    neg[0, 3] = 0
    for kw in (dict(clip_factor=[0.1]), dict(clip_factor=[0.1, float("nan")]), dict(clip_factor=[float("inf"), 0.1]),
               dict(reverb=(fb, dp, bad_comb)), dict(reverb=(fb, dp, neg)), dict(reverb=(fb, dp, comb[:1])), dict(reverb=(fb[:1], dp, comb)),
               dict(reverb=(torch.tensor([0.5, 1.0]), dp, comb)), dict(reverb=(fb, torch.tensor([-0.1, 0.5]), comb)),
               dict(reverb=(fb, dp)), dict(reverb=(fb, dp, comb), sample_rate=96000), dict(reverb=(fb, dp, comb), sample_rate=50),
               dict(wet=float("inf"))):
        with pytest.raises(ValueError):
            _native.clip_effects(x, **kw)
    with pytest.raises(TypeError):
        _native.clip_effects(x, reverb=(fb, dp, comb.float()))
    for bad_x in (torch.zeros(2, 2, 64), torch.zeros(2, 64, dtype=torch.float64), torch.zeros(2, 128)[:, ::2]):
        with pytest.raises(RuntimeError, match="contiguous float32"):
            _native.clip_effects(bad_x)


# ---- EffectsClipSampler's plan -----------------------------------------------------------------------------------------------------------

LENGTHS = (5, 16, 16, 40, 100, 1, 17)
SIZE = 16


def _clips():
    g = torch.Generator().manual_seed(5)
    return PackedClips([torch.randint(-3000, 3000, (n,), generator=g).to(torch.int16) for n in LENGTHS])


def test_the_parents_part_of_the_plan_is_what_clip_sampler_draws():
    clips, noise = _clips(), PackedClips([torch.zeros(50, dtype=torch.int16), torch.zeros(9, dtype=torch.int16)])
    index = torch.arange(len(LENGTHS)).repeat(6)
    for kw in (dict(), dict(num_masks=3, time_perc=0.3, gain_prob=0.6), dict(noise_clips=noise, gaussian_prob=0.5, standardize=True, train=False)):
        a = ClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(21), **kw).plan(index)
        e = EffectsClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(21), clip_prob=0.5, reverb_prob=0.5, **kw).plan(index)
        assert isinstance(e, transforms.ClipEffectsPlan) and len(e) == 6
        for u, v in zip(a, e):
            assert (u is None and v is None) or torch.equal(u, v)
        for name in ("noise", "gaussian", "rec"):
            u, v = getattr(a, name, None), getattr(e, name)
            assert (u is None) == (v is None)
            if u is not None:
                pairs = [(u, v)] if name == "rec" else zip(u, v)
                assert all(torch.equal(torch.as_tensor(s), torch.as_tensor(t)) for s, t in pairs)
        assert e.clip_factor.dtype == torch.float32 and e.clip_factor.shape == (index.numel(),)
        assert [t.dtype for t in e.reverb] == [torch.float32, torch.float32, torch.int32] and e.reverb[2].shape == (index.numel(), 8)


N_CLIPS = 20000


def test_the_effect_draws_lie_in_their_ranges_at_their_rates():
    clips = _clips()
    index = torch.zeros(N_CLIPS, dtype=torch.int64)
    s = EffectsClipSampler(clips, SIZE, generator=torch.Generator().manual_seed(2024), clip_prob=0.3, max_clip_val=0.2, reverb_prob=0.6,
                           reverb_range=(10, 50), damping_range=(20, 40), room_scale_range=(0, 100), sample_rate=16000)
    plan = s.plan(index)
    f = plan.clip_factor
    clipped = f >= 0
    assert bool(((f[clipped] >= 0) & (f[clipped] <= F(0.2))).all()) and bool((f[~clipped] == -1).all())
    fb, dp, comb = plan.reverb
    live = comb[:, 0] > 0
    for count, prob, name in ((int(clipped.sum()), 0.3, "ClipValue"), (int(live.sum()), 0.6, "reverb")):
        assert abs(count - N_CLIPS * prob) <= 4 * math.sqrt(N_CLIPS * prob * (1 - prob)), (name, count)
    assert not comb[~live].any() and not fb[~live].any() and not dp[~live].any()
    assert F(feedback_ref(10)) <= fb[live].min() and fb[live].max() <= F(feedback_ref(50))
    assert F(20 / 100 * 0.3 + 0.2) <= dp[live].min() and dp[live].max() <= F(40 / 100 * 0.3 + 0.2)
    caps, floor = lengths_ref(16000, 100)[0], lengths_ref(16000, 0)[0]
    assert bool(((comb[live] >= torch.tensor(floor)) & (comb[live] <= torch.tensor(caps))).all())
    assert int(comb[live][:, 0].min()) == floor[0] and int(comb[live][:, 0].max()) == caps[0]          # both ends are drawn: inclusive
    assert len(set(fb[live].tolist())) == 41 and len(set(dp[live].tolist())) == 21                      # every integer of the ranges
    _native.clip_effects_plan(N_CLIPS, f, plan.reverb, 16000)                                          # and it is a plan the host accepts


def test_a_sampler_without_effects_carries_all_skip_entries_and_checks_its_constants():
    s = EffectsClipSampler(_clips(), SIZE, generator=torch.Generator().manual_seed(3))
    plan = s.plan(torch.arange(len(LENGTHS)).repeat(30))
    assert bool((plan.clip_factor < 0).all()) and not plan.reverb[2].any() and not plan.reverb[0].any() and not plan.reverb[1].any()
    params = inspect.signature(EffectsClipSampler.__init__).parameters
    want = dict(clip_prob=0.0, max_clip_val=0.2, reverb_prob=0.0, reverb_range=(10, 50), damping_range=(10, 50), room_scale_range=(0, 100),
                sample_rate=16000)
    assert {k: params[k].default for k in want} == want
    assert not set(want) & set(inspect.signature(ClipSampler.__init__).parameters)                     # ClipSampler keeps its keywords
    for bad in (dict(reverb_range=(50, 10)), dict(damping_range=(0, 101)), dict(room_scale_range=(-1, 5)), dict(sample_rate=96000),
                dict(sample_rate=50), dict(max_clip_val=-0.1), dict(max_clip_val=float("nan"))):
        with pytest.raises(ValueError):
            EffectsClipSampler(_clips(), SIZE, **bad)
    assert "unpinned" in EffectsClipSampler.__doc__ and "Left out" in EffectsClipSampler.__doc__
