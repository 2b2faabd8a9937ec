"""Host-side contract of the self-validating table cache (include/leaf_hip.h: leaf_table_cache_bytes, leaf_forward_cached_f32): what
the header declares and the library exports, the size query, and the refusals that answer before any launch (dummy host pointers: no
GPU is needed)."""
import ctypes
import os
import re

from leaf_pytorch_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("leaf_table_cache_bytes", "leaf_forward_cached_f32")
F, K, HOP = 40, 401, 160
L, PADL, MAX_EDGE = 1600, 200, 12               # block length and left padding of the 401 / 160 geometry; kBandMaxEdge
LPHI = 12 * 8                                   # band_lphi(16): half length of the widest decimation filter, in samples
STAMP_BYTES = 128                               # kStampWords * 4


def edge_entries(T):
    """The edge list of csrc/leaf_kernels.hip (band_edges), restated: (frame, block) pairs of the frames whose widened pooling window
    is cut by the clip's ends; None where the tables cannot hold them (then the call runs no band tasks)."""
    TP = (T - 1) // HOP + 1
    lo = -(-(PADL + LPHI) // HOP)
    hi = (T - K - LPHI + PADL) // HOP if T - K - LPHI + PADL >= 0 else -1
    hi = min(hi, TP - 1)
    if hi < lo:
        lo, hi = TP, TP - 1
    n = 0
    for m in range(TP):
        if lo <= m <= hi:
            continue
        ws = m * HOP - PADL
        c = max(0, ws) // L
        while c * L < min(T, ws + K):
            a, b = max(c * L, 0, ws), min((c + 1) * L, T, ws + K)
            if a < b:
                if n == MAX_EDGE:
                    return None
                n += 1
            c += 1
    return n


def test_header_declares_the_entries_and_the_abi_version_stays():
    header = open(os.path.join(REPO, "include", "leaf_hip.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\(", header), name
    assert re.search(r"#define LEAF_ALGO_NO_TABLE_CACHE \(1 << 28\)", header)
    assert _native.ALGO_NO_TABLE_CACHE == 1 << 28
    assert int(re.search(r"#define LEAF_ABI_VERSION (\d+)", header).group(1)) == 6
    assert _native.ABI_VERSION == 6 and _native.load().leaf_abi_version() == 6
    for name in ENTRIES:
        assert name in _native._SIGNATURES and name in _native.EXPORTED_SYMBOLS


def test_cache_bytes_grow_with_the_number_of_edge_entries():
    lib = _native.load()
    sizes = {}
    for T in (16000, 12345, 4000, 20000, 1600, 801, 700, 400, 161, 1):
        n = edge_entries(T)
        nbytes = lib.leaf_table_cache_bytes(F, K, HOP, T)
        assert nbytes > 0 and nbytes % 16 == 0, (T, nbytes)
        sizes.setdefault(0 if n is None else n, set()).add(nbytes)
    assert len(sizes) >= 3, sizes                            # the clip lengths above do differ in their edge lists
    assert all(len(v) == 1 for v in sizes.values()), sizes   # the size depends on T through the number of edge entries alone
    counts = sorted(sizes)
    by_count = [next(iter(sizes[n])) for n in counts]
    # monotone, and exactly one stamp per filter and edge entry apart
    for (n0, b0), (n1, b1) in zip(zip(counts, by_count), zip(counts[1:], by_count[1:])):
        assert b1 - b0 == (n1 - n0) * F * STAMP_BYTES, (n0, b0, n1, b1)
    # the tables of leaf_fft_prepare_tables_f32 are part of it
    assert by_count[0] > lib.leaf_fft_tables_bytes(F, K, HOP)


def test_cache_bytes_are_zero_without_a_2048_sample_plan():
    lib = _native.load()
    assert lib.leaf_table_cache_bytes(F, 2001, 800, 16000) == 0        # a window beyond the 2048-sample plan (K <= 1217)
    assert lib.leaf_table_cache_bytes(F, 1, 1, 16000) == 0             # ... and below it
    assert lib.leaf_table_cache_bytes(0, K, HOP, 16000) == 0 and lib.leaf_table_cache_bytes(F, K, HOP, 0) == 0
    # geometries without band tasks have a 2048-sample plan too: one stamp per filter, whatever the clip length
    a, b = lib.leaf_table_cache_bytes(12, 201, 80, 8000), lib.leaf_table_cache_bytes(12, 201, 80, 123)
    assert a == b == lib.leaf_fft_tables_bytes(12, 201, 80) + 12 * STAMP_BYTES


def test_refusals_answer_before_any_launch():
    """Dummy host pointers: a launch on them would fault, so the status codes alone show that nothing ran."""
    lib = _native.load()
    host = (ctypes.c_char * 8192)()
    base = ctypes.addressof(host)
    base += (-base) % 64
    p = lambda off=0: ctypes.c_void_p(base + off)
    B, T = 24, 16000
    ws_bytes = lib.leaf_workspace_bytes(B, T, F, K, HOP, _native.ALGO_FFT_WG)
    need = lib.leaf_table_cache_bytes(F, K, HOP, T)
    call = lambda cache, cache_bytes, algo=_native.ALGO_FFT_WG, ws=ws_bytes: lib.leaf_forward_cached_f32(
        p(), B, T, p(), p(), p(), p(), p(), p(), p(), F, K, HOP, _native.FLAG_PCEN, algo, p(), p(), ws, cache, cache_bytes, None)
    assert call(p(4), need) == -7                            # LEAF_ERR_ALIGNMENT: the cache needs 16 bytes like the workspace
    assert call(p(), need - 1) == -3                         # LEAF_ERR_WORKSPACE
    assert call(p(), need, ws=ws_bytes - 1) == -3            # the workspace check is leaf_forward_f32's
    assert call(p(4), need, algo=_native.ALGO_FFT_WG | _native.ALGO_NO_TABLE_CACHE) == -7   # alignment is checked on every route
    assert call(p(), need, algo=99) == -4                    # LEAF_ERR_BAD_ALGO, as leaf_forward_f32
