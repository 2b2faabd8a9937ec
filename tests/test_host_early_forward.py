"""Host-side contract of the static workgroup forward kernel's instances (csrc/leaf_fft_wg.hpp: one loader and one tail tile per
instance, the early first-block forward), checkable without a GPU:

* resources -- the code size (ELF symbol table) and the registers / scratch (the AMDGPU metadata note) of every
  ``leaf_fft_wg_kernel<401, 160, 12, ...>`` instance in the BUILT library, against the sizes recorded for the commit before the split
  (profiles/early_forward.txt): 81,728 bytes for the tail-finalize kernel, 72,108 for the streaming-finalize one, <= 168 VGPRs (three
  waves per SIMD), no scratch outside the streaming finalize's explained 48 bytes per lane (tools/kernel_resources.py);
* dispatch -- every (geometry, sample kind, mix, STREAM, tail) combination the kernel table served before has an instance (the
  STREAM instance of a geometry serves every sample kind: it chooses its loader at run time), nothing else has one, and the C ABI
  answers as before for what it refuses.
No instruction is inspected."""
import ctypes
import os
import re
import struct
import subprocess
import tempfile

import pytest

from leaf_pytorch_amd import _native

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
PARENT_BYTES = {False: 81728, True: 72108}                  # leaf_fft_wg_kernel<401, 160, 12, STREAM> before the split
STREAM_SCRATCH = 48                                          # bytes per lane, tools/kernel_resources.py ALLOWED_SCRATCH
MAX_VGPRS = 168                                              # 512 / 3 waves per SIMD, allocation granule 8
GEOMETRIES = ((401, 160, 12), (801, 320, 10), (201, 80, 12))
OTHER_KINDS = ("leaf_inst_fft_wg_x16", "leaf_inst_fft_wg_mix", "leaf_inst_fft_wg_mix16")


def device_code_objects(path):
    """The gfx950 code objects of a library: every clang offload bundle in the file, unbundled by its own table of contents."""
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    for m in re.finditer(magic, data):
        o = m.start()
        n, = struct.unpack_from("<Q", data, o + len(magic))
        q = o + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                yield data[o + off:o + off + size]


def wg_instances():
    """{mangled name: dict(bytes, vgprs, scratch, vgpr_spills)} of the leaf_fft_wg_kernel instances in the built library."""
    out = {}
    for blob in device_code_objects(_native.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".elf") as fh:
            fh.write(blob)
            fh.flush()
            syms = subprocess.run([READELF, "-sW", fh.name], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([READELF, "--notes", fh.name], capture_output=True, text=True, check=True).stdout
        sizes = {}
        for line in syms.splitlines():
            c = line.split()
            if len(c) >= 8 and c[3] == "FUNC" and "leaf_fft_wg_kernel" in c[7]:
                sizes[c[7]] = int(c[2])
        for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if name in sizes:
                field = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", entry).group(1))
                out[name] = dict(bytes=sizes[name], vgprs=field("vgpr_count"), scratch=field("private_segment_fixed_size"),
                                 vgpr_spills=field("vgpr_spill_count"))
    return out


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs llvm-readelf of the ROCm toolchain (no GPU)")
def test_the_16_khz_instances_are_no_larger_than_before_and_keep_their_registers():
    _native.load()
    inst = {k: v for k, v in wg_instances().items() if "ILi401ELi160ELi12E" in k}
    # the default forward's instance keeps its name (tests/test_host_logic.py, tools/refresh_design.py look it up)
    assert any(re.search(r"leaf_fft_wg_kernelILi401ELi160ELi12ELb0EEE", k) for k in inst), sorted(inst)
    streams = [k for k in inst if "ILi401ELi160ELi12ELb1E" in k]     # one STREAM instance: it chooses its loader at run time, as before
    tails = [k for k in inst if k not in streams]                    # fp32 / 16-bit / mixed fp32 / mixed PCM16 x the two tail tiles
    assert len(streams) == 1 and len(tails) == 8, sorted(inst)
    for name, r in sorted(inst.items()):
        stream = name in streams
        print(f"{name}: {r}")
        assert r["bytes"] <= PARENT_BYTES[stream], (name, r)
        assert r["vgprs"] <= MAX_VGPRS and r["vgpr_spills"] == 0, (name, r)
        assert r["scratch"] <= (STREAM_SCRATCH if stream else 0), (name, r)


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs llvm-readelf of the ROCm toolchain (no GPU)")
def test_every_kernel_is_compiled_in_exactly_one_translation_unit():
    """A csrc header is either safe in every unit (templates, device functions, sizes) or leaf_kernels.hip's alone (the plain
    kernels: leaf_kernels_*.hpp, leaf_staged.hpp, leaf_stage_backward.hpp).  What that buys, counted in the BUILT library: over all
    gfx950 code objects (one per translation unit), every kernel -- a FUNC symbol with a `.kd` kernel descriptor beside it -- occurs
    in exactly one."""
    _native.load()
    seen = {}
    blobs = list(device_code_objects(_native.LIB_PATH))
    for unit, blob in enumerate(blobs):
        with tempfile.NamedTemporaryFile(suffix=".elf") as fh:
            fh.write(blob)
            fh.flush()
            syms = subprocess.run([READELF, "-sW", fh.name], capture_output=True, text=True, check=True).stdout
        rows = [line.split() for line in syms.splitlines()]
        rows = [c for c in rows if len(c) >= 8]
        descriptors = {c[7][:-3] for c in rows if c[3] == "OBJECT" and c[7].endswith(".kd")}
        for name in {c[7] for c in rows if c[3] == "FUNC"} & descriptors:
            seen.setdefault(name, []).append(unit)
    assert len(blobs) == len(_native._translation_units(os.path.dirname(_native.SRC_PATH))) and len(seen) > 100, (len(blobs), len(seen))
    twice = {name: units for name, units in seen.items() if len(units) != 1}
    assert not twice, f"kernels compiled in more than one translation unit: {twice}"


def getters():
    """The instance getters of csrc/leaf_inst.hpp by their plain names (C++ linkage: looked up in the dynamic symbol table)."""
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = ctypes.CDLL(_native.LIB_PATH)
    found = {}
    for line in out.splitlines():
        sym = line.split()[-1]
        m = re.fullmatch(r"_Z(\d+)(leaf_inst_fft_wg(?:_streamfin|_x16|_mix16|_mix)?)([ib]+)", sym)
        if m and int(m.group(1)) == len(m.group(2)):
            fn = getattr(lib, sym)
            fn.restype = ctypes.c_void_p
            fn.argtypes = [ctypes.c_bool if ch == "b" else ctypes.c_int for ch in m.group(3)]
            found[m.group(2)] = fn
    return found


def test_every_combination_served_before_has_an_instance_and_nothing_else_has():
    g = getters()
    assert set(g) == {"leaf_inst_fft_wg", "leaf_inst_fft_wg_streamfin", "leaf_inst_fft_wg_x16", "leaf_inst_fft_wg_mix",
                      "leaf_inst_fft_wg_mix16"}, sorted(g)
    handles = []
    for sk, _, nw in GEOMETRIES:
        handles += [g["leaf_inst_fft_wg"](sk, nw, 128), g["leaf_inst_fft_wg"](sk, nw, 64), g["leaf_inst_fft_wg_streamfin"](sk, nw)]
        for tailc in (128, 64):                              # 16-bit (bfloat16 / PCM16), mixed fp32 and mixed PCM16 waveforms
            handles += [g[name](sk, nw, tailc) for name in OTHER_KINDS]
    assert all(handles) and len(set(handles)) == len(handles) == 9 * len(GEOMETRIES)
    # what had no instance has none: other windows, other workgroup sizes (the A/B sizes exist in tools builds only), other tails
    for sk, nw in ((401, 10), (401, 16), (801, 12), (801, 14), (201, 16), (552, 12), (0, 12), (401, 0)):
        assert not g["leaf_inst_fft_wg"](sk, nw, 128) and not g["leaf_inst_fft_wg"](sk, nw, 64)
        assert not g["leaf_inst_fft_wg_streamfin"](sk, nw)
        for tailc in (128, 64):
            assert not any(g[name](sk, nw, tailc) for name in OTHER_KINDS)
    assert not g["leaf_inst_fft_wg"](401, 12, 0) and not g["leaf_inst_fft_wg"](401, 12, 32)
    assert not any(g[name](401, 12, tailc) for name in OTHER_KINDS for tailc in (0, 32))


def test_the_c_abi_answers_as_before():
    """Workspace queries and refusals that involve the static workgroup kernel's sample kinds: the values of the commit before."""
    lib = _native.load()
    wg, pc = _native.ALGO_FFT_WG, _native.FLAG_PCEN
    for K, hop, _ in GEOMETRIES:
        F = 80 if K == 801 else 40
        for B, T in ((2, 16000), (5, 4001), (300, 16000)):
            plain = lib.leaf_workspace_bytes(B, T, F, K, hop, wg)
            assert plain > 0
            assert lib.leaf_forward_mix_workspace_bytes(B, T, F, K, hop, wg) == plain      # the kernel mixes in its loads: no mixed copy
    host = (ctypes.c_char * 4096)()
    base = ctypes.addressof(host)
    p = ctypes.c_void_p(base + (-base) % 64)
    mix = lambda flags: lib.leaf_forward_mix_f32(p, p, p, 2, 2400, p, p, p, p, p, p, p, 40, 401, 160, flags, wg, p, p, 0, None)
    assert mix(pc | _native.FLAG_IO_BF16) == -8              # bfloat16 is not mixed
    assert mix(pc) == -3 and mix(pc | _native.FLAG_X_PCM16) == -3   # accepted: the 0-byte workspace is what is refused next
    fwd = lambda flags, algo: lib.leaf_forward_f32(p, 2, 2400, p, p, p, p, p, p, p, 40, 401, 160, flags, algo, p, p, 0, None)
    for flags in (pc, pc | _native.FLAG_IO_BF16, pc | _native.FLAG_X_PCM16):
        assert fwd(flags, wg) == -3 and fwd(flags, wg | _native.ALGO_STREAM_FINALIZE) == -3
