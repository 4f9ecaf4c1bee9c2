"""CPU: the workgroup-per-sequence CRF kernels (polus_amd/csrc/crf.hip, 17 <= C <= 128) compile for gfx950
without scratch, and the CRF workspace query keeps the C <= 16 layout while covering the new one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRF_SRC = os.path.join(ROOT, "polus_amd", "csrc", "crf.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def crf_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("crf") / "crf.s")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        CRF_SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def _kernel_bodies(asm):
    """{symbol: text of its code} from the .s (function label up to its .size directive)."""
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*\.size\s+\1,", asm, flags=re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    return bodies


def test_crf_kernels_have_no_scratch(crf_asm):
    segs = dict(re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", crf_asm, flags=re.S))
    names = set(segs)
    assert any("crf_nll_wg_kernel" in n for n in names) and any("crf_viterbi_wg_kernel" in n for n in names)
    assert sum("crf_nll_wg_kernel" in n for n in names) == 6          # C_PAD {32, 64, 128} x dpot {f32, bf16}
    assert sum("crf_viterbi_wg_kernel" in n for n in names) == 3
    for name, size in segs.items():
        assert int(size) == 0, f"{name}: private segment {size} B"
    bodies = _kernel_bodies(crf_asm)
    assert names <= set(bodies), names - set(bodies)
    for name in names:
        assert not re.search(r"^\s*scratch_", bodies[name], flags=re.M), f"{name} uses scratch_ instructions"


def test_crf_workspace_bytes():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    lib = _lib.load()
    for B, S, C in [(4, 16, 3), (64, 256, 16), (1, 1, 1), (7, 50, 9)]:
        assert lib.polus_crf_workspace_bytes(B, S, C) == (B * S * C + B + B * C * C) * 4 + 64
    for B, S, C in [(5, 40, 17), (4, 64, 32), (3, 96, 33), (3, 96, 64), (8, 33, 100), (64, 256, 128), (1, 1, 65)]:
        cp = 32 if C <= 32 else (64 if C <= 64 else 128)
        # scaled alpha [B,S,C_PAD] (Viterbi: uint8 back-pointers), log scales [B,S], nll [B], dtrans slabs [B,C,C]
        need = (B * S * cp + B * S + B + B * C * C) * 4
        assert lib.polus_crf_workspace_bytes(B, S, C) >= need
        assert lib.polus_crf_workspace_bytes(B, S, C) >= B * S * cp       # back-pointers


def test_crf_rejects_more_than_128_tags_on_the_host():
    import ctypes
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    rc = lib.polus_crf_nll(0, p, p, None, p, None, p, p, p, 0, 2, 4, 129, p, 1 << 30, None)
    assert rc != 0 and b"128" in lib.polus_last_error()
    rc = lib.polus_crf_viterbi(p, None, p, p, 2, 4, 129, p, 1 << 30, None)
    assert rc != 0 and b"128" in lib.polus_last_error()
