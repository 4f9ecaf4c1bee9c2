"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/polus_hip.h declares (no compute call is made without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "polus_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(polus_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_header_and_binding_agree():
    from polus_amd import _lib
    assert declared_symbols() == sorted(_lib.SIGNATURES)


def test_library_exports_every_declared_symbol(lib):
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert lib.polus_abi_version() == 1


def test_workspace_queries_are_host_only(lib):
    assert lib.polus_gemm_workspace_bytes(768, 768, 1) == 0
    assert lib.polus_gemm_workspace_bytes(768, 768, 4) == 4 * 768 * 768 * 4
    assert lib.polus_attention_bwd_workspace_bytes(2, 128, 12) == 2 * 128 * 12 * 4
    # delta plus, for S = 512 .. 2048 in whole 256-key blocks, S / 256 f32 dQ slabs of [B S, H]: at the edges of that range
    attn_ws = {(2, 512, 12): 6340608, (1, 768, 1): 592896, (1, 2048, 1): 4202496, (1, 256, 1): 1024, (1, 2304, 1): 9216,
               (1, 1088, 1): 4352}
    for shape, nbytes in attn_ws.items():
        assert lib.polus_attention_bwd_workspace_bytes(*shape) == nbytes, shape
    # 512 block partials (POLUS_LN_BWD_BLOCKS default: every workgroup resident at once) + room for
    # ceil(512 / 128) second-stage group partials, [3H] f32 each
    assert lib.polus_layernorm_bwd_workspace_bytes(16384, 768) == (512 + 4) * 3 * 768 * 4
    assert lib.polus_crf_workspace_bytes(4, 16, 3) >= (4 * 16 * 3 + 4 + 4 * 9) * 4
    assert lib.polus_sqnorm_workspace_bytes(10 ** 8) == 1024 * 4
    # without a device the CU count falls back to the MI355X's 256
    f = lib.polus_gemm_auto_split
    assert (f(16384, 768, 3072), f(2048, 768, 3072), f(1024, 1024, 4096)) == (1, 4, 5)
    # the grouped dW plan: the four weight gradients of a BERT-base layer at 16384 tokens, slices chosen by the library
    from polus_amd import _lib, ops
    shapes = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    arr = (_lib.DwProblem * 4)(*[_lib.DwProblem(None, no, None, ni, None, ni, None, no, ni) for no, ni in shapes])
    assert lib.polus_dense_bwd_params_grouped_workspace_bytes(4, arr, 16384, 0) == 56678656
    try:
        ops.set_env("POLUS_DW_STREAMK", 1)
        assert lib.polus_dense_bwd_params_grouped_workspace_bytes(4, arr, 16384, 0) == 113357056
    finally:
        ops.set_env("POLUS_DW_STREAMK")
    # the attention workspace is an upper bound over every route: no switch moves it
    try:
        ops.set_env("POLUS_ATTN_FUSED", 0)
        assert lib.polus_attention_bwd_workspace_bytes(2, 512, 12) == 6340608
    finally:
        ops.set_env("POLUS_ATTN_FUSED")


def test_argument_validation_happens_on_the_host(lib):
    # bad shapes are rejected before any launch, with a message
    rc = lib.polus_gemm(0, 0, 0, 0, None, 8, None, 8, None, 8, 8, 8, 8, 1.0, None, None, 0, None, 0, 0, 0, 1, None, 0, None)
    assert rc != 0 and b"null operand" in lib.polus_last_error()
    rc = lib.polus_attention_fwd(0, ctypes.c_void_p(16), None, ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 8, 2, 32, 0.0, 0, None)
    assert rc != 0 and b"head_dim" in lib.polus_last_error()
    rc = lib.polus_gemm_dropout(1, 0, 0, 1, ctypes.c_void_p(16), 8, ctypes.c_void_p(16), 8, ctypes.c_void_p(16), 8, 8, 8, 8, 1.0,
                                None, None, 0, None, 0, 0, 0, 1, None, 0, 1.5, 7, None)
    assert rc != 0 and b"0 <= p < 1" in lib.polus_last_error()
    # the embedding checks its dropout arguments as polus_layernorm_bwd does: p in [0, 1) and, with dropout on, an element
    # index row * H + col that fits 32 bits (B S H = 2^32 here)
    p = ctypes.c_void_p(16)
    emb_fwd = lambda B, S, H, drop_p: lib.polus_embed_ln_fwd(0, p, p, p, p, p, p, p, p, p, p, B, S, H, 10, S, 2, 1e-12, drop_p, 7, None)
    emb_bwd = lambda B, S, H, drop_p: lib.polus_embed_ln_bwd(0, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 0, 0, B, S, H, 10, S, 2,
                                                             drop_p, 7, p, 1 << 40, None)
    for call in (emb_fwd, emb_bwd):
        for args in ((2, 8, 64, 1.0), (2, 8, 64, -0.1), (65536, 64, 1024, 0.1)):
            assert call(*args) != 0 and b"drop_p" in lib.polus_last_error(), (call, args)
    rc = lib.polus_layernorm_bwd(0, p, p, p, p, p, p, p, p, None, 0, 65536 * 64, 1024, p, 0.1, 7, p, 1 << 40, None)
    assert rc != 0 and b"bad dropout arguments" in lib.polus_last_error()


def test_no_cpu_fallback():
    import torch
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    a = torch.zeros(8, 8)
    with pytest.raises(PolusHipError):
        ops.gemm(a, a, torch.zeros(8, 8))
    if not torch.cuda.is_available():
        from polus_amd.tensor import device
        with pytest.raises(RuntimeError):
            device()


def test_product_never_imports_the_oracle():
    for dp, _, files in os.walk(os.path.join(ROOT, "polus_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)
