"""The gated-residual DiT products (out-projection, ff2) at the benchmark's row count and at ragged ones: every tiling the dispatch can
take - the 128x128 LDS-DMA ring, gemm64_k's 256x128 tiles of sixteen waves, the automatic choice - gives the same bits, with and without
the folded LayerNorm's producer outputs (bf16 of the new residual and the per-64-column row sums)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
vp, i32 = C.c_void_p, C.c_int32


def _lib():
    from fangyan_tts_amd import _lib as lib_mod
    L = lib_mod.lib()
    L.fy_debug_gemm_resid.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    return lib_mod, L


@pytest.mark.parametrize("M,K,fold", [(6400, 1024, False), (6400, 2048, True), (5200, 1024, True), (1300, 2048, False)])
def test_gated_residual_tilings_give_the_same_bits(M, K, fold):
    lib_mod, L = _lib()
    N = 1024
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    gate = (0.25 + torch.rand(N, generator=g)).to(DEV)
    resid0 = torch.randn(M, N, generator=g).to(DEV)
    outs = {}
    for tile in (0, 2003, 6412):       # automatic; the 128x128 ring (16x16x32); gemm64_k 256x128, 16 waves
        resid = resid0.clone()
        h = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) if fold else None
        slots = torch.zeros(M, N // 64, 2, dtype=torch.float32, device=DEV) if fold else None
        lib_mod.check(L.fy_debug_gemm_resid(A.data_ptr(), W.data_ptr(), M, N, K, bias.data_ptr(), gate.data_ptr(), resid.data_ptr(),
                                            h.data_ptr() if fold else None, slots.data_ptr() if fold else None, tile, None))
        torch.cuda.synchronize()
        outs[tile] = (resid, h, slots)
    r0, h0, s0 = outs[0]
    for tile, (r, h, s) in outs.items():
        assert torch.equal(r.view(torch.int32), r0.view(torch.int32)), tile
        if fold:
            assert torch.equal(h.view(torch.int16), h0.view(torch.int16)), tile
            assert torch.equal(s.view(torch.int32), s0.view(torch.int32)), tile
    ref = resid0.double() + gate.double() * (A.double() @ W.double().t() + bias.double())
    assert (r0.double() - ref).abs().max().item() < 1e-3 * max(1.0, ref.abs().max().item())
    if fold:
        assert torch.equal(h0, r0.to(torch.bfloat16))
        s_ref = r0.double().view(M, N // 64, 64)
        assert torch.allclose(s0[..., 0].double(), s_ref.sum(-1), rtol=1e-4, atol=1e-3)
        assert torch.allclose(s0[..., 1].double(), (s_ref * s_ref).sum(-1), rtol=1e-4, atol=1e-2)
