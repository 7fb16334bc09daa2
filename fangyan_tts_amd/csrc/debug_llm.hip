// Test hooks of the speech-token LM's decode products and cache attention (tests/test_llm_kernels_gpu.py): each one enters a
// production launcher (gemv_bf16w, gemv32, gv32_split_rows, llm_attention, llm_attention_step) with arguments the tests build
// themselves, one operation at a time.  Not declared in include/fy_cosy3.h; the tests set the argtypes.
#include "attn.h"
#include "gemm.h"
#include "gemv32.h"
#include "runtime.h"

namespace {
// the split-K workspace of the hooks: kept between calls so that a test can run a product twice on the SAME partial sums and
// arrival counters.  ws: 0 = the product runs without one, 1 = allocated (if need be) and zeroed first, 2 = as the last call left it
struct DebugWs {
    float* partial = nullptr;
    int* counters = nullptr;
    size_t floats = 0, ints = 0;
};
int debug_ws(DebugWs& w, size_t floats, size_t ints, int ws, hipStream_t st) {
    FY_CHECK(ws == 1 || (ws == 2 && w.partial && floats <= w.floats && ints <= w.ints), FY_ERR_ARG, "debug workspace: nothing to reuse");
    if (floats > w.floats || ints > w.ints) {
        HIP_TRY(hipStreamSynchronize(st));
        if (w.partial) HIP_TRY(hipFree(w.partial));
        if (w.counters) HIP_TRY(hipFree(w.counters));
        w = DebugWs();
        HIP_TRY(hipMalloc(&w.partial, floats * sizeof(float)));
        HIP_TRY(hipMalloc(&w.counters, ints * sizeof(int)));
        w.floats = floats; w.ints = ints;
    }
    if (ws == 1) {
        HIP_TRY(hipMemsetAsync(w.partial, 0, w.floats * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(w.counters, 0, w.ints * sizeof(int), st));
    }
    return FY_OK;
}
// test-only state: one caller at a time (no lock), and the two allocations live until the process ends (never freed, by design)
DebugWs g_ws8, g_ws32;
}  // namespace

// y = W x through gemv_pack + gemv_bf16w.  W: fp32 [N][K]; packed: scratch of ceil(N/32) (K/16) 512 bf16; x (fp32 [R][ldx], the
// LDS-staged form) or x_split (bf16 [ceil(R/8)][24][ldx], the direct form); mode: GV_*; ws: see DebugWs (it takes effect for
// K >= 2048 only, as in production).  counters_out (device, ceil(R/8) ceil(N/32) ints, with ws != 0): the arrival counters after the call.
extern "C" int fy_debug_gemv(const float* W, void* packed, const float* x, const void* x_split, int32_t ldx, int32_t R, int32_t N, int32_t K, const float* bias,
                             const float* norm_w, float eps, int32_t mode, float* y, void* y_split, int32_t ldy, int32_t ws, int32_t* counters_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    FY_CHECK(W && packed && R >= 1 && N >= 1 && K >= 16 && ws >= 0 && ws <= 2, FY_ERR_ARG, "fy_debug_gemv: bad arguments");
    FY_TRY(gemv_pack(W, (bf16_t*)packed, N, K, st));
    GemvArgs a;
    a.W = (const bf16_t*)packed; a.x = x; a.x_split = (const bf16_t*)x_split; a.ldx = ldx; a.R = R; a.N = N; a.K = K;
    a.bias = bias; a.norm_w = norm_w; a.eps = eps; a.mode = mode; a.y = y; a.y_split = (bf16_t*)y_split; a.ldy = ldy;
    const size_t pf = gemv_partial_floats(R, N, K), ci = gemv_counter_ints(R, N, K);
    const bool use_ws = ws != 0 && pf != 0;
    if (use_ws) {
        FY_TRY(debug_ws(g_ws8, pf, ci, ws, st));
        a.partial = g_ws8.partial; a.counters = g_ws8.counters;
    }
    FY_TRY(gemv_bf16w(a, st));
    if (use_ws && counters_out) HIP_TRY(hipMemcpyAsync(counters_out, g_ws8.counters, ci * sizeof(int), hipMemcpyDeviceToDevice, st));
    return FY_OK;
}

// the operand image of gv32_split_rows on its own: x fp32 [R][ldx] -> img (gv32_image_elems(R, K) bf16) of ln * x, ssq (optional)
extern "C" int fy_debug_gv32_split_rows(const float* x, int32_t ldx, int32_t R, int32_t K, const float* ln, void* img, float* ssq, void* stream) {
    return gv32_split_rows(x, ldx, R, K, ln, (bf16_t*)img, ssq, (hipStream_t)stream);
}

// gemv_pack of W (and of W_lo, both fp32 [N][K]; packed: scratch of one or two planes of ceil(N/32) (K/16) 512 bf16), then gemv32 on the
// operand image img.  ssq / n_ssq / eps: the fused RMSNorm; mode: GV32_*; ws and counters_out (ceil(R/32) ceil(N/32) ints) as in fy_debug_gemv.
extern "C" int fy_debug_gemv32(const float* W, const float* W_lo, void* packed, const void* img, int32_t R, int32_t N, int32_t K, const float* ssq, int32_t n_ssq,
                               float eps, const float* bias, int32_t mode, float* y, int32_t ldy, const float* ln_next, void* img_out, float* ssq_out, int32_t ws,
                               int32_t* counters_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    FY_CHECK(W && packed && R >= 1 && N >= 1 && K >= 16 && ws >= 0 && ws <= 2, FY_ERR_ARG, "fy_debug_gemv32: bad arguments");
    bf16_t* p0 = (bf16_t*)packed;
    FY_TRY(gemv_pack(W, p0, N, K, st));
    Gv32Args a;
    a.W = p0;
    if (W_lo) {
        bf16_t* p1 = p0 + gemv_packed_elems(N, K);
        FY_TRY(gemv_pack(W_lo, p1, N, K, st));
        a.W_lo = p1;
    }
    a.img = (const bf16_t*)img; a.R = R; a.N = N; a.K = K; a.ssq = ssq; a.n_ssq = n_ssq; a.eps = eps; a.bias = bias; a.mode = mode;
    a.y = y; a.ldy = ldy; a.ln_next = ln_next; a.img_out = (bf16_t*)img_out; a.ssq_out = ssq_out;
    const size_t pf = gv32_partial_floats(R, N, K), ci = gv32_counter_ints(R, N, K);
    const bool use_ws = ws != 0 && pf != 0;
    if (use_ws) {
        FY_TRY(debug_ws(g_ws32, pf, ci, ws, st));
        a.partial = g_ws32.partial; a.counters = g_ws32.counters;
    }
    FY_TRY(gemv32(a, st));
    if (use_ws && counters_out) HIP_TRY(hipMemcpyAsync(counters_out, g_ws32.counters, ci * sizeof(int), hipMemcpyDeviceToDevice, st));
    return FY_OK;
}

extern "C" int fy_debug_llm_attention(const float* q, int32_t q_ld, const float* Kc, const float* Vc, const int32_t* row_seq, const int32_t* row_pos, float* out,
                                      int32_t o_ld, int32_t R, int32_t Hq, int32_t Hk, int32_t max_ctx, void* stream) {
    return llm_attention(q, q_ld, Kc, Vc, row_seq, row_pos, out, o_ld, R, Hq, Hk, max_ctx, (hipStream_t)stream);
}

// form: llm_attention_step's (0 = the rule, 1 = per-head kernel, 2 = group kernel); out or img (A image of the R x Hq 64 result)
extern "C" int fy_debug_llm_attention_step(const float* qkv, float* Kc, float* Vc, const int32_t* row_seq, const int32_t* row_pos, const float* inv_freq, float* out,
                                           int32_t o_ld, int32_t R, int32_t Hq, int32_t Hk, int32_t max_ctx, void* img, int32_t form, void* stream) {
    return llm_attention_step(qkv, Kc, Vc, row_seq, row_pos, inv_freq, out, o_ld, R, Hq, Hk, max_ctx, (hipStream_t)stream, (bf16_t*)img, form);
}
