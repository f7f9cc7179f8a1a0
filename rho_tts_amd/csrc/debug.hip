// Kernel-level test hooks of the C ABI (include/rho_tts_amd.h, "kernel-level test hooks").
#include <algorithm>
#include <vector>

#include "kernels.h"
#include "voice_plan.h"

namespace {
__global__ void k_touch(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = p[i] * 1.0001f + 1.0f;
}
template <int MODE>
__global__ void k_bench_barrier(unsigned* bar, int n, float* buf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (i + blockDim.x) % (gridDim.x * blockDim.x);     // the next workgroup's element
    float acc = buf[i];
    for (int e = 1; e <= n; ++e) {
        if (MODE == 2) st_agent(buf + i, acc + 1.0f); else buf[i] = acc + 1.0f;      // something to publish ...
        if (!grid_barrier<MODE>(bar, gridDim.x, (unsigned)e, 1u << 20)) return;
        acc = MODE == 2 ? ld_agent(buf + j) : buf[j];                                 // ... and to fetch
        if (acc != (float)e && i == 0) bar[2] = 1u;                                   // stale read detector
    }
    buf[i] = acc;
}
// Pair hand-off ping-pong (rt_bench_grid_barrier modes 3 / 4): workgroups b and b ^ P (P = 1: neighbours in launch order, i.e. two
// XCDs; P = 8: the same XCD) pass 2 KB and a flag back and forth, n times - what ONE workgroup-to-workgroup hand-off costs when a
// K-split pair of a decode GEMM would add its halves in a fixed order.  flags[b] counts what b has published.
template <int P>
__global__ void k_bench_pair(unsigned* flags, int n, float* buf, unsigned* bar) {
    const int b = blockIdx.x, mate = b ^ P, t = threadIdx.x;
    float* mine = buf + (size_t)b * 512;
    const float* theirs = buf + (size_t)mate * 512;
    const bool first = (b & P) == 0;
    for (int e = 1; e <= n; ++e) {
        const bool give = first == ((e & 1) == 1);          // odd rounds: the lower workgroup gives, even rounds: the upper one
        if (give) {
            if (t < 512) st_agent(mine + t, (float)e);
            __syncthreads();
            if (t == 0) __hip_atomic_store(flags + b * 32, (unsigned)e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (t == 0) {
                unsigned spins = 0;
                while (__hip_atomic_load(flags + mate * 32, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)e)
                    if (++spins > (1u << 22)) { bar[1] = 1u; break; }
            }
            __syncthreads();
            if (bar[1]) return;                              // (spin bound hit somewhere: everybody leaves)
            if (t < 512 && ld_agent(theirs + t) != (float)e) bar[2] = 1u;
        }
    }
}
__global__ void k_iota64(int64_t* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

// row-major <-> fragment-tiled (common.h tile_off) converters for the column-GEMM hook; ld = the tiled buffer's width, K rounded
// up to whole 32-column k-tiles (a width that is none would fold a row block's last half tile onto the next row block's first)
template <typename T>
__global__ void k_tile_rows(const T* __restrict__ src, int M, int K, int row_off, T* __restrict__ dst, int ld) {
    const int64_t n = (int64_t)M * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / K), k = (int)(i % K);
        dst[tile_off(row_off + m, k, ld)] = src[i];
    }
}
template <typename T>
__global__ void k_untile_rows(const T* __restrict__ src, int M, int K, int row_off, T* __restrict__ dst, int ld) {
    const int64_t n = (int64_t)M * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / K), k = (int)(i % K);
        dst[i] = src[tile_off(row_off + m, k, ld)];
    }
}
}  // namespace

// The launch-plan switches: defined here, from the table in knobs.h, next to the one function that writes them.
#define RT_KNOB_DEFINE(base, name, def, lo, hi, doc) rt_knob name{def};
RT_KNOBS(RT_KNOB_DEFINE)
RT_KNOB_ARG(RT_KNOB_DEFINE)
#undef RT_KNOB_DEFINE
std::atomic<int> g_tune_epoch{0};
namespace {
struct KnobRow { int base, lo, hi; rt_knob* knob; };
#define RT_KNOB_ROW(base, name, def, lo, hi, doc) {base, lo, hi, &name},
const KnobRow kKnobs[] = {RT_KNOBS(RT_KNOB_ROW)};
const KnobRow kKnobArg[] = {RT_KNOB_ARG(RT_KNOB_ROW)};       // set by the second argument of the codes of the row with its base
#undef RT_KNOB_ROW
}  // namespace

extern "C" {

int rt_debug_gemm(rt_ctx* ctx, const void* d_a, int32_t a_is_f32, int64_t M, int32_t cin, int32_t taps, int32_t tap_stride,
                  int32_t tap_offset, int32_t rows_out, int32_t rows_in, const void* d_w_bf16, int32_t N, const float* d_bias,
                  int32_t act, float* d_out, int32_t mode, int32_t split_k) {
    if (!ctx || !d_a || !d_w_bf16 || !d_out || M < 1 || N < 1 || cin < 8 || taps < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int K = cin * taps;
    bf16_t* packed = nullptr;
    float* slabs = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&packed, packed_bytes(N, K)));
    PackedW pw;
    int rc = launch_pack_weight(ctx, (const bf16_t*)d_w_bf16, N, K, packed, &pw);
    if (!rc) {
        if (mode == 2) {             // the prompt-prefill kernel (k_gemm_mid): plain bf16 A, 65..1024 rows, K a multiple of 64
            if (a_is_f32 || taps != 1 || !gemm_mid_ok((int)M, pw)) rc = rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm: mid mode needs a plain bf16 A, 65..1024 rows, K %% 64 == 0");
            else {
                if (hipMalloc((void**)&slabs, (size_t)M * N * 4) != hipSuccess) rc = RT_ERR_OOM;
                if (!rc) rc = launch_gemm_mid(ctx, (const bf16_t*)d_a, (int)M, pw, slabs, N);
                if (!rc) rc = launch_reduce_slabs(ctx, slabs, 1, M, N, d_bias, act, d_out, nullptr);
            }
        } else if (mode == 1) {
            if (a_is_f32 || taps != 1) rc = rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm: skinny mode needs a plain bf16 A");
            else {
                if (split_k < 1) split_k = skinny_pick_split((int)M, N, K, ctx->n_cu);
                if (hipMalloc((void**)&slabs, (size_t)split_k * M * N * 4) != hipSuccess) rc = RT_ERR_OOM;
                if (!rc) rc = launch_gemm_skinny(ctx, (const bf16_t*)d_a, (int)M, pw, slabs, N, split_k);
                if (!rc) rc = launch_reduce_slabs(ctx, slabs, split_k, M, N, d_bias, act, d_out, nullptr);
            }
        } else {
            GemmA a; a.ptr = d_a; a.is_f32 = a_is_f32 == 1 || a_is_f32 == 2; a.split = a_is_f32 >= 2; a.M = M; a.Cin = cin; a.taps = taps; a.tap_stride = tap_stride; a.tap_offset = tap_offset;
            a.rows_out = rows_out; a.rows_in = rows_in;
            if (a_is_f32 == 3) {     // operand planes: the bf16 hi plane, then the bf16 lo plane, each [input rows][cin]
                const int64_t in_rows = rows_out > 0 ? (M / rows_out) * rows_in : M;
                a.ptr_lo = (const bf16_t*)d_a + in_rows * cin;
            }
            GemmEpi e; e.ldc = N;
            if (split_k <= 1) {
                e.bias = d_bias; e.act = act; e.out_f32 = d_out; e.split_k = 1;
                rc = launch_gemm(ctx, a, pw, e);
            } else {
                if (hipMalloc((void**)&slabs, (size_t)split_k * M * N * 4) != hipSuccess) rc = RT_ERR_OOM;
                e.out_f32 = slabs; e.split_k = split_k;
                if (!rc) rc = launch_gemm(ctx, a, pw, e);
                if (!rc) rc = launch_reduce_slabs(ctx, slabs, split_k, M, N, d_bias, act, d_out, nullptr);
            }
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    if (packed) (void)hipFree(packed);
    if (slabs) (void)hipFree(slabs);
    return rc;
}

int rt_debug_attention(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, const int32_t* d_row_slot,
                       const int32_t* d_row_pos, int32_t window, const void* d_k, const void* d_v, int32_t slots, int32_t max_pos,
                       void* d_out_bf16) {
    if (!ctx || !d_q || !d_k || !d_v || !d_out_bf16) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention: null argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    KvCache kv;
    kv.k = (bf16_t*)d_k; kv.v = (bf16_t*)d_v; kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    int rc = launch_attention(ctx, d_q, M, heads, kv_heads, head_dim, d_row_slot, d_row_pos, 0, window, kv, 0, (bf16_t*)d_out_bf16);
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

// hi + lo plane caches with a float32 output, launched as stack_forward launches the codec / encoder stacks' attention
int rt_debug_attention_planes(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, const int32_t* d_row_slot,
                              const int32_t* d_row_pos, int32_t window, const void* d_k_hi, const void* d_k_lo, const void* d_v_hi, const void* d_v_lo,
                              int32_t slots, int32_t max_pos, float* d_out_f32) {
    if (!ctx || !d_q || !d_k_hi || !d_k_lo || !d_v_hi || !d_v_lo || !d_out_f32) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_planes: null argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    KvCache kv;
    kv.k = (bf16_t*)d_k_hi; kv.v = (bf16_t*)d_v_hi; kv.k_lo = (bf16_t*)d_k_lo; kv.v_lo = (bf16_t*)d_v_lo;
    kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    int rc = launch_attention(ctx, d_q, M, heads, kv_heads, head_dim, d_row_slot, d_row_pos, 0, window, kv, 0, nullptr, nullptr, 0, d_out_f32);
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

// The column-owner decode GEMM (k_gemm_col) on its own, launched exactly as model_stack.hip's col_gemm launches it (row blocks of
// 128 / 64 / 32, the production sub-tile split unless one is forced).  Row-major operands at the ABI; the hook tiles / un-tiles.
int rt_debug_gemm_col(rt_ctx* ctx, const void* d_a_bf16, int32_t M, int32_t K, const void* d_w_bf16, int32_t N, int32_t epi, int32_t split,
                      int32_t row_off, int32_t nt, const float* d_rowsq, int32_t rowsq_n, float eps, const float* d_bias, const float* d_scale,
                      float* d_x, const float* d_next_norm_w, void* d_next_bf16, float* d_rowsq_out, void* d_act_bf16) {
    if (!ctx || !d_a_bf16 || !d_w_bf16 || M < 1 || M > 128 || K < 32 || K % 32 || N < 1 || row_off < 0 || row_off % 16)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm_col: bad argument (1 <= M <= 128, K %% 32 == 0, row_off %% 16 == 0)");
    if (epi < COL_STORE || epi > COL_SILU) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm_col: epi %d", epi);
    if ((epi != COL_SILU && !d_x) || (epi == COL_SILU && (!d_act_bf16 || N % 32)) || (epi == COL_RESID && !d_rowsq_out))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm_col: missing output for epilogue %d", epi);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int No = epi == COL_SILU ? N / 2 : N;                  // output width
    if (split <= 0) split = epi == COL_SILU ? col_split_silu(N, ctx->n_cu) : col_split_for(N, ctx->n_cu);
    const int rows = (row_off + M + 31) / 32 * 32;               // tiled buffers hold whole 32-row blocks (alloc_dec_ws)
    const int ldt = (No + 31) / 32 * 32;                         // ... of whole 32-column k-tiles (No itself in the model: every width is a multiple of 32)
    bf16_t *w16 = nullptr, *a_t = nullptr, *next_t = nullptr, *act_t = nullptr;
    float *x_t = nullptr, *rowsq_all = nullptr, *rowsq_out_all = nullptr;
    int rc = RT_OK;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : {(void*)w16, (void*)a_t, (void*)next_t, (void*)act_t, (void*)x_t, (void*)rowsq_all, (void*)rowsq_out_all}) if (p) (void)hipFree(p);
    };
#define DBG_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { cleanup(); return rt_fail(ctx, rt_hip_status(_e), "%s failed: %s", #expr, hipGetErrorString(_e)); } } while (0)
    DBG_HIP(hipMalloc((void**)&w16, packed16_bytes(N, K)));
    DBG_HIP(hipMalloc((void**)&a_t, (size_t)rows * K * 2));
    DBG_HIP(hipMemsetAsync(a_t, 0, (size_t)rows * K * 2, ctx->stream));
    PackedW pw;
    pw.N = N; pw.K = K;
    rc = launch_pack_weight16(ctx, (const bf16_t*)d_w_bf16, N, K, w16, &pw);
    const int nb = 256;
    hipLaunchKernelGGL((k_tile_rows<bf16_t>), dim3(nb), dim3(256), 0, ctx->stream, (const bf16_t*)d_a_bf16, M, K, row_off, a_t, K);
    const int n_part = (N + 15) / 16 * split;                    // RESID: rowsq partials per row
    ColArgs c;
    c.A = a_t; c.M = M; c.K = K; c.epi = epi; c.split = split; c.row_off = row_off; c.nt = nt ? 1 : 0; c.eps = eps;
    c.bias = d_bias; c.scale = d_scale; c.ldc = epi == COL_STORE ? No : ldt;
    if (d_rowsq) {                                               // rowsq rows are addressed by absolute row (row_off + m)
        DBG_HIP(hipMalloc((void**)&rowsq_all, (size_t)rows * rowsq_n * 4));
        DBG_HIP(hipMemsetAsync(rowsq_all, 0, (size_t)rows * rowsq_n * 4, ctx->stream));
        DBG_HIP(hipMemcpyAsync(rowsq_all + (size_t)row_off * rowsq_n, d_rowsq, (size_t)M * rowsq_n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        c.post_scale = 1; c.rowsq = rowsq_all; c.rowsq_n = rowsq_n;
    }
    if (epi == COL_STORE) {
        c.out = d_x - (size_t)row_off * No;                       // as col_head does: output rows are indexed from row_off
    } else if (epi == COL_RESID) {
        DBG_HIP(hipMalloc((void**)&x_t, (size_t)rows * ldt * 4));
        DBG_HIP(hipMemsetAsync(x_t, 0, (size_t)rows * ldt * 4, ctx->stream));
        hipLaunchKernelGGL((k_tile_rows<float>), dim3(nb), dim3(256), 0, ctx->stream, (const float*)d_x, M, No, row_off, x_t, ldt);
        DBG_HIP(hipMalloc((void**)&rowsq_out_all, (size_t)rows * n_part * 4));
        DBG_HIP(hipMemsetAsync(rowsq_out_all, 0, (size_t)rows * n_part * 4, ctx->stream));
        c.out = x_t; c.rowsq_out = rowsq_out_all; c.rowsq_out_n = n_part;
        if (d_next_bf16) {
            DBG_HIP(hipMalloc((void**)&next_t, (size_t)rows * ldt * 2));
            DBG_HIP(hipMemsetAsync(next_t, 0, (size_t)rows * ldt * 2, ctx->stream));
            c.next_bf16 = next_t; c.next_norm_w = d_next_norm_w;
        }
    } else {
        DBG_HIP(hipMalloc((void**)&act_t, (size_t)rows * ldt * 2));
        DBG_HIP(hipMemsetAsync(act_t, 0, (size_t)rows * ldt * 2, ctx->stream));
        c.out_bf16 = act_t;
    }
    const int blk = (M > 64 && g_col_rows128) ? 128 : (g_col_rows64 ? 64 : 32);   // (65..128 rows: what a generation that wide launches)
    for (int r0 = 0; r0 < M && !rc; r0 += blk) {                 // model_stack.hip col_gemm
        ColArgs a = c;
        a.M = std::min(blk, M - r0);
        a.row_off = row_off + r0;
        rc = launch_gemm_col(ctx, a, pw);
    }
    if (!rc && epi == COL_RESID) {
        hipLaunchKernelGGL((k_untile_rows<float>), dim3(nb), dim3(256), 0, ctx->stream, (const float*)x_t, M, No, row_off, d_x, ldt);
        if (next_t) hipLaunchKernelGGL((k_untile_rows<bf16_t>), dim3(nb), dim3(256), 0, ctx->stream, (const bf16_t*)next_t, M, No, row_off, (bf16_t*)d_next_bf16, ldt);
        DBG_HIP(hipMemcpyAsync(d_rowsq_out, rowsq_out_all + (size_t)row_off * n_part, (size_t)M * n_part * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (!rc && epi == COL_SILU)
        hipLaunchKernelGGL((k_untile_rows<bf16_t>), dim3(nb), dim3(256), 0, ctx->stream, (const bf16_t*)act_t, M, No, row_off, (bf16_t*)d_act_bf16, ldt);
    if (!rc) DBG_HIP(hipGetLastError());
#undef DBG_HIP
    cleanup();
    return rc;
}

// The decode step's fused attention (q/k-RMSNorm + RoPE + KV append + attention, shared voice-prefix slot) on its own.
int rt_debug_attention_fused(rt_ctx* ctx, const float* d_qkv, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, const float* d_q_norm_w,
                             const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin, const int32_t* d_row_slot,
                             const int32_t* d_row_pos, int32_t pos_add, void* d_k, void* d_v, int32_t slots, int32_t max_pos,
                             int32_t prefix_slot, int32_t prefix_len, void* d_out_bf16) {
    // (d_row_slot == NULL: row i uses slot i; d_row_pos == NULL: every row at pos_add - the array-free form the predictor's passes take)
    if (!ctx || !d_qkv || !d_cos || !d_sin || !d_k || !d_v || !d_out_bf16 || M < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused: null argument");
    if (prefix_slot >= slots || prefix_len < 0 || prefix_len > max_pos) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused: bad prefix");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    KvCache kv;
    kv.k = (bf16_t*)d_k; kv.v = (bf16_t*)d_v; kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    kv.prefix_slot = prefix_slot; kv.prefix_len = prefix_slot >= 0 ? prefix_len : 0;
    bf16_t* vt = nullptr;
    if (prefix_slot >= 0 && prefix_len > 0 && head_dim == 128) {      // the matrix-core path reads the prefix through fragment-tiled copies
        kv.vt_stride = (prefix_len + 31) / 32 * 4096;
        kv.prefix_slot_alloc = prefix_slot;
        RT_HIP(ctx, hipMalloc((void**)&vt, (size_t)2 * kv_heads * kv.vt_stride * 2));
        kv.kt_prefix = vt;
        kv.vt_prefix = vt + (size_t)kv_heads * kv.vt_stride;
        const int rt = launch_transpose_prefix_v(ctx, kv, prefix_len);
        if (rt) { (void)hipFree(vt); return rt; }
    }
    const int rc = launch_attention_fused(ctx, d_qkv, M, heads, kv_heads, head_dim, d_q_norm_w, d_k_norm_w, eps, d_cos, d_sin, d_row_slot, d_row_pos,
                                          pos_add, 0, kv, 0, (bf16_t*)d_out_bf16, nullptr, 0, 0);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (vt) (void)hipFree(vt);
    RT_HIP(ctx, se);
    return rc;
}

// The same launch as a multi-voice decode step takes it: the rows are cut into 4-row blocks, block b reads the prefix of voice
// h_block_voice[b], whose rows [0, h_prefix_len[v]) sit in slot slots - n_voices + v.  The tiles of every voice that takes the matrix-core
// form are built here, as the entry above builds them for its one prefix.
int rt_debug_attention_fused_voices(rt_ctx* ctx, const float* d_qkv, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, const float* d_q_norm_w,
                                    const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin, const int32_t* d_row_slot,
                                    const int32_t* d_row_pos, int32_t pos_add, void* d_k, void* d_v, int32_t slots, int32_t max_pos, int32_t n_voices,
                                    const int32_t* h_prefix_len, const int32_t* h_block_voice, void* d_out_bf16) {
    if (!ctx || !d_qkv || !d_cos || !d_sin || !d_k || !d_v || !d_out_bf16 || !d_row_slot || !d_row_pos || !h_prefix_len || !h_block_voice)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused_voices: null argument");
    if (M < 1 || M > 128 || n_voices < 1 || n_voices > 8 || slots < n_voices || heads < 1 || kv_heads < 1 || heads % kv_heads || max_pos < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused_voices: bad shape");
    const int n_blocks = (M + 3) / 4;
    for (int v = 0; v < n_voices; ++v)
        if (h_prefix_len[v] < 0 || h_prefix_len[v] > max_pos) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused_voices: bad prefix length");
    for (int b = 0; b < n_blocks; ++b)
        if (h_block_voice[b] < 0 || h_block_voice[b] >= n_voices) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_fused_voices: block %d names voice %d of %d", b, h_block_voice[b], n_voices);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    KvCache kv;
    kv.k = (bf16_t*)d_k; kv.v = (bf16_t*)d_v; kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    bf16_t* tiles = nullptr;
    void* d_tab = nullptr;
    auto cleanup = [&]() { if (tiles) (void)hipFree(tiles); if (d_tab) (void)hipFree(d_tab); };
    int longest = 0;
    for (int v = 0; v < n_voices; ++v) longest = std::max(longest, h_prefix_len[v]);
    const int64_t per_voice = (int64_t)kv_heads * ((longest + 31) / 32 * 4096);
    if (head_dim == 128 && longest > 0) {
        kv.vt_stride = (longest + 31) / 32 * 4096;
        RT_HIP(ctx, hipMalloc((void**)&tiles, (size_t)2 * n_voices * per_voice * 2));
        for (int v = 0; v < n_voices; ++v) {
            if (h_prefix_len[v] < 1) continue;
            kv.kt_prefix = tiles + (int64_t)2 * v * per_voice; kv.vt_prefix = kv.kt_prefix + per_voice; kv.prefix_slot_alloc = slots - n_voices + v;
            const int rt = launch_transpose_prefix_v(ctx, kv, h_prefix_len[v]);
            if (rt) { cleanup(); return rt; }
        }
    }
    std::vector<VoiceBlock> blocks(n_blocks);
    std::vector<int32_t> lists(n_blocks + M, -1);              // [the matrix-core launch's blocks][the vector launch's rows]
    VoiceTable vt;
    vt.rows = M; vt.n_blocks = n_blocks;
    int n_mf = 0, n_vr = 0;
    kv.kt_prefix = tiles; kv.vt_prefix = tiles;                // (what says that tiles exist; the launches read the table's pointers)
    for (int b = 0; b < n_blocks; ++b) {
        const int v = h_block_voice[b];
        const bool mf = attention_mfma_voice_ok(heads, kv_heads, head_dim, kv, h_prefix_len[v]);
        blocks[b].prefix_slot = slots - n_voices + v; blocks[b].prefix_len = h_prefix_len[v];
        blocks[b].kt = mf ? tiles + (int64_t)2 * v * per_voice : nullptr; blocks[b].vt = mf ? blocks[b].kt + per_voice : nullptr;
        if (mf) { lists[n_mf++] = b; vt.any_mfma = true; }
        else { for (int r = 4 * b; r < std::min(M, 4 * b + 4); ++r) lists[n_blocks + n_vr++] = r; vt.any_vec = true; }
    }
    const size_t tab_bytes = blocks.size() * sizeof(VoiceBlock), list_bytes = lists.size() * 4;
    hipError_t e = hipMalloc(&d_tab, tab_bytes + list_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_tab, blocks.data(), tab_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)d_tab + tab_bytes, lists.data(), list_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); RT_HIP(ctx, e); }
    vt.blocks = (const VoiceBlock*)d_tab;
    vt.mfma_blocks = (const int32_t*)((char*)d_tab + tab_bytes);
    vt.vec_rows = vt.mfma_blocks + n_blocks;
    kv.voices = &vt;
    const int rc = launch_attention_fused(ctx, d_qkv, M, heads, kv_heads, head_dim, d_q_norm_w, d_k_norm_w, eps, d_cos, d_sin, d_row_slot, d_row_pos,
                                          pos_add, 0, kv, 0, (bf16_t*)d_out_bf16, nullptr, 0, 0);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    cleanup();
    RT_HIP(ctx, se);
    return rc;
}

// The row plan of a multi-voice generation (voice_plan.h) as host arithmetic; no GPU is touched.  first != 0: the first wave of
// n_items items on at most max_rows rows - the three state arrays are outputs, the result is the run's row count.  first == 0: a
// hand-over - max_rows is the run's row count, the arrays hold its state with the freed rows set to -1 in h_row_item; the waiting
// items that find a row are placed and the result is their number.  h_revoiced (optional) receives the blocks that changed voice.
int rt_debug_voice_row_plan(const int32_t* h_voice, int32_t n_items, int32_t max_rows, int32_t first, int32_t* h_row_item, int32_t* h_block_voice,
                            int32_t* h_placed, int32_t* h_revoiced) {
    if (!h_voice || !h_row_item || !h_block_voice || !h_placed || n_items < 1 || max_rows < 1 || max_rows > 128) return -1;
    for (int i = 0; i < n_items; ++i) if (h_voice[i] < 0 || h_voice[i] >= 8) return -1;
    voice_plan::State s;
    int result = 0, revoiced = 0;
    if (first) {
        voice_plan::start(h_voice, n_items, max_rows, s, nullptr, nullptr);
        result = s.rows;
    } else {
        s.rows = max_rows;
        s.row_item.assign(h_row_item, h_row_item + max_rows);
        s.block_voice.assign(h_block_voice, h_block_voice + s.n_blocks());
        s.placed.resize(n_items);
        for (int i = 0; i < n_items; ++i) s.placed[i] = h_placed[i] != 0;
        for (int r = 0; r < max_rows; ++r) if (s.row_item[r] >= n_items) return -1;
        result = voice_plan::place(h_voice, n_items, s, nullptr, nullptr, &revoiced);
    }
    for (int r = 0; r < max_rows; ++r) h_row_item[r] = r < s.rows ? s.row_item[r] : -1;
    for (int b = 0; b < (max_rows + 3) / 4; ++b) h_block_voice[b] = b < s.n_blocks() ? s.block_voice[b] : -1;
    for (int i = 0; i < n_items; ++i) h_placed[i] = s.placed[i];
    if (h_revoiced) *h_revoiced = revoiced;
    return result;
}

// Prompt-prefill attention behind a shared prefix slot (q prepared, K / V rows already in the caches): mode 0 = the vector-unit
// kernel (k_attention), 1 = the matrix-core form the model uses for prompt rows (attention_mfma.hip, head_dim 128, 2 query heads per
// kv head, prefix of >= 64 rows)
int rt_debug_attention_prefill(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, const int32_t* d_row_slot,
                               const int32_t* d_row_pos, const void* d_k, const void* d_v, int32_t slots, int32_t max_pos, int32_t prefix_slot,
                               int32_t prefix_len, int32_t mode, void* d_out_bf16) {
    if (!ctx || !d_q || !d_row_slot || !d_row_pos || !d_k || !d_v || !d_out_bf16 || M < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_prefill: null argument");
    if (prefix_slot < 0 || prefix_slot >= slots || prefix_len < 1 || prefix_len > max_pos) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_attention_prefill: bad prefix");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    KvCache kv;
    kv.k = (bf16_t*)d_k; kv.v = (bf16_t*)d_v; kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    kv.prefix_slot = prefix_slot; kv.prefix_len = prefix_len;
    bf16_t* vt = nullptr;
    if (mode) {             // (mode 0 builds no tiles: launch_attention cannot take the matrix-core form, whatever g_prefill_attn_mfma says)
        if (head_dim != 128) return rt_fail(ctx, RT_ERR_UNSUPPORTED, "rt_debug_attention_prefill: the matrix-core form needs head_dim 128");
        kv.vt_stride = (prefix_len + 31) / 32 * 4096;
        kv.prefix_slot_alloc = prefix_slot;
        RT_HIP(ctx, hipMalloc((void**)&vt, (size_t)2 * kv_heads * kv.vt_stride * 2));
        kv.kt_prefix = vt;
        kv.vt_prefix = vt + (size_t)kv_heads * kv.vt_stride;
        const int rt = launch_transpose_prefix_v(ctx, kv, prefix_len);
        if (rt) { (void)hipFree(vt); return rt; }
        if (!attention_prefill_mfma_shape_ok(heads, kv_heads, head_dim, 0, kv)) {
            (void)hipFree(vt);
            return rt_fail(ctx, RT_ERR_UNSUPPORTED, "rt_debug_attention_prefill: shape not served by the matrix-core form");
        }
    }
    int rc;
    if (mode == 2) {        // the prefix slot's own prefill: rows = positions 0 .. M - 1 of prefix_slot, causal (tiles made by the call itself)
        kv.prefix_slot = -1; kv.prefix_len = 0;
        kv.vt_stride = std::max(kv.vt_stride, (M + 31) / 32 * 4096);
        if (vt) { (void)hipFree(vt); vt = nullptr; }
        hipError_t me = hipMalloc((void**)&vt, (size_t)2 * kv_heads * kv.vt_stride * 2);
        if (me != hipSuccess) return rt_fail(ctx, rt_hip_status(me), "rt_debug_attention_prefill: out of memory");
        kv.kt_prefix = vt;
        kv.vt_prefix = vt + (size_t)kv_heads * kv.vt_stride;
        rc = attention_block_prefix_shape_ok(M, heads, kv_heads, head_dim, 0, kv)
                 ? launch_attention_block_prefix(ctx, d_q, M, heads, kv_heads, d_row_slot, d_row_pos, kv, 0, (bf16_t*)d_out_bf16)
                 : rt_fail(ctx, RT_ERR_UNSUPPORTED, "rt_debug_attention_prefill: shape not served by the block-prefix form");
    } else if (mode) {
        rc = launch_attention_prefill_mfma(ctx, d_q, M, heads, kv_heads, d_row_slot, d_row_pos, 0, kv, 0, (bf16_t*)d_out_bf16);
    } else {
        rc = launch_attention(ctx, d_q, M, heads, kv_heads, head_dim, d_row_slot, d_row_pos, 0, 0, kv, 0, (bf16_t*)d_out_bf16);
    }
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (vt) (void)hipFree(vt);
    RT_HIP(ctx, se);
    return rc;
}

int rt_debug_sample(rt_ctx* ctx, const float* d_logits, int32_t M, int32_t V, const rt_sampling* sp, uint64_t seed, int32_t frame,
                    int32_t group, int32_t suppress_from, int32_t allow_token, uint8_t* d_seen, int32_t* d_out) {
    if (!ctx || !d_logits || !sp || !d_out || M < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_sample: null argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int64_t* items = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&items, (size_t)M * 8));
    hipLaunchKernelGGL(k_iota64, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, items, M);
    SampleArgs a{};
    a.logits = d_logits; a.n_slabs = 1; a.M = M; a.V = V;
    a.do_sample = sp->do_sample; a.temperature = sp->temperature; a.top_k = sp->top_k; a.top_p = sp->top_p; a.rep_penalty = sp->repetition_penalty;
    a.seen = d_seen; a.suppress_from = suppress_from; a.allow_token = allow_token; a.seed = seed; a.item_ids = items; a.frame = frame; a.group = group;
    a.forced = nullptr; a.out = d_out; a.out_stride = 1; a.eos_token = -1; a.eos_flag = nullptr; a.logits_copy = nullptr;
    a.frame_ptr = nullptr; a.seed_ptr = nullptr; a.stamps = nullptr;
    int rc = launch_sample(ctx, a);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(items);
    return rc;
}

// ------------------------------------------------------------------ row kernels on their own (rowops.hip through its launchers)
extern "C++" {
namespace {
// frees what a hook allocated, after the stream has drained (every exit of a hook runs it)
struct DbgBufs {
    rt_ctx* ctx;
    std::vector<void*> ptrs;
    explicit DbgBufs(rt_ctx* c) : ctx(c) {}
    ~DbgBufs() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t alloc(T** out, size_t bytes) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e == hipSuccess) ptrs.push_back(p);
        *out = (T*)p;
        return e;
    }
};
// the device array of bf16 sources from the host arrays of the ABI
int upload_srcs(rt_ctx* ctx, DbgBufs& bufs, const void* const* h_tables, const int64_t* h_row_strides, int n_src, GatherSrc** out) {
    *out = nullptr;
    if (n_src <= 0) return RT_OK;
    std::vector<GatherSrc> h((size_t)n_src);
    for (int j = 0; j < n_src; ++j) {
        if (!h_tables[j]) return rt_fail(ctx, RT_ERR_INVALID, "debug hook: source table %d is null", j);
        h[j].table = (const bf16_t*)h_tables[j];
        h[j].row_stride = h_row_strides[j];
    }
    RT_HIP(ctx, bufs.alloc(out, sizeof(GatherSrc) * (size_t)n_src));
    RT_HIP(ctx, hipMemcpy(*out, h.data(), sizeof(GatherSrc) * (size_t)n_src, hipMemcpyHostToDevice));
    return RT_OK;
}
int dbg_finish(rt_ctx* ctx, int rc) {
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    RT_HIP(ctx, se);
    return RT_OK;
}
// tiled working copies of the caller's row-major [rows][H] outputs (see the header: what the kernel leaves alone keeps its bytes)
template <typename T>
int dbg_tile_in(rt_ctx* ctx, DbgBufs& bufs, const T* rows_rm, int rows, int H, T** tiled) {
    const size_t pad = (size_t)(rows + 15) / 16 * 16;
    RT_HIP(ctx, bufs.alloc(tiled, pad * H * sizeof(T)));
    RT_HIP(ctx, hipMemsetAsync(*tiled, 0, pad * H * sizeof(T), ctx->stream));
    hipLaunchKernelGGL((k_tile_rows<T>), dim3(256), dim3(256), 0, ctx->stream, rows_rm, rows, H, 0, *tiled, H);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}
template <typename T>
int dbg_tile_out(rt_ctx* ctx, const T* tiled, int rows, int H, T* rows_rm) {
    hipLaunchKernelGGL((k_untile_rows<T>), dim3(256), dim3(256), 0, ctx->stream, tiled, rows, H, 0, rows_rm, H);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}
int dbg_read_i32(rt_ctx* ctx, const int32_t* d, int n, std::vector<int32_t>& h) {
    h.assign((size_t)n, 0);
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RT_HIP(ctx, hipMemcpy(h.data(), d, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}
}  // namespace
}  // extern "C++"

int rt_debug_add_rmsnorm(rt_ctx* ctx, float* d_x, int32_t M, int32_t H, const float* d_slabs, int32_t n_slabs, const float* d_slab_bias,
                         const float* d_scale, const float* d_w, float eps, void* d_out_bf16, float* d_out_f32) {
    if (!ctx || !d_x || M < 1 || H < 1 || n_slabs < 0 || (n_slabs > 0 && !d_slabs))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_add_rmsnorm: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_add_rmsnorm(ctx, d_x, M, H, d_slabs, n_slabs, d_slab_bias, d_scale, d_w, eps, (bf16_t*)d_out_bf16, d_out_f32));
}

int rt_debug_rowsq(rt_ctx* ctx, const float* d_x, int32_t M, int32_t H, float* d_rowsq, int32_t rowsq_n, float* d_x_out, void* d_a_out_bf16,
                   const float* d_norm_w, const int32_t* d_src_rows, const int32_t* d_dst_rows, int32_t out_rows, const float* d_g_table,
                   const int32_t* d_g_idx, int32_t g_idx_stride, int32_t g_first, const int32_t* d_g_frame_ptr, int64_t g_idx_frame_stride,
                   int32_t raw_tiled) {
    const bool tiled_out = d_x_out || d_a_out_bf16;
    if (!ctx || !d_rowsq || M < 1 || rowsq_n < 1 || out_rows < 1 || H < 4 || H % 4 || (tiled_out && H % 32) || (d_a_out_bf16 && !d_norm_w) ||
        (!d_dst_rows && out_rows < M) || (!d_x && !(d_g_table && g_first == 0)))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_rowsq: bad argument (H %% 4 == 0, H %% 32 == 0 with a tiled output, out_rows >= M without a row map)");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> h;
    if (d_src_rows) {
        RT_TRY(dbg_read_i32(ctx, d_src_rows, M, h));
        for (int32_t v : h) if (v < 0 || v >= M) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_rowsq: source row %d outside [0, %d)", v, M);
    }
    if (d_dst_rows) {
        RT_TRY(dbg_read_i32(ctx, d_dst_rows, M, h));
        for (int32_t v : h) if (v < 0 || v >= out_rows) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_rowsq: output row %d outside [0, %d)", v, out_rows);
    }
    DbgBufs bufs(ctx);
    float* x_t = d_x_out;
    bf16_t* a_t = (bf16_t*)d_a_out_bf16;
    if (!raw_tiled) {
        if (d_x_out) RT_TRY(dbg_tile_in(ctx, bufs, (const float*)d_x_out, out_rows, H, &x_t));
        if (d_a_out_bf16) RT_TRY(dbg_tile_in(ctx, bufs, (const bf16_t*)d_a_out_bf16, out_rows, H, &a_t));
    }
    RowsqGather gt;
    gt.table = d_g_table; gt.idx = d_g_idx; gt.idx_stride = g_idx_stride; gt.first = g_first; gt.frame_ptr = d_g_frame_ptr; gt.idx_frame_stride = g_idx_frame_stride;
    int rc = launch_rowsq(ctx, d_x, M, H, d_rowsq, rowsq_n, x_t, a_t, d_norm_w, d_src_rows, d_dst_rows, d_g_table ? &gt : nullptr);
    if (!rc && !raw_tiled) {
        if (d_x_out) rc = dbg_tile_out(ctx, (const float*)x_t, out_rows, H, d_x_out);
        if (!rc && d_a_out_bf16) rc = dbg_tile_out(ctx, (const bf16_t*)a_t, out_rows, H, (bf16_t*)d_a_out_bf16);
    }
    return dbg_finish(ctx, rc);
}

int rt_debug_norm_tiled_rows(rt_ctx* ctx, const float* d_x, const float* d_rowsq, int32_t rowsq_n, const float* d_w, float eps, int32_t M, int32_t H,
                             float* d_out) {
    if (!ctx || !d_x || !d_rowsq || !d_w || !d_out || M < 1 || rowsq_n < 1 || H < 32 || H % 32)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_norm_tiled_rows: bad argument (H %% 32 == 0)");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DbgBufs bufs(ctx);
    float* x_t = nullptr;
    RT_TRY(dbg_tile_in(ctx, bufs, d_x, M, H, &x_t));
    return dbg_finish(ctx, launch_norm_tiled_rows(ctx, x_t, d_rowsq, rowsq_n, d_w, eps, M, H, d_out));
}

int rt_debug_embed_rowsq(rt_ctx* ctx, const void* const* h_tables, const int64_t* h_row_strides, int32_t n_src, const float* d_f32_table,
                         const int32_t* d_idx, int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride, int32_t M, int32_t H,
                         const float* d_add_vec, float* d_rowsq, int32_t rowsq_n, float* d_x_out, void* d_a_out_bf16, const float* d_norm_w,
                         int32_t* d_frame_inc, uint32_t* d_arrive, const float* d_qkv_table, float* d_qkv_out, int32_t qkv_n, int32_t raw_tiled) {
    if (!ctx || !d_idx || M < 1 || H < 32 || H % 32 || n_src < 0 || idx_stride < 1 || (n_src > 0 && (!h_tables || !h_row_strides)) ||
        (n_src == 0 && !d_f32_table) || !d_x_out || !d_a_out_bf16 || !d_rowsq || rowsq_n < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_embed_rowsq: bad argument (H %% 32 == 0, a source, all three outputs)");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DbgBufs bufs(ctx);
    GatherSrc* srcs = nullptr;
    if (n_src <= 16) RT_TRY(upload_srcs(ctx, bufs, h_tables, h_row_strides, n_src, &srcs));     // (more: the launcher's refusal)
    float* x_t = d_x_out;
    bf16_t* a_t = (bf16_t*)d_a_out_bf16;
    if (!raw_tiled) {
        RT_TRY(dbg_tile_in(ctx, bufs, (const float*)d_x_out, M, H, &x_t));
        RT_TRY(dbg_tile_in(ctx, bufs, (const bf16_t*)d_a_out_bf16, M, H, &a_t));
    }
    int rc = launch_embed_rowsq(ctx, srcs, n_src, d_f32_table, d_idx, idx_stride, d_frame_ptr, idx_frame_stride, M, H, d_add_vec, d_rowsq, rowsq_n,
                                x_t, a_t, d_norm_w, d_frame_inc, (unsigned*)d_arrive, d_qkv_table, d_qkv_out, qkv_n);
    if (!rc && !raw_tiled) {
        rc = dbg_tile_out(ctx, (const float*)x_t, M, H, d_x_out);
        if (!rc) rc = dbg_tile_out(ctx, (const bf16_t*)a_t, M, H, (bf16_t*)d_a_out_bf16);
    }
    return dbg_finish(ctx, rc);
}

int rt_debug_sample_frame(rt_ctx* ctx, const rt_debug_sample_frame_args* p) {
    if (!ctx || !p || !p->d_logits || !p->d_item_ids || !p->d_seed || !p->d_frame || !p->d_out || p->M < 1 || p->V < 1 || p->n_slabs < 1 ||
        p->out_stride < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_sample_frame: bad argument (logits, item ids, seed, frame and out are needed; M, V, n_slabs, out_stride >= 1)");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int M = p->M, H = p->emb_H;
    // what moves an address is read back first: the frame (every frame-strided buffer), the rows' starts, forced tokens that index a table
    std::vector<int32_t> hf, h;
    RT_TRY(dbg_read_i32(ctx, p->d_frame, 1, hf));
    if (hf[0] < 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_sample_frame: frame %d", hf[0]);
    if (p->d_frame_off) {
        RT_TRY(dbg_read_i32(ctx, p->d_frame_off, M, h));
        for (int32_t v : h) if (v > hf[0]) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_sample_frame: a row starts at frame %d, after frame %d", v, hf[0]);
    }
    if (p->d_forced && p->d_emb_table) {
        RT_TRY(dbg_read_i32(ctx, p->d_forced + (int64_t)hf[0] * p->forced_fs, M, h));
        for (int32_t v : h) if (v >= p->V) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_sample_frame: forced token %d outside the embedding table", v);
    }
    DbgBufs bufs(ctx);
    float* x_t = p->d_emb_x;
    bf16_t* a_t = (bf16_t*)p->d_emb_a_bf16;
    // (a width the tiled layout cannot hold goes to the launcher as it is: the refusal is launch_sample's, and nothing is launched)
    const bool tiled = p->d_emb_table && H >= 32 && H % 32 == 0;
    if (tiled && x_t) RT_TRY(dbg_tile_in(ctx, bufs, (const float*)p->d_emb_x, M, H, &x_t));
    if (tiled && a_t) RT_TRY(dbg_tile_in(ctx, bufs, (const bf16_t*)p->d_emb_a_bf16, M, H, &a_t));
    SampleArgs a{};
    a.logits = p->d_logits; a.n_slabs = p->n_slabs; a.M = M; a.V = p->V;
    a.do_sample = p->sp.do_sample; a.temperature = p->sp.temperature; a.top_k = p->sp.top_k; a.top_p = p->sp.top_p; a.rep_penalty = p->sp.repetition_penalty;
    a.seen = p->d_seen; a.suppress_from = p->suppress_from; a.allow_token = -1;
    a.seed_ptr = p->d_seed; a.item_ids = p->d_item_ids; a.frame = 0; a.group = p->group;
    a.forced = p->d_forced; a.forced_fs = p->forced_fs;
    a.out = p->d_out; a.out_stride = p->out_stride; a.out_fs = p->out_fs;
    a.eos_token = p->eos_token; a.eos_flag = p->d_eos_flag; a.eos_fs = p->eos_fs;
    a.logits_copy = p->d_logits_copy; a.copy_fs = p->copy_fs;
    a.frame_ptr = p->d_frame; a.frame_off = p->d_frame_off; a.eos_live = p->eos_live; a.min_frames = p->min_frames;
    a.emb_table = p->d_emb_table; a.emb_H = H; a.emb_norm_w = p->d_emb_norm_w; a.emb_rowsq = p->d_emb_rowsq; a.emb_rowsq_n = p->emb_rowsq_n;
    a.emb_x_tiled = x_t; a.emb_a_tiled = a_t;
    a.emb_qkv_table = p->d_emb_qkv_table; a.emb_qkv_out = p->d_emb_qkv_out; a.emb_qkv_n = p->emb_qkv_n;
    int rc = launch_sample(ctx, a);
    if (!rc && tiled) {
        rc = dbg_tile_out(ctx, (const float*)x_t, M, H, p->d_emb_x);
        if (!rc) rc = dbg_tile_out(ctx, (const bf16_t*)a_t, M, H, (bf16_t*)p->d_emb_a_bf16);
    }
    return dbg_finish(ctx, rc);
}

int rt_debug_silu_mul(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int32_t M, int32_t I, void* d_out_bf16, float* d_out_f32) {
    if (!ctx || !d_slabs || n_slabs < 1 || M < 1 || I < 1 || (!d_out_bf16 && !d_out_f32)) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_silu_mul: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_silu_mul(ctx, d_slabs, n_slabs, M, I, (bf16_t*)d_out_bf16, d_out_f32));
}

int rt_debug_reduce_slabs(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int64_t M, int32_t N, const float* d_bias, int32_t act, float* d_out_f32,
                          void* d_out_bf16) {
    if (!ctx || !d_slabs || n_slabs < 1 || M < 1 || N < 1 || act < ACT_NONE || act > ACT_GELU || (!d_out_bf16 && !d_out_f32))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_reduce_slabs: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_reduce_slabs(ctx, d_slabs, n_slabs, M, N, d_bias, act, d_out_f32, (bf16_t*)d_out_bf16));
}

int rt_debug_f32_to_bf16(rt_ctx* ctx, const float* d_x, int64_t n, void* d_out_bf16) {
    if (!ctx || !d_x || !d_out_bf16 || n < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_f32_to_bf16: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_f32_to_bf16(ctx, d_x, n, (bf16_t*)d_out_bf16));
}

int rt_debug_qkv_post(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                      const float* d_q_norm_w, const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin, const int32_t* d_row_slot,
                      const int32_t* d_row_pos, int32_t pos_add, float* d_q_out, void* d_k, void* d_v, void* d_k_lo, void* d_v_lo, int32_t slots,
                      int32_t max_pos, const int32_t* d_frame_ptr) {
    if (!ctx || !d_slabs || n_slabs < 1 || M < 1 || heads < 1 || kv_heads < 1 || head_dim < 1 || !d_row_slot || !d_row_pos || !d_q_out || !d_k || !d_v ||
        !d_k_lo != !d_v_lo || !d_cos != !d_sin || slots < 1 || max_pos < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_qkv_post: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> hs, hp, hf(1, 0);
    RT_TRY(dbg_read_i32(ctx, d_row_slot, M, hs));
    RT_TRY(dbg_read_i32(ctx, d_row_pos, M, hp));
    if (d_frame_ptr) RT_TRY(dbg_read_i32(ctx, d_frame_ptr, 1, hf));
    for (int r = 0; r < M; ++r) {
        const int64_t pos = (int64_t)hp[r] + pos_add + hf[0];
        if (hs[r] < 0 || hs[r] >= slots || pos < 0 || pos >= max_pos)
            return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_qkv_post: row %d at slot %d position %lld is outside the caches", r, hs[r], (long long)pos);
    }
    KvCache kv;
    kv.k = (bf16_t*)d_k; kv.v = (bf16_t*)d_v; kv.k_lo = (bf16_t*)d_k_lo; kv.v_lo = (bf16_t*)d_v_lo;
    kv.layers = 1; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    return dbg_finish(ctx, launch_qkv_post(ctx, d_slabs, n_slabs, M, heads, kv_heads, head_dim, d_q_norm_w, d_k_norm_w, eps, d_cos, d_sin, d_row_slot,
                                           d_row_pos, pos_add, d_q_out, kv, 0, d_frame_ptr));
}

int rt_debug_gather_sum(rt_ctx* ctx, const void* const* h_tables, const int64_t* h_row_strides, int32_t n_src, const int32_t* d_idx, int32_t M, int32_t H,
                        const float* d_add_vec, const float* d_add_rows, const int32_t* d_add_row_idx, float* d_out_f32, void* d_out_bf16,
                        int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride) {
    if (!ctx || M < 1 || H < 1 || n_src < 0 || n_src > 64 || idx_stride < 0 || (n_src > 0 && (!h_tables || !h_row_strides || !d_idx)) ||
        (!d_out_f32 && !d_out_bf16))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gather_sum: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DbgBufs bufs(ctx);
    GatherSrc* srcs = nullptr;
    RT_TRY(upload_srcs(ctx, bufs, h_tables, h_row_strides, n_src, &srcs));
    return dbg_finish(ctx, launch_gather_sum(ctx, srcs, n_src, d_idx, M, H, d_add_vec, d_add_rows, d_add_row_idx, d_out_f32, (bf16_t*)d_out_bf16,
                                             idx_stride, d_frame_ptr, idx_frame_stride));
}

int rt_debug_gather_f32(rt_ctx* ctx, const float* d_table, int32_t H, const int32_t* d_idx, int32_t M, float* d_out_f32, void* d_out_bf16,
                        int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride) {
    if (!ctx || !d_table || !d_idx || M < 1 || H < 1 || idx_stride < 1 || (!d_out_f32 && !d_out_bf16))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gather_f32: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_gather_f32(ctx, d_table, H, d_idx, M, d_out_f32, (bf16_t*)d_out_bf16, idx_stride, d_frame_ptr, idx_frame_stride));
}

int rt_debug_dwconv_ln(rt_ctx* ctx, const float* d_x, int32_t B, int32_t T, int32_t C, const float* d_w, const float* d_b, const float* d_ln_w,
                       const float* d_ln_b, float eps, float* d_out) {
    if (!ctx || !d_x || !d_w || !d_b || !d_ln_w || !d_ln_b || !d_out || B < 1 || T < 1 || C < 1 || (size_t)C * 4 > 64 * 1024)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_dwconv_ln: bad argument (a row of C floats must fit 64 KiB of LDS)");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_dwconv_ln(ctx, d_x, B, T, C, d_w, d_b, d_ln_w, d_ln_b, eps, d_out));
}

int rt_debug_code_embed_mean(rt_ctx* ctx, const void* d_table_bf16, int32_t codebook, int32_t Q, int32_t H, const int32_t* d_codes, int64_t rows,
                             float* d_out) {
    if (!ctx || !d_table_bf16 || !d_codes || !d_out || codebook < 1 || Q < 1 || H < 1 || rows < 1 || rows > 0x7fffffff)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_code_embed_mean: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_code_embed_mean(ctx, (const bf16_t*)d_table_bf16, codebook, Q, H, d_codes, rows, d_out));
}

int rt_debug_final_conv(rt_ctx* ctx, const void* d_hi, const void* d_lo, int32_t B, int32_t T, int32_t C, const float* d_w, const float* d_bias,
                        float* d_wav, int64_t wav_stride) {
    if (!ctx || !d_hi || !d_lo || !d_w || !d_bias || !d_wav || B < 1 || T < 1 || C < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_final_conv: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_final_conv(ctx, (const bf16_t*)d_hi, (const bf16_t*)d_lo, B, T, C, d_w, d_bias, d_wav, wav_stride));
}

// ------------------------------------------------------------------ the conditioning front-end's kernels (encoder.hip through its launchers)
int rt_debug_enc_conv0(rt_ctx* ctx, const float* d_pcm, int64_t T, int32_t C, int32_t K, const float* d_w, const float* d_bias, float* d_x, void* d_hi,
                       void* d_lo) {
    if (!ctx || !d_pcm || !d_w || !d_bias || !d_x || !d_hi || !d_lo || T < 0 || K < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_enc_conv0: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_enc_conv0(ctx, d_pcm, T, C, K, d_w, d_bias, d_x, (bf16_t*)d_hi, (bf16_t*)d_lo));
}

int rt_debug_rvq(rt_ctx* ctx, const float* d_sem, float* d_aco, int32_t T, int32_t D, int32_t K, int32_t Q, const void* const* h_cbT, int32_t* d_codes) {
    if (!ctx || !d_sem || !d_aco || !d_codes || T < 0 || D < 1 || K < 1 || (Q > 0 && !h_cbT)) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_rvq: bad argument");
    for (int q = 0; q < Q; ++q)
        if (!h_cbT[q]) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_rvq: codebook %d is null", q);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DbgBufs bufs(ctx);
    const float** d_cbT = nullptr;
    if (Q > 0) {
        RT_HIP(ctx, bufs.alloc(&d_cbT, sizeof(float*) * (size_t)Q));
        RT_HIP(ctx, hipMemcpy(d_cbT, h_cbT, sizeof(float*) * (size_t)Q, hipMemcpyHostToDevice));
    }
    return dbg_finish(ctx, launch_rvq(ctx, d_sem, d_aco, T, D, K, Q, d_cbT, d_codes));
}

int rt_debug_stats_pool(rt_ctx* ctx, const float* d_x, int32_t T, int32_t C, float* d_out) {
    if (!ctx || !d_x || !d_out || C < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stats_pool: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_stats_pool(ctx, d_x, T, C, d_out));
}

int rt_debug_gemv_f32(rt_ctx* ctx, const float* d_W, const float* d_b_or_NULL, const float* d_x, int32_t N, int32_t K, int32_t relu, float* d_y) {
    if (!ctx || !d_W || !d_x || !d_y || N < 1 || K < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemv_f32: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return dbg_finish(ctx, launch_gemv_f32(ctx, d_W, d_b_or_NULL, d_x, N, K, relu, d_y));
}

// rt_debug_gemm's tiled mode with the whole GemmEpi exposed, and optionally the fused conv pair
namespace {
bool dbg_epi(const rt_debug_epi& s, int N, GemmEpi* e) {
    e->bias = s.bias; e->scale = s.scale; e->residual = s.residual; e->out_f32 = s.out_f32; e->out_bf16 = (bf16_t*)s.out_bf16;
    e->act = s.act; e->snake_a = s.snake_a; e->snake_ib = s.snake_ib; e->out2_bf16 = (bf16_t*)s.out2_bf16; e->out2_f32 = s.out2_f32;
    e->out_hi = (bf16_t*)s.out_hi; e->out_lo = (bf16_t*)s.out_lo; e->out2_hi = (bf16_t*)s.out2_hi; e->out2_lo = (bf16_t*)s.out2_lo;
    e->snake2_a = s.snake2_a; e->snake2_ib = s.snake2_ib; e->act2 = s.act2; e->ldc = s.ldc > 0 ? s.ldc : N; e->split_k = 1;
    const bool two = s.out2_f32 || s.out2_bf16 || s.out2_hi || s.out2_lo;
    // what the kernel would dereference without a test of its own (the plane pairs are the launcher's to refuse)
    return e->ldc >= N && s.act >= ACT_NONE && s.act <= ACT_ELU && (s.act != ACT_SNAKE || (s.snake_a && s.snake_ib)) &&
           (!two || s.act2 == ACT_ELU || (s.act2 == ACT_SNAKE && s.snake2_a && s.snake2_ib));
}
}  // namespace

int rt_debug_gemm_epi(rt_ctx* ctx, const void* d_a, int32_t a_form, int64_t M, int32_t cin, int32_t taps, int32_t tap_stride, int32_t tap_offset,
                      int32_t rows_out, int32_t rows_in, const void* d_w_bf16, int32_t N, const rt_debug_epi* e, const void* d_w2_bf16,
                      const rt_debug_epi* e2, int32_t pair_mode) {
    if (!ctx || !d_a || !d_w_bf16 || !e || M < 1 || N < 1 || cin < 8 || taps < 1 || a_form < 0 || a_form > 3 || (rows_out > 0 && (rows_in < 1 || M % rows_out)) ||
        (d_w2_bf16 && (!e2 || (pair_mode != 1 && pair_mode != 2))))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm_epi: bad argument");
    GemmEpi ge, ge2;
    if (!dbg_epi(*e, N, &ge) || (d_w2_bf16 && !dbg_epi(*e2, N, &ge2)))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_gemm_epi: ldc < N, an unknown activation or SnakeBeta without its constants");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DbgBufs bufs(ctx);
    const int K = cin * taps;
    bf16_t *packed = nullptr, *packed2 = nullptr;
    RT_HIP(ctx, bufs.alloc(&packed, packed_bytes(N, K)));
    PackedW pw, pw2;
    RT_TRY(launch_pack_weight(ctx, (const bf16_t*)d_w_bf16, N, K, packed, &pw));
    GemmA a; a.ptr = d_a; a.is_f32 = a_form == 1 || a_form == 2; a.split = a_form >= 2; a.M = M; a.Cin = cin; a.taps = taps; a.tap_stride = tap_stride;
    a.tap_offset = tap_offset; a.rows_out = rows_out; a.rows_in = rows_in;
    if (a_form == 3) {           // operand planes: the bf16 hi plane, then the bf16 lo plane, each [input rows][cin]
        const int64_t in_rows = rows_out > 0 ? (M / rows_out) * rows_in : M;
        a.ptr_lo = (const bf16_t*)d_a + in_rows * cin;
    }
    int rc;
    if (d_w2_bf16) {
        RT_HIP(ctx, bufs.alloc(&packed2, packed_bytes(N, N)));
        RT_TRY(launch_pack_weight(ctx, (const bf16_t*)d_w2_bf16, N, N, packed2, &pw2));
        if (pair_mode == 1 && !conv_pair_fusable(a, pw, ge, pw2)) rc = rt_fail(ctx, RT_ERR_UNSUPPORTED, "rt_debug_gemm_epi: conv_pair_fusable declines this pair");
        else rc = launch_gemm(ctx, a, pw, ge, &pw2, &ge2);
    } else {
        rc = launch_gemm(ctx, a, pw, ge);
    }
    return dbg_finish(ctx, rc);
}

int rt_debug_tune(int32_t code, int32_t arg) {
    // exclusive: waits until no call is executing on any context (CtxLock holds this lock shared), and a resumable generation in
    // flight keeps the plan it began with - the switch is refused rather than applied under it
    std::unique_lock<std::shared_mutex> all(g_tune_mu);
    if (g_runs_in_flight.load() > 0) return RT_ERR_STATE;
    for (const KnobRow& r : kKnobs)
        if (code >= r.base + r.lo && code <= r.base + r.hi) {
            *r.knob = code - r.base;
            if (r.base == kKnobArg[0].base && arg >= kKnobArg[0].lo && arg <= kKnobArg[0].hi) *kKnobArg[0].knob = arg;
            ++g_tune_epoch;
            return RT_OK;
        }
    return RT_ERR_INVALID;          // a code no row of knobs.h accepts: nothing changes
}

// launch_gemm_col's row-block decision (gemm_col.hip col_workgroups + col_row_blocks) without a launch
int rt_debug_col_row_blocks(int32_t n_cu, int32_t M, int32_t N, int32_t epi, int32_t split) {
    if (n_cu < 1 || M < 1 || M > 128 || N < 1 || epi < COL_STORE || epi > COL_SILU || (epi == COL_SILU && N % 32) || split > 4 || split == 3) return -1;
    std::shared_lock<std::shared_mutex> plan(g_tune_mu);      // (the switches do not move under the two reads)
    bool x_form = false;
    const int wg = col_workgroups(n_cu, M, N, epi, split, &x_form);
    return col_row_blocks(n_cu, M, wg, x_form);
}

// ... and its tile-block decision (col_tile_blocks, taken only where the row-block rule does not hold)
int rt_debug_col_tile_blocks(int32_t n_cu, int32_t M, int32_t N, int32_t epi, int32_t split) {
    if (n_cu < 1 || M < 1 || M > 128 || N < 1 || epi < COL_STORE || epi > COL_SILU || (epi == COL_SILU && N % 32) || split > 4 || split == 3) return -1;
    std::shared_lock<std::shared_mutex> plan(g_tune_mu);
    if (epi == COL_SILU) return 0;
    if (split <= 0) split = col_split_for(N, n_cu);
    bool x_form = false;
    if (col_row_blocks(n_cu, M, col_workgroups(n_cu, M, N, epi, split, &x_form), x_form)) return 0;
    return col_tile_blocks(n_cu, M, (N + 15) / 16, epi, split);
}

int rt_bench_gemm_skinny(rt_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t split_k, int32_t n_mats, int32_t iters, double* avg_us,
                         int32_t* used_split) {
    if (!ctx || !avg_us || M < 1 || M > 64 || N < 32 || K < 16 || K % 16 || n_mats < 1 || iters < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_gemm_skinny: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = packed_bytes(N, K);
    bf16_t* wbuf = nullptr;
    bf16_t* a = nullptr;
    float* out = nullptr;
    if (split_k < 1) split_k = skinny_pick_split(M, N, K, ctx->n_cu);
    if (used_split) *used_split = split_k;
    RT_HIP(ctx, hipMalloc((void**)&wbuf, pb * n_mats));
    RT_HIP(ctx, hipMalloc((void**)&a, (size_t)M * K * 2));
    RT_HIP(ctx, hipMalloc((void**)&out, (size_t)split_k * M * N * 4));
    RT_HIP(ctx, hipMemsetAsync(wbuf, 0x3c, pb * n_mats, ctx->stream));     // bf16 0x3c3c = 0.0115: non-zero operands
    RT_HIP(ctx, hipMemsetAsync(a, 0x3c, (size_t)M * K * 2, ctx->stream));
    PackedW pw;
    pw.N = N; pw.K = K; pw.Np = (N + 31) / 32 * 32; pw.Kp = K;
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    int rc = RT_OK;
    for (int i = 0; i < n_mats && !rc; ++i) { pw.data = wbuf + (pb / 2) * i; rc = launch_gemm_skinny(ctx, a, M, pw, out, N, split_k); }
    RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters && !rc; ++i) { pw.data = wbuf + (pb / 2) * (i % n_mats); rc = launch_gemm_skinny(ctx, a, M, pw, out, N, split_k); }
    RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(wbuf); (void)hipFree(a); (void)hipFree(out);
    return rc;
}

// Back-to-back launches of the column-owner GEMM over n_mats weight matrices (> 512 MB in total => HBM-cold).
int rt_bench_gemm_col(rt_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t a_norm, int32_t epi, int32_t n_mats, int32_t iters,
                      double* avg_us, int64_t* stamps8) {
    if (!ctx || !avg_us || M < 1 || M > 128 || N < 64 || K < 16 || K % 16 || n_mats < 1 || iters < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_gemm_col: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = packed_bytes(N, K);
    bf16_t* wbuf = nullptr;
    void* a = nullptr;
    float *out = nullptr, *rowsq = nullptr, *rowsq_out = nullptr, *normw = nullptr;
    bf16_t* act = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&wbuf, pb * n_mats));
    const size_t R = M > 64 ? 128 : 64;      // rows the buffers hold (whole 32-row blocks of the tiled ones)
    RT_HIP(ctx, hipMalloc(&a, R * K * 4));
    RT_HIP(ctx, hipMalloc((void**)&out, R * N * 4));
    RT_HIP(ctx, hipMalloc((void**)&act, R * N * 2));
    RT_HIP(ctx, hipMalloc((void**)&rowsq, R * 512 * 4));
    RT_HIP(ctx, hipMalloc((void**)&rowsq_out, R * (N / 4 + 4) * 4));
    RT_HIP(ctx, hipMalloc((void**)&normw, (size_t)std::max(K, N) * 4));
    RT_HIP(ctx, hipMemsetAsync(wbuf, 0x3c, pb * n_mats, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(a, 0x3c, R * K * 4, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(out, 0, R * N * 4, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(rowsq, 0x3c, R * 512 * 4, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(normw, 0x3c, (size_t)std::max(K, N) * 4, ctx->stream));
    PackedW pw;
    pw.N = N; pw.K = K; pw.Np = (N + 31) / 32 * 32; pw.Kp = K; pw.Np16 = (N + 15) / 16 * 16;
    ColArgs c;
    c.nt = (a_norm & 2) ? 0 : 1;             // bit 1: cacheable weight loads (hot-cache experiment with n_mats = 1)
    a_norm &= 1;
    // (as many partials per row as the RESID launch of width K in front of such a launch emits: 256 at K = 2048, 128 at K = 1024)
    c.A = a; c.post_scale = a_norm; c.rowsq = rowsq; c.rowsq_n = K / 16 * col_split_for(K, ctx->n_cu); c.eps = 1e-6f; c.M = M; c.K = K; c.epi = epi;
    c.next_bf16 = epi == COL_RESID ? act : nullptr; c.next_norm_w = normw;
    c.out = out; c.ldc = epi == COL_SILU ? N / 2 : N; c.split = epi == COL_SILU ? col_split_silu(N, ctx->n_cu) : col_split_for(N, ctx->n_cu);
    c.rowsq_out = rowsq_out; c.rowsq_out_n = N / 16 * c.split; c.out_bf16 = act;
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    int rc = RT_OK;
    // 65..128 rows: one 128-row launch, or (rt_debug_tune 3200) the two 64-row launches it replaces - the A/B of g_col_rows128
    auto launch = [&](const ColArgs& c1) {
        if (c1.M <= 64 || g_col_rows128) return launch_gemm_col(ctx, c1, pw);
        ColArgs lo = c1, hi = c1;
        lo.M = 64; hi.M = c1.M - 64; hi.row_off = 64;
        const int r = launch_gemm_col(ctx, lo, pw);
        return r ? r : launch_gemm_col(ctx, hi, pw);
    };
    for (int i = 0; i < n_mats && !rc; ++i) { pw.data16 = wbuf + (pb / 2) * i; rc = launch(c); }
    RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters && !rc; ++i) {
        pw.data16 = wbuf + (pb / 2) * (i % n_mats);
        rc = launch(c);
    }
    RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / iters;
    if (stamps8 && !rc) {       // one more launch with the in-kernel phase stamps of workgroup 0
        long long* st = nullptr;
        RT_HIP(ctx, hipMalloc((void**)&st, 64));
        RT_HIP(ctx, hipMemsetAsync(st, 0, 64, ctx->stream));
        c.stamps = st;
        pw.data16 = wbuf + (pb / 2) * (iters % n_mats);
        rc = launch_gemm_col(ctx, c, pw);
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the context's stream does not wait for, nor hold up, the copy below)
        RT_HIP(ctx, hipMemcpy(stamps8, st, 64, hipMemcpyDeviceToHost));
        (void)hipFree(st);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(wbuf); (void)hipFree(a); (void)hipFree(out); (void)hipFree(act); (void)hipFree(rowsq); (void)hipFree(rowsq_out); (void)hipFree(normw);
    return rc;
}

// Launch-floor microbenchmark: n dependent launches of a trivial kernel (grid_wgs x 256 threads), eagerly or as one
// captured hipGraph replayed `reps` times.  Returns microseconds per launch.
int rt_bench_launch(rt_ctx* ctx, int32_t grid_wgs, int32_t n, int32_t use_graph, int32_t reps, double* us_per_launch) {
    if (!ctx || !us_per_launch || grid_wgs < 1 || n < 1 || reps < 1) return RT_ERR_INVALID;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    float* buf = nullptr;
    const int elems = grid_wgs * 256;
    RT_HIP(ctx, hipMalloc((void**)&buf, (size_t)elems * 4));
    RT_HIP(ctx, hipMemsetAsync(buf, 0, (size_t)elems * 4, ctx->stream));
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (use_graph) {
        RT_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_touch, dim3(grid_wgs), dim3(256), 0, ctx->stream, buf, elems);
        RT_HIP(ctx, hipStreamEndCapture(ctx->stream, &graph));
        RT_HIP(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        RT_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_touch, dim3(grid_wgs), dim3(256), 0, ctx->stream, buf, elems);
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int rpt = 0; rpt < reps; ++rpt) {
        if (use_graph) RT_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
        else for (int i = 0; i < n; ++i) hipLaunchKernelGGL(k_touch, dim3(grid_wgs), dim3(256), 0, ctx->stream, buf, elems);
    }
    RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *us_per_launch = (double)ms * 1e3 / ((double)n * reps);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    return RT_OK;
}

// Sampler microbenchmark: `iters` back-to-back launches over M rows of V logits; returns the average launch time and
// (row 0 of the last launch) the 100-MHz wall-clock stamps at the kernel's phase boundaries.
int rt_bench_sample(rt_ctx* ctx, const float* d_logits, int32_t M, int32_t V, const rt_sampling* sp, int32_t iters, double* avg_us,
                    int64_t* stamps8) {
    if (!ctx || !d_logits || !sp || !avg_us || M < 1 || iters < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_sample: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int64_t* items = nullptr;
    int32_t* out = nullptr;
    long long* st = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&items, (size_t)M * 8));
    RT_HIP(ctx, hipMalloc((void**)&out, (size_t)M * 4));
    RT_HIP(ctx, hipMalloc((void**)&st, 8 * 8));
    RT_HIP(ctx, hipMemsetAsync(st, 0, 64, ctx->stream));
    hipLaunchKernelGGL(k_iota64, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, items, M);
    SampleArgs a{};
    a.logits = d_logits; a.n_slabs = 1; a.M = M; a.V = V;
    a.do_sample = sp->do_sample; a.temperature = sp->temperature; a.top_k = sp->top_k; a.top_p = sp->top_p; a.rep_penalty = sp->repetition_penalty;
    a.suppress_from = V; a.allow_token = -1; a.seed = 1; a.item_ids = items; a.out = out; a.out_stride = 1; a.eos_token = -1;
    a.stamps = st;
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    int rc = launch_sample(ctx, a);
    RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters && rc == RT_OK; ++i) { a.frame = i; rc = launch_sample(ctx, a); }
    RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / iters;
    if (stamps8) RT_HIP(ctx, hipMemcpy(stamps8, st, 64, hipMemcpyDeviceToHost));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(items); (void)hipFree(out); (void)hipFree(st);
    return rc;
}

// Decode-attention microbenchmark: `iters` back-to-back launches of the decode step's fused attention over M rows, each row at
// position prefix_len + own_len - 1 of its own slot, positions < prefix_len read from a shared prefix slot (shared != 0) or from
// the row's own slot (shared == 0: what the launch would cost without the shared voice prefix).  The launches cycle through
// `layers` cache regions (as the model's 28 layers do: a layer's K / V is L2-cold when its turn comes).  Operands are zeros
// (uniform softmax): the timing does not depend on the values.
int rt_bench_attention_fused(rt_ctx* ctx, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t prefix_len, int32_t own_len,
                             int32_t shared, int32_t layers, int32_t iters, double* avg_us) {
    if (!ctx || !avg_us || M < 1 || M > 128 || heads < 1 || kv_heads < 1 || heads % kv_heads || prefix_len < 0 || own_len < 1 || layers < 1 || iters < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_attention_fused: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // (more than 64 cache rows select the 16-wave form of the talker's decode step; the predictor's <= 16 positions the 4-wave form)
    const int max_pos = std::max((prefix_len + own_len + 8 + 63) / 64 * 64, (prefix_len > 0 || own_len > 16) ? 128 : 64), slots = M + 1, width = (heads + 2 * kv_heads) * head_dim;
    KvCache kv;
    kv.layers = layers; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    kv.prefix_slot = shared && prefix_len > 0 ? M : -1;
    kv.prefix_len = kv.prefix_slot >= 0 ? prefix_len : 0;
    const size_t cache_bytes = (size_t)layers * kv.layer_stride() * sizeof(bf16_t);
    float *qkv = nullptr, *cs = nullptr, *nw = nullptr;
    int32_t *pos = nullptr, *slot = nullptr;
    bf16_t* out = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&kv.k, cache_bytes));
    RT_HIP(ctx, hipMalloc((void**)&kv.v, cache_bytes));
    RT_HIP(ctx, hipMalloc((void**)&qkv, (size_t)M * width * 4));
    RT_HIP(ctx, hipMalloc((void**)&cs, (size_t)max_pos * head_dim * 4));
    RT_HIP(ctx, hipMalloc((void**)&nw, (size_t)head_dim * 4));
    RT_HIP(ctx, hipMalloc((void**)&pos, (size_t)M * 4));
    RT_HIP(ctx, hipMalloc((void**)&slot, (size_t)M * 4));
    RT_HIP(ctx, hipMalloc((void**)&out, ((size_t)M + 31) / 32 * 32 * heads * head_dim * 2));
    RT_HIP(ctx, hipMemsetAsync(kv.k, 0, cache_bytes, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(kv.v, 0, cache_bytes, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(qkv, 0, (size_t)M * width * 4, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(cs, 0, (size_t)max_pos * head_dim * 4, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(nw, 0, (size_t)head_dim * 4, ctx->stream));
    std::vector<int32_t> hp(M, prefix_len + own_len - 1), hs(M);
    for (int i = 0; i < M; ++i) hs[i] = i;
    RT_HIP(ctx, hipMemcpyAsync(pos, hp.data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(slot, hs.data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream));
    bf16_t* tiles = nullptr;
    if (kv.prefix_slot >= 0 && prefix_len >= 64 && head_dim == 128) {      // fragment-tiled prefix copies: what the matrix-core forms read
        kv.vt_stride = (prefix_len + 31) / 32 * 4096;
        kv.prefix_slot_alloc = kv.prefix_slot;
        RT_HIP(ctx, hipMalloc((void**)&tiles, (size_t)2 * layers * kv_heads * kv.vt_stride * 2));
        kv.kt_prefix = tiles;
        kv.vt_prefix = tiles + (size_t)layers * kv_heads * kv.vt_stride;
        const int rt = launch_transpose_prefix_v(ctx, kv, prefix_len);
        if (rt) return rt;
    }
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    const float* cosT = cs;
    const float* sinT = cs + (size_t)max_pos * head_dim / 2;
    int rc = RT_OK;
    for (int i = 0; i < layers && rc == RT_OK; ++i)          // warm-up: one pass over every layer
        rc = launch_attention_fused(ctx, qkv, M, heads, kv_heads, head_dim, nw, nw, 1e-6f, cosT, sinT, slot, pos, 0, 0, kv, i, out, nullptr, 1, -1);
    RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // more than 64 rows: frame-indexed, as a decode step on a wide batch launches it (one launch that keeps the 16-wave split);
    // shared & 2: the same rows as blocks of 64 (the alternative that was weighed against it)
    int32_t* frame = nullptr;
    if (M > 64) {
        RT_HIP(ctx, hipMalloc((void**)&frame, 4));
        RT_HIP(ctx, hipMemsetAsync(frame, 0, 4, ctx->stream));
    }
    const int blk = (M > 64 && (shared & 2)) ? 64 : M;
    for (int i = 0; i < iters && rc == RT_OK; ++i)
        for (int r0 = 0; r0 < M && rc == RT_OK; r0 += blk)
            rc = launch_attention_fused(ctx, qkv + (size_t)r0 * width, std::min(blk, M - r0), heads, kv_heads, head_dim, nw, nw, 1e-6f, cosT, sinT, slot + r0, pos + r0, 0,
                                        0, kv, i % layers, out + (size_t)r0 * heads * head_dim, frame, 1, -1);
    RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    for (void* p : {(void*)kv.k, (void*)kv.v, (void*)qkv, (void*)cs, (void*)nw, (void*)pos, (void*)slot, (void*)out, (void*)tiles, (void*)frame}) if (p) (void)hipFree(p);
    return rc;
}

// The decode step's attention launch back to back, single-voice kernel against multi-voice kernel (tools/bench_voices.py): M rows at
// position prefix_len + own_len - 1 behind n_voices prefixes of prefix_len rows each (slots M ..), zeros as operands, cycling through
// `layers` cache regions.  Single: every row behind voice 0 (launch_attention_fused as a single-voice run takes it).  Multi: block b
// behind voice b % n_voices, read from the block table.  Two alternating passes of `iters` launches each; the mean per launch.
int rt_bench_attention_fused_voices(rt_ctx* ctx, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t prefix_len, int32_t own_len,
                                    int32_t n_voices, int32_t layers, int32_t iters, double* us_single, double* us_multi) {
    if (!ctx || !us_single || !us_multi || M < 1 || M > 128 || heads < 1 || kv_heads < 1 || heads % kv_heads || prefix_len < 1 || own_len < 1 || layers < 1 ||
        iters < 1 || n_voices < 1 || n_voices > 8 || (head_dim != 32 && head_dim != 64 && head_dim != 128))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_attention_fused_voices: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int max_pos = std::max((prefix_len + own_len + 8 + 63) / 64 * 64, 128), slots = M + n_voices, width = (heads + 2 * kv_heads) * head_dim;
    const int n_blocks = (M + 3) / 4;
    KvCache kv;
    kv.layers = layers; kv.slots = slots; kv.kv_heads = kv_heads; kv.max_pos = max_pos; kv.head_dim = head_dim;
    const size_t cache_bytes = (size_t)layers * kv.layer_stride() * sizeof(bf16_t);
    std::vector<void*> owned;
    auto cleanup = [&]() { for (void* p : owned) (void)hipFree(p); };
    auto alloc = [&](size_t bytes, bool zero) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        owned.push_back(p);
        if (zero) (void)hipMemsetAsync(p, 0, bytes, ctx->stream);
        return p;
    };
    kv.k = (bf16_t*)alloc(cache_bytes, true); kv.v = (bf16_t*)alloc(cache_bytes, true);
    float* qkv = (float*)alloc((size_t)M * width * 4, true);
    float* cs = (float*)alloc((size_t)max_pos * head_dim * 4, true);
    float* nw = (float*)alloc((size_t)head_dim * 4, true);
    int32_t* pos = (int32_t*)alloc((size_t)M * 4, false);
    int32_t* slot = (int32_t*)alloc((size_t)M * 4, false);
    int32_t* frame = (int32_t*)alloc(4, true);
    bf16_t* out = (bf16_t*)alloc(((size_t)M + 31) / 32 * 32 * heads * head_dim * 2, false);
    VoiceBlock* d_blocks = (VoiceBlock*)alloc((size_t)n_blocks * sizeof(VoiceBlock), false);
    int32_t* d_lists = (int32_t*)alloc((size_t)(n_blocks + M) * 4, false);
    if (!kv.k || !kv.v || !qkv || !cs || !nw || !pos || !slot || !frame || !out || !d_blocks || !d_lists) {
        cleanup();
        return rt_fail(ctx, RT_ERR_OOM, "rt_bench_attention_fused_voices: out of memory");
    }
    std::vector<int32_t> hp(M, prefix_len + own_len - 1), hs(M);
    for (int i = 0; i < M; ++i) hs[i] = i;
    hipError_t e = hipMemcpyAsync(pos, hp.data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(slot, hs.data(), (size_t)M * 4, hipMemcpyHostToDevice, ctx->stream);
    // tiles per voice, where the matrix-core form takes them: [voice][K | V][layers][kv_heads][vt_stride]
    bf16_t* tiles = nullptr;
    int64_t per_plane = 0;
    int rc = RT_OK;
    if (e == hipSuccess && prefix_len >= 64 && head_dim == 128) {
        kv.vt_stride = (prefix_len + 31) / 32 * 4096;
        per_plane = (int64_t)layers * kv_heads * kv.vt_stride;
        tiles = (bf16_t*)alloc((size_t)2 * n_voices * per_plane * 2, false);
        if (!tiles) { cleanup(); return rt_fail(ctx, RT_ERR_OOM, "rt_bench_attention_fused_voices: out of memory"); }
        for (int v = 0; v < n_voices && rc == RT_OK; ++v) {
            kv.kt_prefix = tiles + 2 * v * per_plane; kv.vt_prefix = kv.kt_prefix + per_plane; kv.prefix_slot_alloc = M + v;
            rc = launch_transpose_prefix_v(ctx, kv, prefix_len);
        }
    }
    VoiceTable vt;
    std::vector<VoiceBlock> blocks(n_blocks);
    std::vector<int32_t> lists(n_blocks + M, -1);
    vt.rows = M; vt.n_blocks = n_blocks; vt.blocks = d_blocks; vt.mfma_blocks = d_lists; vt.vec_rows = d_lists + n_blocks;
    kv.kt_prefix = tiles; kv.vt_prefix = tiles ? tiles + per_plane : nullptr;        // voice 0: the single-voice launch's
    const bool mf = attention_mfma_voice_ok(heads, kv_heads, head_dim, kv, prefix_len);
    for (int b = 0, n_vr = 0; b < n_blocks; ++b) {
        const int v = b % n_voices;
        blocks[b].prefix_slot = M + v; blocks[b].prefix_len = prefix_len;
        blocks[b].kt = mf ? tiles + 2 * v * per_plane : nullptr; blocks[b].vt = mf ? blocks[b].kt + per_plane : nullptr;
        if (mf) lists[b] = b;
        else for (int r = 4 * b; r < std::min(M, 4 * b + 4); ++r) lists[n_blocks + n_vr++] = r;
    }
    vt.any_mfma = mf; vt.any_vec = !mf;
    if (e == hipSuccess) e = hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(VoiceBlock), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_lists, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (e == hipSuccess) e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    const float* cosT = cs;
    const float* sinT = cs + (size_t)max_pos * head_dim / 2;
    double total[2] = {0.0, 0.0};
    for (int pass = 0; pass < 3 && rc == RT_OK && e == hipSuccess; ++pass)          // pass 0 warms both forms up and is not counted
        for (int which = 0; which < 2 && rc == RT_OK && e == hipSuccess; ++which) {
            kv.voices = which ? &vt : nullptr;
            kv.prefix_slot = which ? -1 : M; kv.prefix_len = which ? 0 : prefix_len;
            const int n = pass ? iters : layers;
            e = hipEventRecord(ev[0], ctx->stream);
            for (int i = 0; i < n && rc == RT_OK; ++i)
                rc = launch_attention_fused(ctx, qkv, M, heads, kv_heads, head_dim, nw, nw, 1e-6f, cosT, sinT, slot, pos, 0, 0, kv, i % layers, out, frame, 1, -1);
            if (e == hipSuccess) e = hipEventRecord(ev[1], ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            float ms = 0;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
            if (pass) total[which] += ms;
        }
    *us_single = total[0] * 1e3 / (2.0 * iters);
    *us_multi = total[1] * 1e3 / (2.0 * iters);
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    cleanup();
    RT_HIP(ctx, e);
    return rc;
}

// Grid-barrier microbenchmark: one persistent launch of `wgs` x `threads`, n barriers; microseconds per barrier (and the
// abort flag: non-zero = the grid was not co-resident or a spin bound was hit).
int rt_bench_grid_barrier(rt_ctx* ctx, int32_t wgs, int32_t threads, int32_t n, int32_t mode, double* us_per_barrier, int32_t* aborted) {
    if (!ctx || !us_per_barrier || wgs < 1 || threads < 64 || threads > 1024 || n < 1) return RT_ERR_INVALID;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int per_cu = 0;
    auto kern = mode == 2 ? k_bench_barrier<2> : (mode == 1 ? k_bench_barrier<1> : k_bench_barrier<0>);
    if (mode >= 3 && (threads < 512 || wgs % 16)) return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_grid_barrier: the pair modes take >= 512 threads and a multiple of 16 workgroups");
    RT_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0));
    if ((int64_t)per_cu * ctx->n_cu < wgs) return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_grid_barrier: %d workgroups cannot be co-resident (%d per CU x %d CUs)", wgs, per_cu, ctx->n_cu);
    unsigned* bar = nullptr;
    float* buf = nullptr;
    unsigned* flags = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&bar, 64));
    RT_HIP(ctx, hipMalloc((void**)&buf, (size_t)wgs * threads * 4));
    RT_HIP(ctx, hipMalloc((void**)&flags, (size_t)wgs * 128));
    RT_HIP(ctx, hipMemsetAsync(buf, 0, (size_t)wgs * threads * 4, ctx->stream));
    hipEvent_t e0, e1;
    RT_HIP(ctx, hipEventCreate(&e0));
    RT_HIP(ctx, hipEventCreate(&e1));
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {
        RT_HIP(ctx, hipMemsetAsync(bar, 0, 64, ctx->stream));
        RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
        RT_HIP(ctx, hipMemsetAsync(buf, 0, (size_t)wgs * threads * 4, ctx->stream));
        RT_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)wgs * 128, ctx->stream));
        if (mode == 3) hipLaunchKernelGGL(k_bench_pair<1>, dim3(wgs), dim3(threads), 0, ctx->stream, flags, n, buf, bar);
        else if (mode == 4) hipLaunchKernelGGL(k_bench_pair<8>, dim3(wgs), dim3(threads), 0, ctx->stream, flags, n, buf, bar);
        else hipLaunchKernelGGL(kern, dim3(wgs), dim3(threads), 0, ctx->stream, bar, n, buf);
        RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    }
    unsigned h[3] = {0, 0, 0};
    RT_HIP(ctx, hipMemcpy(h, bar, 12, hipMemcpyDeviceToHost));
    if (aborted) *aborted = (int32_t)(h[1] | (h[2] << 1));     // bit 0: spin bound hit, bit 1: a stale value was read
    *us_per_barrier = (double)ms * 1e3 / n;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(bar); (void)hipFree(buf); (void)hipFree(flags);
    return RT_OK;
}

// The kernels of rt_stt_align one at a time (csrc/stt_align.hip): the production launchers over tables made for the call
int rt_debug_stt_align_probs(rt_ctx* ctx, const float* d_q, int32_t q_rows, int32_t heads, int32_t head_dim, const uint16_t* d_k_hi, const uint16_t* d_k_lo,
                             int32_t slots, int32_t n_ctx, const int32_t* h_src, const int32_t* h_slot, const int32_t* h_frames, int32_t n_rows,
                             const int32_t* h_heads, int32_t n_heads, int32_t ldw, float* d_W) {
    if (!ctx || !d_q || !d_k_hi || !h_src || !h_slot || !h_frames || !h_heads || !d_W || q_rows < 1 || heads < 1 || slots < 1 || n_ctx < 1 || n_rows < 1 ||
        n_heads < 1 || n_heads > ALIGN_HEADS_MAX || ldw < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_align_probs: bad argument");
    AlignHeads hs{};
    for (int i = 0; i < n_heads; ++i) {
        if (h_heads[i] < 0 || h_heads[i] >= heads) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_align_probs: head %d outside %d heads", h_heads[i], heads);
        hs.head[i] = h_heads[i]; hs.out[i] = i;
    }
    hs.n = n_heads;
    std::vector<int32_t> tab(3 * (size_t)n_rows);
    std::vector<int64_t> off(n_rows);
    for (int a = 0; a < n_rows; ++a) {
        if (h_src[a] < 0 || h_src[a] >= q_rows || h_slot[a] < 0 || h_slot[a] >= slots || h_frames[a] < 0 || h_frames[a] > std::min(ldw, n_ctx))
            return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_align_probs: row %d: source row, slot or frames out of range", a);
        tab[a] = h_src[a]; tab[n_rows + a] = h_slot[a]; tab[2 * (size_t)n_rows + a] = h_frames[a];
        off[a] = (int64_t)a * ldw;
    }
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* d_tab = nullptr;
    int64_t* d_off = nullptr;
    auto run = [&]() -> int {
        RT_HIP(ctx, hipMalloc((void**)&d_tab, tab.size() * 4));
        RT_HIP(ctx, hipMalloc((void**)&d_off, off.size() * 8));
        RT_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(ctx, hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        KvCache kv;
        kv.layers = 1; kv.slots = slots; kv.kv_heads = heads; kv.max_pos = n_ctx; kv.head_dim = head_dim;
        kv.k = (bf16_t*)d_k_hi; kv.k_lo = (bf16_t*)d_k_lo;
        RT_TRY(launch_align_probs(ctx, d_q, heads, head_dim, kv, 0, AlignRows{d_tab, d_tab + n_rows, d_tab + 2 * (size_t)n_rows, d_off}, n_rows, hs, (int64_t)n_rows * ldw, d_W));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RT_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    if (d_tab) (void)hipFree(d_tab);
    if (d_off) (void)hipFree(d_off);
    return rc;
}

int rt_debug_stt_align_matrix(rt_ctx* ctx, const float* d_W, int32_t n_heads, int32_t n, int32_t F, int32_t median_width, float* d_M) {
    if (!ctx || !d_W || !d_M || n < 1 || F < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_align_matrix: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const AlignWin win{n, F, 0, 0, 0, 0};
    AlignWin* d_win = nullptr;
    double* stats = nullptr;
    auto run = [&]() -> int {
        RT_HIP(ctx, hipMalloc((void**)&d_win, sizeof(AlignWin)));
        RT_HIP(ctx, hipMalloc((void**)&stats, (size_t)std::max(n_heads, 1) * F * 2 * sizeof(double)));
        RT_HIP(ctx, hipMemcpyAsync(d_win, &win, sizeof(AlignWin), hipMemcpyHostToDevice, ctx->stream));
        RT_TRY(launch_align_matrix(ctx, d_W, d_win, 1, n_heads, (int64_t)n * F, F, n, F, median_width, stats, d_M));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RT_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    if (d_win) (void)hipFree(d_win);
    if (stats) (void)hipFree(stats);
    return rc;
}

int rt_debug_stt_dtw(rt_ctx* ctx, const float* d_M, int32_t n, int32_t F, int32_t trace_mode, int32_t* h_frames) {
    if (!ctx || !d_M || !h_frames || n < 1 || F < 1 || trace_mode < -1 || trace_mode > 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_dtw: bad argument");
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const AlignWin win{n, F, 0, 0, 0, 0};
    AlignWin* d_win = nullptr;
    uint32_t* trace = nullptr;
    int32_t* frames = nullptr;
    auto run = [&]() -> int {
        RT_HIP(ctx, hipMalloc((void**)&d_win, sizeof(AlignWin)));
        RT_HIP(ctx, hipMalloc((void**)&trace, align_trace_words(n, F) * 4));
        RT_HIP(ctx, hipMalloc((void**)&frames, (size_t)n * 4));
        RT_HIP(ctx, hipMemcpyAsync(d_win, &win, sizeof(AlignWin), hipMemcpyHostToDevice, ctx->stream));
        RT_TRY(launch_align_dtw(ctx, d_M, d_win, 1, n, F, trace, trace_mode, frames));
        RT_HIP(ctx, hipMemcpyAsync(h_frames, frames, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RT_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)d_win, (void*)trace, (void*)frames}) if (p) (void)hipFree(p);
    return rc;
}

}  // extern "C"
