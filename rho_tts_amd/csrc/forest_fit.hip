// Training the accent-drift classifier's forests on the GPU (the trainer half): rt_forest_fit grows every tree of
// every forest of a CalibratedClassifierCV(RandomForestClassifier(...), cv)-shaped fit in ONE call.  rho_tts_amd/forest_train.py
// states the rules and holds the definition, fit_host; the two kernels here do its steps on its integers, so the tables are the host's
// bit for bit and a tree depends on nothing else in the call:
//
//   k_fit_rank   one thread per (feature, row): the row's position in the order of its column by (float32 value, row index), by
//                counting the rows before it (tiles of the column through LDS); writes rank[f][row] and the sorted column sval[f][rank].
//                Built once per call; a node's rows ordered by rank ARE its rows ordered by (value, row index).
//   k_fit_tree   one workgroup of 256 threads per (forest, tree).  Bootstrap multiplicities are counted in LDS (integer atomics on
//                16-bit halves) from the counter hash, the tree's distinct rows are compacted into a per-tree row array in global
//                memory, and the tree is grown depth first in pre-order from an explicit stack in LDS, so that the table layout (left
//                child = k + 1) falls out without renumbering.  A node is a contiguous span of the row array.  Per candidate feature the
//                node's rows are scattered to their rank positions in an LDS array of one 16-bit slot per data-set row (class and
//                multiplicity; 0 = not in the node) - no sort - every thread walks a contiguous piece of it behind a workgroup prefix
//                sum of (distinct rows, multiplicities per class, last occupied position), scores its boundaries from those integers in
//                float64, and a workgroup arg-max with the tie rule (larger score, then lower position; features in draw order, a later
//                one must be strictly better) picks the split.  The span is then partitioned by rank <= the split position.
//
// No floating-point atomics, no grid-wide barrier, no spin waits.  Every loop is bounded: the node loop by the tree's node capacity,
// the stack by max_depth + 2, the scans by the row count.  Built with -ffp-contract=off: a score's multiplies and adds round separately,
// as numpy's do.  rt_forest_fit is one host-to-device copy, two launches, one device-to-host copy and one stream synchronisation.
#include <algorithm>
#include <cmath>
#include <vector>

#include "forest_check.h"
#include "kernels.h"

namespace {

constexpr int FIT_MAX_ROWS = 16384;      // 16-bit ranks; one 16-bit LDS slot per row (32 KiB)
constexpr int FIT_MAX_FEATURES = 1024;   // the feature permutation of a node in LDS
constexpr int FIT_STACK = FOREST_MAX_DEPTH + 4;
constexpr int FIT_THREADS = 256;

struct FitArgs {
    const float* sval;              // [F][n] every column in order
    const unsigned short* rank;     // [F][n] the position of row i in its column's order
    const unsigned char* y;         // [n]
    const unsigned short* midx;     // [n_forests][n] the member rows of every forest, ascending
    const int* fhead;               // [n_forests][3]: member count, node capacity of a tree, first output node of the forest
    unsigned* rows_a;               // [trees][row_stride] row | class << 14 | multiplicity << 15
    unsigned* rows_b;               // the partition's other side
    double* out_value;
    int* out_feature;
    int* out_right;                 // tree-local
    int* out_count;                 // [trees]
    int n, n_features, n_trees, max_depth, min_leaf, min_split, max_features, bootstrap, row_stride;
    double w0, w1;
    unsigned seed_lo, seed_hi;
};

struct FitNode {
    int lo, m, m0, m1, depth, parent;
    unsigned key;
};

__device__ __forceinline__ unsigned fit_mix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned fit_draw(unsigned h, unsigned m) { return (unsigned)(((unsigned long long)h * m) >> 32); }

__global__ void __launch_bounds__(FIT_THREADS) k_fit_rank(const float* __restrict__ xT, int n, unsigned short* __restrict__ rank,
                                                          float* __restrict__ sval) {
    __shared__ float tile[FIT_THREADS];
    const int f = blockIdx.y, i = blockIdx.x * FIT_THREADS + threadIdx.x;
    const float* col = xT + (size_t)f * n;
    const float v = i < n ? col[i] : 0.0f;
    int before = 0;
    for (int base = 0; base < n; base += FIT_THREADS) {
        const int j = base + threadIdx.x;
        tile[threadIdx.x] = j < n ? col[j] : 0.0f;
        __syncthreads();
        const int cnt = min(FIT_THREADS, n - base);
        for (int k = 0; k < cnt; ++k) {
            const float u = tile[k];
            before += (u < v || (u == v && base + k < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n) {
        rank[(size_t)f * n + i] = (unsigned short)before;      // before < n <= 16384
        sval[(size_t)f * n + before] = v;
    }
}

// Exclusive prefix over the 256 threads of two sums and one maximum (-1 = nothing yet), and the totals of the sums.
__device__ __forceinline__ void fit_scan(unsigned a, unsigned b, int last, unsigned (*wsum)[4], int* wmax, unsigned& ea, unsigned& eb, int& elast,
                                         unsigned& ta, unsigned& tb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned ia = wave_scan_incl_u32(a), ib = wave_scan_incl_u32(b);
    int im = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(im, o, 64);
        if (lane >= o) im = max(im, u);
    }
    int em = __shfl_up(im, 1, 64);
    if (lane == 0) em = -1;
    __syncthreads();                                           // (the arrays' readers of the call before are done)
    if (lane == 63) { wsum[0][w] = ia; wsum[1][w] = ib; wmax[w] = im; }
    __syncthreads();
    unsigned pa = 0, pb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned sa = wsum[0][k], sb = wsum[1][k];
        if (k < w) { pa += sa; pb += sb; em = max(em, wmax[k]); }
        ta += sa; tb += sb;
    }
    ea = pa + ia - a; eb = pb + ib - b; elast = em;
}

__global__ void __launch_bounds__(FIT_THREADS) k_fit_tree(const FitArgs a) {
    __shared__ unsigned slots32[FIT_MAX_ROWS / 2];
    __shared__ unsigned short perm[FIT_MAX_FEATURES];
    __shared__ FitNode stack[FIT_STACK];
    __shared__ unsigned wsum[2][4];
    __shared__ int wmax[4];
    __shared__ double red_s[4];
    __shared__ int red_q[4];
    __shared__ int win[4];                                     // the winning boundary's right position, left rows, left multiplicities
    __shared__ int part[2];
    unsigned short* slots = reinterpret_cast<unsigned short*>(slots32);

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tree = blockIdx.x, c = tree / a.n_trees, t = tree - c * a.n_trees;
    const int n = a.n, m_c = a.fhead[3 * c], cap = a.fhead[3 * c + 1];
    const size_t out0 = (size_t)a.fhead[3 * c + 2] + (size_t)t * cap;
    const unsigned short* midx = a.midx + (size_t)c * n;
    unsigned* rows_a = a.rows_a + (size_t)tree * a.row_stride;
    unsigned* rows_b = a.rows_b + (size_t)tree * a.row_stride;
    const int chunk = (n + FIT_THREADS - 1) / FIT_THREADS;     // <= 64
    const int p0 = min(n, tid * chunk), p1 = min(n, p0 + chunk);
    const int n_words = (chunk * FIT_THREADS + 1) / 2;         // <= 8192

    unsigned tkey = fit_mix32(a.seed_lo ^ 0x85EBCA6Bu);
    tkey = fit_mix32(tkey + a.seed_hi * 0x9E3779B1u);
    tkey = fit_mix32(tkey + (unsigned)c * 0x85EBCA77u);
    tkey = fit_mix32(tkey + (unsigned)t * 0xC2B2AE3Du);

    // ---- the tree's rows: bootstrap multiplicities in LDS, then the distinct rows in ascending order
    for (int i = tid; i < n_words; i += FIT_THREADS) slots32[i] = 0u;
    __syncthreads();
    if (a.bootstrap) {
        const unsigned bk = fit_mix32(tkey + 0x9E3779B1u);
        for (int j = tid; j < m_c; j += FIT_THREADS) {
            const unsigned r = midx[fit_draw(fit_mix32(bk + (unsigned)j * 0x85EBCA77u), (unsigned)m_c)];
            atomicAdd(&slots32[r >> 1], 1u << (16 * (r & 1u)));          // (a half holds at most m_c <= 16384: no carry)
        }
    } else {
        for (int j = tid; j < m_c; j += FIT_THREADS) slots[midx[j]] = 1;
    }
    __syncthreads();
    {
        unsigned cnt = 0, mm = 0;
        for (int p = p0; p < p1; ++p) {
            const unsigned s = slots[p];
            if (s) { cnt += 1; mm += a.y[p] ? (s << 16) : s; }
        }
        unsigned ec, em, tc, tm;
        int el;
        fit_scan(cnt, mm, -1, wsum, wmax, ec, em, el, tc, tm);
        for (int p = p0; p < p1; ++p) {
            const unsigned s = slots[p];
            if (s) rows_a[ec++] = (unsigned)p | ((unsigned)(a.y[p] ? 1u : 0u) << 14) | (s << 15);
        }
        if (tid == 0) stack[0] = FitNode{0, (int)tc, (int)(tm & 0xFFFFu), (int)(tm >> 16), 0, -1, fit_mix32(tkey + 0x3C6EF362u)};
    }
    __syncthreads();

    // ---- depth first, pre-order.  `top` and `next` are the same in every thread: all control flow below is workgroup-uniform.
    int top = 1, next = 0;
    for (int iter = 0; iter < cap && top > 0; ++iter) {
        const FitNode nd = stack[top - 1];
        __syncthreads();                                       // (everyone has read the entry before it is overwritten)
        --top;
        const int k = next++;
        if (tid == 0 && nd.parent >= 0) a.out_right[out0 + nd.parent] = k;
        const bool stop = nd.depth >= a.max_depth || nd.m < a.min_split || nd.m < 2 * a.min_leaf || nd.m0 == 0 || nd.m1 == 0 || top + 2 > FIT_STACK;
        double best_s = -1.0;
        int best_f = -1, best_q = 0, best_q2 = 0, best_cnt = 0, best_m0 = 0, best_m1 = 0;
        if (!stop) {
            for (int i = tid; i < a.n_features; i += FIT_THREADS) perm[i] = (unsigned short)i;
            __syncthreads();
            if (tid == 0) {
                const unsigned base = nd.key ^ 0x68E31DA4u;
                for (int j = 0; j < a.max_features; ++j) {
                    const int r = j + (int)fit_draw(fit_mix32(base + (unsigned)j * 0x85EBCA77u), (unsigned)(a.n_features - j));
                    const unsigned short u = perm[j];
                    perm[j] = perm[r];
                    perm[r] = u;
                }
            }
            __syncthreads();
            for (int jf = 0; jf < a.max_features; ++jf) {
                const int f = perm[jf];
                const unsigned short* rank = a.rank + (size_t)f * n;
                const float* sval = a.sval + (size_t)f * n;
                for (int i = tid; i < n_words; i += FIT_THREADS) slots32[i] = 0u;
                __syncthreads();
                for (int j = tid; j < nd.m; j += FIT_THREADS) {
                    const unsigned e = rows_a[nd.lo + j];
                    slots[rank[e & 0x3FFFu]] = (unsigned short)(e >> 14);          // class | multiplicity << 1, never 0
                }
                __syncthreads();
                unsigned cnt = 0, mm = 0;
                int last = -1;
                for (int p = p0; p < p1; ++p) {
                    const unsigned s = slots[p];
                    if (s) { cnt += 1; mm += (s & 1u) ? ((s >> 1) << 16) : (s >> 1); last = p; }
                }
                unsigned ec, em, tc, tm;
                int prev;
                fit_scan(cnt, mm, last, wsum, wmax, ec, em, prev, tc, tm);
                // this thread's boundaries: between the occupied position before p and p, the left side's counts being the prefix
                int c0 = (int)(em & 0xFFFFu), c1 = (int)(em >> 16), cl = (int)ec;
                float pv = prev >= 0 ? sval[prev] : 0.0f;
                double my_s = -1.0;
                int my_q = 0x7FFFFFFF, my_q2 = 0, my_cnt = 0, my_m0 = 0, my_m1 = 0;
                for (int p = p0; p < p1; ++p) {
                    const unsigned s = slots[p];
                    if (!s) continue;
                    const float v = sval[p];
                    if (prev >= 0 && pv != v && cl >= a.min_leaf && nd.m - cl >= a.min_leaf) {
                        const double l0 = a.w0 * (double)c0, l1 = a.w1 * (double)c1;
                        const double r0 = a.w0 * (double)(nd.m0 - c0), r1 = a.w1 * (double)(nd.m1 - c1);
                        const double sc = (l0 * l0 + l1 * l1) / (l0 + l1) + (r0 * r0 + r1 * r1) / (r0 + r1);
                        if (sc > my_s) { my_s = sc; my_q = prev; my_q2 = p; my_cnt = cl; my_m0 = c0; my_m1 = c1; }
                    }
                    cl += 1;
                    if (s & 1u) c1 += (int)(s >> 1); else c0 += (int)(s >> 1);
                    prev = p; pv = v;
                }
                // the workgroup's best: larger score, then lower position (positions are distinct, so the winner is one thread)
                double rs = my_s;
                int rq = my_q;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double os = __shfl_xor(rs, o, 64);
                    const int oq = __shfl_xor(rq, o, 64);
                    if (os > rs || (os == rs && oq < rq)) { rs = os; rq = oq; }
                }
                if (lane == 0) { red_s[wv] = rs; red_q[wv] = rq; }
                __syncthreads();
                rs = red_s[0]; rq = red_q[0];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const double os = red_s[w];
                    const int oq = red_q[w];
                    if (os > rs || (os == rs && oq < rq)) { rs = os; rq = oq; }
                }
                const bool better = rs >= 0.0 && rs > best_s;  // (a later feature must be strictly better)
                if (better && my_s >= 0.0 && my_q == rq) { win[0] = my_q2; win[1] = my_cnt; win[2] = my_m0; win[3] = my_m1; }
                __syncthreads();
                if (better) { best_s = rs; best_f = f; best_q = rq; best_q2 = win[0]; best_cnt = win[1]; best_m0 = win[2]; best_m1 = win[3]; }
            }
        }
        if (best_f < 0) {
            if (tid == 0) {
                const double w0m = a.w0 * (double)nd.m0, w1m = a.w1 * (double)nd.m1;
                a.out_feature[out0 + k] = -1;
                a.out_right[out0 + k] = -1;
                a.out_value[out0 + k] = w1m / (w0m + w1m);
            }
            continue;
        }
        const unsigned short* rank = a.rank + (size_t)best_f * n;
        if (tid == 0) {
            const float* sval = a.sval + (size_t)best_f * n;
            a.out_feature[out0 + k] = best_f;
            a.out_right[out0 + k] = -1;                        // set when the right child is reached
            a.out_value[out0 + k] = (double)sval[best_q] / 2.0 + (double)sval[best_q2] / 2.0;
            part[0] = 0; part[1] = 0;
        }
        __syncthreads();
        for (int j = tid; j < nd.m; j += FIT_THREADS) {        // left rows from the span's front, right rows from its back
            const unsigned e = rows_a[nd.lo + j];
            if ((int)rank[e & 0x3FFFu] <= best_q) rows_b[nd.lo + atomicAdd(&part[0], 1)] = e;
            else rows_b[nd.lo + nd.m - 1 - atomicAdd(&part[1], 1)] = e;
        }
        __syncthreads();
        for (int j = tid; j < nd.m; j += FIT_THREADS) rows_a[nd.lo + j] = rows_b[nd.lo + j];
        if (tid == 0) {
            stack[top] = FitNode{nd.lo + best_cnt, nd.m - best_cnt, nd.m0 - best_m0, nd.m1 - best_m1, nd.depth + 1, k, fit_mix32(nd.key + 2u * 0xC2B2AE3Du)};
            stack[top + 1] = FitNode{nd.lo, best_cnt, best_m0, best_m1, nd.depth + 1, -1, fit_mix32(nd.key + 0xC2B2AE3Du)};
        }
        top += 2;
        __syncthreads();
    }
    if (tid == 0) a.out_count[tree] = next;
}

size_t fit_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int64_t rt_forest_fit_capacity(const rt_forest_fit_params* p, int32_t n_members) {
    if (!p || n_members < 1 || p->min_samples_leaf < 1 || p->max_depth < 0) return 0;
    const int64_t by_rows = std::max<int64_t>(1, 2 * (int64_t)(n_members / p->min_samples_leaf) - 1);
    const int64_t by_depth = ((int64_t)1 << (std::min(p->max_depth, 30) + 1)) - 1;
    return std::min(by_rows, by_depth);
}

int rt_forest_fit(rt_ctx* ctx, const double* h_x, int32_t n, int32_t n_features, const uint8_t* h_y, const uint8_t* h_member, int32_t n_forests,
                  const rt_forest_fit_params* p, int32_t node_cap, int32_t* h_tree_first, int32_t* h_node_feature, int32_t* h_node_right,
                  double* h_node_value, int32_t* h_n_nodes) {
    if (!ctx) return RT_ERR_INVALID;
    CtxLock g(ctx);
    if (h_n_nodes) *h_n_nodes = 0;
    if (!h_x || !h_y || !h_member || !p || !h_tree_first || !h_node_feature || !h_node_right || !h_node_value || !h_n_nodes)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: null argument");
    if (n < 1 || n_features < 1 || n_forests < 1 || n_forests > FOREST_MAX_FORESTS)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: n = %d, n_features = %d, n_forests = %d", (int)n, (int)n_features, (int)n_forests);
    if (n > FIT_MAX_ROWS || n_features > FIT_MAX_FEATURES)
        return rt_fail(ctx, RT_ERR_LENGTH, "rt_forest_fit: %d rows of %d features (at most %d rows, %d features)", (int)n, (int)n_features,
                       FIT_MAX_ROWS, FIT_MAX_FEATURES);
    if (p->max_depth > FOREST_MAX_DEPTH)
        return rt_fail(ctx, RT_ERR_LENGTH, "rt_forest_fit: max_depth = %d (at most %d)", (int)p->max_depth, FOREST_MAX_DEPTH);
    int mf = p->max_features;
    if (mf == 0) {
        mf = 1;
        while ((mf + 1) * (mf + 1) <= n_features) ++mf;
    }
    if (p->n_trees < 1 || p->max_depth < 0 || p->min_samples_leaf < 1 || p->min_samples_split < 2 || mf < 1 || mf > n_features ||
        !(p->w0 > 0.0) || !(p->w1 > 0.0) || !std::isfinite(p->w0) || !std::isfinite(p->w1))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: a parameter is out of range");
    for (int i = 0; i < n; ++i)
        if (h_y[i] > 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: y[%d] = %d is neither 0 nor 1", i, (int)h_y[i]);
    if (!forest_features_to_f32(h_x, (int64_t)n * n_features, nullptr))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: a feature is NaN, infinite or beyond float32's range");
    std::vector<int> fhead((size_t)n_forests * 3);
    int64_t total_cap = 0;
    int stride = 0;
    for (int c = 0; c < n_forests; ++c) {
        int m = 0;
        for (int i = 0; i < n; ++i) m += h_member[(size_t)c * n + i] ? 1 : 0;
        if (m == 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_fit: forest %d has no member rows", c);
        const int64_t cap = rt_forest_fit_capacity(p, m);
        fhead[3 * c] = m;
        fhead[3 * c + 1] = (int)cap;
        fhead[3 * c + 2] = (int)total_cap;
        total_cap += cap * p->n_trees;
        stride = std::max(stride, m);
        if (total_cap > 0x7FFFFFFF) return rt_fail(ctx, RT_ERR_LENGTH, "rt_forest_fit: the node capacity of the call exceeds 2^31 - 1");
    }
    const int64_t n_total_trees = (int64_t)n_forests * p->n_trees;
    if (n_total_trees > 0x7FFFFFFF / 4) return rt_fail(ctx, RT_ERR_LENGTH, "rt_forest_fit: %lld trees", (long long)n_total_trees);
    if ((int64_t)node_cap < total_cap)
        return rt_fail(ctx, RT_ERR_LENGTH, "rt_forest_fit: node_cap = %d, the capacity bound of this call is %lld nodes", (int)node_cap,
                       (long long)total_cap);

    // one input block, one output block: a copy each
    const size_t nf = (size_t)n_features, nn = (size_t)n, trees = (size_t)n_total_trees;
    const size_t in_x = 0, in_y = fit_up(in_x + nf * nn * 4), in_m = fit_up(in_y + nn), in_h = fit_up(in_m + (size_t)n_forests * nn * 2);
    const size_t in_bytes = fit_up(in_h + fhead.size() * 4);
    const size_t o_val = 0, o_feat = fit_up(o_val + (size_t)total_cap * 8), o_right = fit_up(o_feat + (size_t)total_cap * 4);
    const size_t o_cnt = fit_up(o_right + (size_t)total_cap * 4), out_bytes = fit_up(o_cnt + trees * 4);
    const size_t d_rank = in_bytes, d_sval = fit_up(d_rank + nf * nn * 2), d_ra = fit_up(d_sval + nf * nn * 4);
    const size_t d_rb = fit_up(d_ra + trees * (size_t)stride * 4), d_out = fit_up(d_rb + trees * (size_t)stride * 4), d_bytes = d_out + out_bytes;

    RT_HIP(ctx, hipSetDevice(ctx->device));
    void *hp = nullptr, *dp = nullptr;
    RT_TRY(rt_ctx_pinned(ctx, in_bytes + out_bytes, &hp));
    RT_TRY(rt_ctx_scratch(ctx, d_bytes, &dp));
    char *h = (char*)hp, *d = (char*)dp;
    float* hx = (float*)(h + in_x);
    for (size_t i = 0; i < nn; ++i)
        for (size_t f = 0; f < nf; ++f) hx[f * nn + i] = (float)h_x[i * nf + f];
    std::memcpy(h + in_y, h_y, nn);
    unsigned short* hm = (unsigned short*)(h + in_m);
    for (int c = 0; c < n_forests; ++c) {
        size_t k = 0;
        for (size_t i = 0; i < nn; ++i)
            if (h_member[(size_t)c * nn + i]) hm[(size_t)c * nn + k++] = (unsigned short)i;
        for (; k < nn; ++k) hm[(size_t)c * nn + k] = 0;
    }
    std::memcpy(h + in_h, fhead.data(), fhead.size() * 4);
    RT_HIP(ctx, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));

    FitArgs a;
    a.sval = (const float*)(d + d_sval);
    a.rank = (const unsigned short*)(d + d_rank);
    a.y = (const unsigned char*)(d + in_y);
    a.midx = (const unsigned short*)(d + in_m);
    a.fhead = (const int*)(d + in_h);
    a.rows_a = (unsigned*)(d + d_ra);
    a.rows_b = (unsigned*)(d + d_rb);
    a.out_value = (double*)(d + d_out + o_val);
    a.out_feature = (int*)(d + d_out + o_feat);
    a.out_right = (int*)(d + d_out + o_right);
    a.out_count = (int*)(d + d_out + o_cnt);
    a.n = n; a.n_features = n_features; a.n_trees = p->n_trees; a.max_depth = p->max_depth; a.min_leaf = p->min_samples_leaf;
    a.min_split = p->min_samples_split; a.max_features = mf; a.bootstrap = p->bootstrap ? 1 : 0; a.row_stride = stride;
    a.w0 = p->w0; a.w1 = p->w1;
    a.seed_lo = (unsigned)(p->seed & 0xFFFFFFFFull); a.seed_hi = (unsigned)(p->seed >> 32);
    hipLaunchKernelGGL(k_fit_rank, dim3((unsigned)((n + FIT_THREADS - 1) / FIT_THREADS), (unsigned)n_features), dim3(FIT_THREADS), 0, ctx->stream,
                       (const float*)(d + in_x), (int)n, (unsigned short*)(d + d_rank), (float*)(d + d_sval));
    hipLaunchKernelGGL(k_fit_tree, dim3((unsigned)n_total_trees), dim3(FIT_THREADS), 0, ctx->stream, a);
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(h + in_bytes, d + d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // the trees one behind the other in table layout (right children count through the whole call)
    const double* ov = (const double*)(h + in_bytes + o_val);
    const int *of = (const int*)(h + in_bytes + o_feat), *orr = (const int*)(h + in_bytes + o_right), *oc = (const int*)(h + in_bytes + o_cnt);
    int64_t at = 0;
    h_tree_first[0] = 0;
    for (int c = 0; c < n_forests; ++c)
        for (int t = 0; t < p->n_trees; ++t) {
            const size_t tr = (size_t)c * p->n_trees + t, src = (size_t)fhead[3 * c + 2] + (size_t)t * fhead[3 * c + 1];
            const int cnt = oc[tr];
            if (cnt < 1 || cnt > fhead[3 * c + 1] || at + cnt > node_cap)
                return rt_fail(ctx, RT_ERR_STATE, "rt_forest_fit: tree %d of forest %d came back with %d nodes (capacity %d)", t, c, cnt, fhead[3 * c + 1]);
            for (int k = 0; k < cnt; ++k) {
                h_node_feature[at + k] = of[src + k];
                h_node_right[at + k] = orr[src + k] < 0 ? -1 : (int32_t)(at + orr[src + k]);
                h_node_value[at + k] = ov[src + k];
            }
            at += cnt;
            h_tree_first[tr + 1] = (int32_t)at;
        }
    *h_n_nodes = (int32_t)at;
    return RT_OK;
}

}  // extern "C"
