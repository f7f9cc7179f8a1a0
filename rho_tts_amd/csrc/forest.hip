// The accent-drift classifier on the GPU: random-forest inference with isotonic calibration from exported tables (SURVEY.md 8f-3,
// the classifier half).  Stands behind validation/classifier/__init__.py:115-118 - `model.predict_proba(x)[0][1]` of a
// CalibratedClassifierCV(RandomForestClassifier(200 trees, depth 10), isotonic, cv = 5) - for a whole chunk of feature rows in one call.
// rho_tts_amd/forest.py documents the table format and holds the definition, predict_host; the two kernels here do its steps in its
// order, so that a row's probability is the host's bit for bit and depends on nothing else in the call:
//
//   k_forest_walk    one thread per (row, tree): from the tree's root, `(double)float32 feature <= threshold` goes left (node + 1), else to
//                    the stored right child - the feature and both 16-byte children are loaded together, so a level is ONE dependent
//                    round trip - for at most max_depth levels (the depth the host check computed, not "until a leaf"); the reached
//                    leaf's class-1 fraction goes to leaf[row][tree]
//   k_forest_finish  one wave per row: lane c sums forest c's leaf fractions one after the other in tree order (staged through LDS in
//                    coalesced pieces), divides by the tree count, clips to the calibrator's knots and interpolates with np.interp's
//                    arithmetic; lane 0 sums the calibrated values in order and divides by their count
//
// No floating-point atomics, no grid-wide barrier; built with -ffp-contract=off (the interpolation's multiply and add round separately,
// as numpy's do).  rt_forest_predict is one host-to-device copy, two launches, one device-to-host copy and one stream synchronisation.
#include <algorithm>
#include <vector>

#include "forest_check.h"
#include "kernels.h"

struct alignas(16) forest_node {
    double value;        // threshold of a split node / class-1 fraction of a leaf
    int32_t feature;     // -1 = leaf
    int32_t right;       // right child (the left one is the next node)
};
static_assert(sizeof(forest_node) == 16, "one 16-byte load per level");

struct rt_forest {
    rt_ctx* ctx = nullptr;
    bool set = false;
    int n_features = 0, n_forests = 0, n_trees = 0, n_nodes = 0, n_cal = 0, max_depth = 0;
    forest_node* d_nodes = nullptr;
    int *d_tree_first = nullptr, *d_forest_first = nullptr, *d_iso_first = nullptr;
    double *d_iso_x = nullptr, *d_iso_y = nullptr;
    // workspaces, grown on demand and kept: a steady-state call allocates nothing
    float* h_x = nullptr;                          // pinned: the features as float32
    float* d_x = nullptr;                          // [rows][n_features]
    double *d_leaf = nullptr, *d_prob = nullptr;   // [rows][n_trees], [rows]
    size_t h_x_cap = 0, d_x_cap = 0, leaf_cap = 0, prob_cap = 0;
};

namespace {

constexpr int FINISH_CHUNK = 1024;

__global__ void __launch_bounds__(256) k_forest_walk(const forest_node* __restrict__ nodes, const int* __restrict__ tree_first,
                                                     const float* __restrict__ x, int n_features, int n_trees, long long n_pairs, int max_depth,
                                                     double* __restrict__ leaf) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (long long)gridDim.x * 256) {
        const long long row = i / n_trees;
        const int tree = (int)(i - row * n_trees);
        const float* xr = x + row * n_features;
        int k = tree_first[tree];
        forest_node nd = nodes[k];
        for (int d = 0; d < max_depth && nd.feature >= 0; ++d) {
            // both children (checked indices) are fetched beside the feature: one dependent round trip per level, not two
            const forest_node lc = nodes[k + 1], rc = nodes[nd.right];
            const bool left = (double)xr[nd.feature] <= nd.value;
            k = left ? k + 1 : nd.right;
            nd = left ? lc : rc;
        }
        leaf[i] = nd.feature < 0 ? nd.value : __builtin_nan("");      // (a checked model always ends on a leaf)
    }
}

__global__ void __launch_bounds__(64) k_forest_finish(const double* __restrict__ leaf, const int* __restrict__ forest_first, int n_forests, int n_trees,
                                                      const int* __restrict__ iso_first, const double* __restrict__ iso_x,
                                                      const double* __restrict__ iso_y, int n_cal, double* __restrict__ prob) {
    __shared__ double chunk[FINISH_CHUNK];
    __shared__ double cal[FOREST_MAX_FORESTS];
    const int lane = threadIdx.x;
    const double* lr = leaf + (long long)blockIdx.x * n_trees;
    int t0 = 0, t1 = 0;
    if (lane < n_forests) { t0 = forest_first[lane]; t1 = forest_first[lane + 1]; }
    double s = 0.0;
    for (int base = 0; base < n_trees; base += FINISH_CHUNK) {
        const int m = min(FINISH_CHUNK, n_trees - base);
        for (int j = lane; j < m; j += 64) chunk[j] = lr[base + j];
        __syncthreads();
        const int a = max(t0, base) - base, b = min(t1, base + m) - base;
#pragma unroll 8
        for (int j = a; j < b; ++j) s = s + chunk[j];      // (in order; unrolled so that the LDS reads run ahead of the adds)
        __syncthreads();
    }
    if (lane < n_forests) {
        double p = s / (double)(t1 - t0);
        if (n_cal > 0) {
            const int k0 = iso_first[lane], nk = iso_first[lane + 1] - k0;
            const double *kx = iso_x + k0, *ky = iso_y + k0;
            if (nk == 1) {
                p = ky[0];
            } else {
                const double lo_x = kx[0], hi_x = kx[nk - 1];
                double v = p < lo_x ? lo_x : p;
                v = v > hi_x ? hi_x : v;
                int lo = 0, hi = nk - 1;                                   // the last knot at or below v
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (kx[mid] <= v) lo = mid; else hi = mid - 1;
                }
                if (lo >= nk - 1) {
                    p = ky[nk - 1];
                } else if (kx[lo] == v) {
                    p = ky[lo];
                } else {
                    const double slope = (ky[lo + 1] - ky[lo]) / (kx[lo + 1] - kx[lo]);
                    const double d = v - kx[lo];
                    const double md = slope * d;
                    p = md + ky[lo];
                }
            }
        }
        cal[lane] = p;
    }
    __syncthreads();
    if (lane == 0) {
        if (n_cal == 0) {
            prob[blockIdx.x] = cal[0];
        } else {
            double acc = 0.0;
            for (int c = 0; c < n_cal; ++c) acc = acc + cal[c];
            prob[blockIdx.x] = acc / (double)n_cal;
        }
    }
}

template <class T>
int forest_grow(rt_ctx* ctx, T*& p, size_t& cap, size_t need) {
    if (need <= cap && p) return RT_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    RT_HIP(ctx, hipMalloc((void**)&p, std::max<size_t>(need, 1) * sizeof(T)));
    cap = need;
    return RT_OK;
}

template <class T>
int forest_upload(rt_ctx* ctx, T*& d, const T* h, size_t n) {
    RT_HIP(ctx, hipMalloc((void**)&d, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) RT_HIP(ctx, hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

void forest_free_model(rt_forest* f) {
    for (void* p : {(void*)f->d_nodes, (void*)f->d_tree_first, (void*)f->d_forest_first, (void*)f->d_iso_first, (void*)f->d_iso_x, (void*)f->d_iso_y})
        if (p) (void)hipFree(p);
    f->d_nodes = nullptr;
    f->d_tree_first = f->d_forest_first = f->d_iso_first = nullptr;
    f->d_iso_x = f->d_iso_y = nullptr;
    f->set = false;
}

}  // namespace

extern "C" {

int rt_forest_create(rt_ctx* ctx, rt_forest** out) {
    if (!ctx || !out) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_create: null argument");
    *out = nullptr;
    CtxLock g(ctx);
    rt_forest* f = new rt_forest();
    f->ctx = ctx;
    *out = f;
    return RT_OK;
}

int rt_forest_destroy(rt_forest* f) {
    if (!f) return RT_OK;
    rt_ctx* ctx = f->ctx;
    CtxLock g(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    forest_free_model(f);
    for (void* p : {(void*)f->d_x, (void*)f->d_leaf, (void*)f->d_prob})
        if (p) (void)hipFree(p);
    if (f->h_x) (void)hipHostFree(f->h_x);
    delete f;
    return RT_OK;
}

int rt_forest_set_model(rt_forest* f, int32_t n_features, int32_t n_forests, const int32_t* h_forest_first, int32_t n_trees,
                        const int32_t* h_tree_first, int32_t n_nodes, const int32_t* h_node_feature, const int32_t* h_node_right,
                        const double* h_node_value, int32_t n_calibrators, const int32_t* h_iso_first, const double* h_iso_x, const double* h_iso_y) {
    if (!f) return RT_ERR_INVALID;
    rt_ctx* ctx = f->ctx;
    CtxLock g(ctx);
    forest_tables t;
    t.n_features = n_features;
    t.n_forests = n_forests;       t.forest_first = h_forest_first;
    t.n_trees = n_trees;           t.tree_first = h_tree_first;
    t.n_nodes = n_nodes;           t.node_feature = h_node_feature; t.node_right = h_node_right; t.node_value = h_node_value;
    t.n_calibrators = n_calibrators; t.iso_first = h_iso_first;     t.iso_x = h_iso_x;           t.iso_y = h_iso_y;
    int depth = 0;
    if (const char* why = forest_check(t, &depth)) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_set_model: %s", why);   // nothing uploaded
    std::vector<forest_node> nodes((size_t)n_nodes);
    for (int k = 0; k < n_nodes; ++k) nodes[(size_t)k] = forest_node{h_node_value[k], h_node_feature[k], h_node_right[k]};
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    forest_free_model(f);                                  // (a failed upload leaves the handle without a model)
    const size_t n_knots = (size_t)h_iso_first[n_calibrators];
    RT_TRY(forest_upload(ctx, f->d_nodes, nodes.data(), nodes.size()));
    RT_TRY(forest_upload(ctx, f->d_tree_first, h_tree_first, (size_t)n_trees + 1));
    RT_TRY(forest_upload(ctx, f->d_forest_first, h_forest_first, (size_t)n_forests + 1));
    RT_TRY(forest_upload(ctx, f->d_iso_first, h_iso_first, (size_t)n_calibrators + 1));
    RT_TRY(forest_upload(ctx, f->d_iso_x, h_iso_x, n_knots));
    RT_TRY(forest_upload(ctx, f->d_iso_y, h_iso_y, n_knots));
    f->n_features = n_features; f->n_forests = n_forests; f->n_trees = n_trees; f->n_nodes = n_nodes; f->n_cal = n_calibrators;
    f->max_depth = depth;
    f->set = true;
    return RT_OK;
}

int rt_forest_predict(rt_forest* f, const double* h_x, int32_t n_rows, double* h_prob) {
    if (!f) return RT_ERR_INVALID;
    rt_ctx* ctx = f->ctx;
    CtxLock g(ctx);
    if (!f->set) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_predict: no model set");
    if (n_rows < 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_predict: n_rows = %d", (int)n_rows);
    if (n_rows == 0) return RT_OK;
    if (!h_x || !h_prob) return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_predict: null argument");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_el = (size_t)n_rows * (size_t)f->n_features;
    const long long n_pairs = (long long)n_rows * f->n_trees;
    if (n_el > f->h_x_cap || !f->h_x) {
        if (f->h_x) (void)hipHostFree(f->h_x);
        f->h_x = nullptr; f->h_x_cap = 0;
        RT_HIP(ctx, hipHostMalloc((void**)&f->h_x, n_el * sizeof(float), hipHostMallocDefault));
        f->h_x_cap = n_el;
    }
    if (!forest_features_to_f32(h_x, (int64_t)n_el, f->h_x))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_forest_predict: a feature is NaN, infinite or beyond float32's range");   // before any launch
    RT_TRY(forest_grow(ctx, f->d_x, f->d_x_cap, n_el));
    RT_TRY(forest_grow(ctx, f->d_leaf, f->leaf_cap, (size_t)n_pairs));
    RT_TRY(forest_grow(ctx, f->d_prob, f->prob_cap, (size_t)n_rows));
    RT_HIP(ctx, hipMemcpyAsync(f->d_x, f->h_x, n_el * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned)std::min<long long>((n_pairs + 255) / 256, 4096);
    hipLaunchKernelGGL(k_forest_walk, dim3(blocks), dim3(256), 0, ctx->stream, f->d_nodes, f->d_tree_first, f->d_x, f->n_features, f->n_trees, n_pairs,
                       f->max_depth, f->d_leaf);
    hipLaunchKernelGGL(k_forest_finish, dim3((unsigned)n_rows), dim3(64), 0, ctx->stream, f->d_leaf, f->d_forest_first, f->n_forests, f->n_trees,
                       f->d_iso_first, f->d_iso_x, f->d_iso_y, f->n_cal, f->d_prob);
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(h_prob, f->d_prob, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
