// The host-side check of a drift classifier's tables (rho_tts_amd/forest.py documents the format): what rt_forest_set_model
// runs before anything is uploaded, restating in C the index and range conditions of forest.validate - they are what keeps the
// walk kernel inside its arrays and every walk finite.  Plain C++ without HIP, so that it also builds into a stand-alone host
// program (tools/forest_check_main.cpp, the sanitizer run).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

constexpr int FOREST_MAX_DEPTH = 64;      // edges from a root to its deepest leaf
constexpr int FOREST_MAX_FORESTS = 64;    // one lane of the finishing wave per forest

struct forest_tables {
    int32_t n_features = 0;
    int32_t n_forests = 0;
    const int32_t* forest_first = nullptr;    // [n_forests + 1] tree ranges
    int32_t n_trees = 0;
    const int32_t* tree_first = nullptr;      // [n_trees + 1] node ranges
    int32_t n_nodes = 0;
    const int32_t* node_feature = nullptr;    // [n_nodes] split feature, -1 = leaf
    const int32_t* node_right = nullptr;      // [n_nodes] right child (the left one is k + 1), -1 for a leaf
    const double* node_value = nullptr;       // [n_nodes] threshold / class-1 fraction of a leaf
    int32_t n_calibrators = 0;
    const int32_t* iso_first = nullptr;       // [n_calibrators + 1] knot ranges
    const double* iso_x = nullptr;
    const double* iso_y = nullptr;
};

// nullptr when the tables are sound (and *max_depth = edges to the deepest reachable node), else what is wrong.
inline const char* forest_check(const forest_tables& t, int* max_depth) {
    if (t.n_features < 1) return "n_features below 1";
    if (t.n_forests < 1 || t.n_forests > FOREST_MAX_FORESTS) return "forest count outside 1 .. 64";
    if (t.n_trees < t.n_forests || t.n_nodes < t.n_trees) return "fewer trees than forests or fewer nodes than trees";
    if (!t.forest_first || !t.tree_first || !t.node_feature || !t.node_right || !t.node_value || !t.iso_first) return "null table pointer";
    if (t.forest_first[0] != 0 || t.forest_first[t.n_forests] != t.n_trees) return "forest ranges do not cover the trees";
    for (int c = 0; c < t.n_forests; ++c)
        if (t.forest_first[c + 1] <= t.forest_first[c]) return "an empty or descending forest range";
    if (t.tree_first[0] != 0 || t.tree_first[t.n_trees] != t.n_nodes) return "tree ranges do not cover the nodes";
    for (int r = 0; r < t.n_trees; ++r)
        if (t.tree_first[r + 1] <= t.tree_first[r]) return "an empty or descending tree range";
    // children lie behind their parent and inside its tree: one ascending pass gives every node's depth
    std::vector<int> depth((size_t)t.n_nodes, 0);
    int deepest = 0;
    for (int r = 0; r < t.n_trees; ++r) {
        const int end = t.tree_first[r + 1];
        for (int k = t.tree_first[r]; k < end; ++k) {
            const int f = t.node_feature[k];
            const double v = t.node_value[k];
            if (!std::isfinite(v)) return "a threshold or leaf value that is not finite";
            if (f < 0) {
                if (f != -1 || t.node_right[k] != -1) return "a leaf with a child or a feature below -1";
                if (v < 0.0 || v > 1.0) return "a leaf value outside [0, 1]";
                continue;
            }
            if (f >= t.n_features) return "a split feature not below n_features";
            const int right = t.node_right[k];
            if (right <= k) return "a child index not greater than its parent's";
            if (right >= end) return "a child index outside its tree";          // (then k + 1 < end too)
            const int d = depth[(size_t)k] + 1;
            if (d > FOREST_MAX_DEPTH) return "a tree deeper than 64";
            if (d > depth[(size_t)k + 1]) depth[(size_t)k + 1] = d;
            if (d > depth[(size_t)right]) depth[(size_t)right] = d;
            if (d > deepest) deepest = d;
        }
    }
    if (t.n_calibrators != 0 && t.n_calibrators != t.n_forests) return "calibrator count is neither 0 nor the forest count";
    if (t.n_calibrators == 0 && t.n_forests != 1) return "several forests without calibrators";
    if (t.iso_first[0] != 0) return "calibrator ranges do not start at 0";
    if (t.n_calibrators > 0 && (!t.iso_x || !t.iso_y)) return "null calibrator pointer";
    for (int c = 0; c < t.n_calibrators; ++c) {
        const int a = t.iso_first[c], b = t.iso_first[c + 1];
        if (b <= a) return "an empty calibrator";
        for (int j = a; j < b; ++j) {
            if (!std::isfinite(t.iso_x[j]) || !std::isfinite(t.iso_y[j])) return "a calibrator knot that is not finite";
            if (j > a && !(t.iso_x[j] > t.iso_x[j - 1])) return "calibrator knots that do not increase strictly";
        }
    }
    if (max_depth) *max_depth = deepest;
    return nullptr;
}

// Features as the trees see them: float32.  false when one is NaN, infinite or beyond float32's range (scikit-learn raises for the
// same inputs); `out` may be null (check only).
inline bool forest_features_to_f32(const double* x, int64_t n, float* out) {
    bool ok = true;
    for (int64_t i = 0; i < n; ++i) {
        const bool fits = std::fabs(x[i]) < 0x1.ffffffp+127;      // below FLT_MAX + half an ulp: rounds to a finite float (NaN: false)
        ok &= fits;
        if (out) out[i] = fits ? (float)x[i] : 0.0f;
    }
    return ok;
}
