// Stand-alone host program around csrc/forest_check.h, the check rt_forest_set_model runs before it uploads a drift classifier: feeds it
// a sound model and the malformed tables of tests/forest_cases.py and expects each verdict.  It exists to be built with the host
// sanitizers (no GPU, no HIP, nothing loaded into python):
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/forest_check_main.cpp -o forest_check && ./forest_check
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../rho_tts_amd/csrc/forest_check.h"

struct Model {
    int n_features = 1;
    std::vector<int32_t> forest_first{0}, tree_first{0}, feature, right, iso_first{0};
    std::vector<double> value, iso_x, iso_y;
    void tree(const std::vector<int>& f, const std::vector<double>& v, const std::vector<int>& r) {
        const int base = tree_first.back();
        for (size_t i = 0; i < f.size(); ++i) { feature.push_back(f[i]); value.push_back(v[i]); right.push_back(r[i] >= 0 ? r[i] + base : -1); }
        tree_first.push_back(base + (int)f.size());
    }
    void end_forest() { forest_first.push_back((int)tree_first.size() - 1); }
    void calibrator(const std::vector<double>& x, const std::vector<double>& y) {
        iso_x.insert(iso_x.end(), x.begin(), x.end()); iso_y.insert(iso_y.end(), y.begin(), y.end());
        iso_first.push_back((int)iso_x.size());
    }
    void chain(int depth) {
        std::vector<int> f, r; std::vector<double> v;
        for (int i = 0; i < depth; ++i) { f.push_back(0); v.push_back(i); r.push_back(2 * i + 2); f.push_back(-1); v.push_back(i / 100.0); r.push_back(-1); }
        f.push_back(-1); v.push_back(0.99); r.push_back(-1);
        tree(f, v, r);
    }
    forest_tables view() const {
        forest_tables t;
        t.n_features = n_features;
        t.n_forests = (int)forest_first.size() - 1; t.forest_first = forest_first.data();
        t.n_trees = (int)tree_first.size() - 1;     t.tree_first = tree_first.data();
        t.n_nodes = (int)feature.size();            t.node_feature = feature.data(); t.node_right = right.data(); t.node_value = value.data();
        t.n_calibrators = (int)iso_first.size() - 1; t.iso_first = iso_first.data(); t.iso_x = iso_x.data(); t.iso_y = iso_y.data();
        return t;
    }
};

static Model base() {      // two ladder trees in one forest, one calibrator (tests/forest_cases.py malformed())
    Model m;
    for (int k = 0; k < 2; ++k) m.tree({0, -1, 0, -1, 0, -1, -1}, {1.0, 0.05, 2.0, 0.3, 3.0, 0.5, 0.95}, {2, -1, 4, -1, 6, -1, -1});
    m.end_forest();
    m.calibrator({0.1, 0.3, 0.7, 0.9}, {0.0, 0.2, 0.6, 1.0});
    return m;
}

static int failures = 0;
static void expect(const char* what, const Model& m, const char* fragment, int want_depth = -1) {
    int depth = -1;
    const char* why = forest_check(m.view(), &depth);
    const bool ok = fragment ? (why && std::strstr(why, fragment)) : (!why && (want_depth < 0 || depth == want_depth));
    std::printf("%-32s %s  (%s%s)\n", what, ok ? "ok" : "WRONG", why ? why : "accepted, depth ", why ? "" : std::to_string(depth).c_str());
    failures += !ok;
}

int main() {
    expect("the sound model", base(), nullptr, 3);
    { Model m; m.chain(64); m.end_forest(); expect("a chain of depth 64", m, nullptr, 64); }
    { Model m = base(); m.right[2] = 2; expect("a child index <= its parent", m, "not greater than its parent"); }
    { Model m = base(); m.right[0] = 8; expect("a child outside its tree", m, "outside its tree"); }
    { Model m = base(); m.right[7] = 1 << 30; expect("a child far outside the arrays", m, "outside its tree"); }
    { Model m = base(); m.feature[0] = 1; expect("feature >= n_features", m, "below n_features"); }
    { Model m = base(); m.value[0] = std::numeric_limits<double>::quiet_NaN(); expect("a NaN threshold", m, "not finite"); }
    { Model m = base(); m.value[1] = 1.5; expect("a leaf value of 1.5", m, "outside [0, 1]"); }
    { Model m = base(); m.iso_x[2] = 0.3; expect("non-increasing iso_x", m, "increase strictly"); }
    { Model m = base(); m.iso_first = {0, 0}; m.iso_x.clear(); m.iso_y.clear(); expect("an empty calibrator", m, "empty calibrator"); }
    { Model m; m.chain(65); m.end_forest(); expect("depth 65", m, "deeper than 64"); }
    { Model m = base(); m.tree_first = {0, 7, 7}; expect("an empty tree range", m, "tree range"); }
    { Model m = base(); m.forest_first = {0, 3}; expect("a forest range past the trees", m, "forest ranges"); }
    { Model m = base(); m.feature[13] = 0; m.right[13] = 14; expect("a split as the last node", m, "outside its tree"); }
    const double inf = std::numeric_limits<double>::infinity();
    const double fine[4] = {0.0, -3.4e38, 3.4028235e38, 1e-300}, bad[4][1] = {{inf}, {-inf}, {std::numeric_limits<double>::quiet_NaN()}, {3.5e38}};
    float out[4];
    bool conv = forest_features_to_f32(fine, 4, out) && out[1] == -3.4e38f && out[3] == 0.0f;
    for (auto& b : bad) conv = conv && !forest_features_to_f32(b, 1, out) && !forest_features_to_f32(b, 1, nullptr);
    std::printf("%-32s %s\n", "features to float32", conv ? "ok" : "WRONG");
    failures += !conv;
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
