// The row plan of a generation whose items speak with different voices.  Pure host arithmetic (no HIP): generate.hip runs it,
// rt_debug_voice_row_plan answers from it without a GPU (tests/test_voice_bank_cpu.py).
//
// The decode step's matrix-core attention gives one workgroup FOUR consecutive rows that share the prefix tiles
// (attention_mfma.hip), so the rows are cut into 4-row blocks and a block holds rows of one voice only:
//   an item takes the lowest free row of a block of its voice,
//   else the first row of the lowest block whose rows are all free - that block is re-voiced,
//   else it waits, and so does every later item of its voice (array order is kept within a voice; another voice may pass).
// The first wave is the same rule on empty rows.  With one distinct voice this is the layout a run had before there was a bank: item b
// on row b, min(n_items, max_rows) rows, and at a hand-over the next items in array order on the free rows in row order.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace voice_plan {

constexpr int BLOCK = 4;

struct State {
    int rows = 0;                     // decode rows of the run
    std::vector<int> row_item;        // [rows] item on the row, -1: free
    std::vector<int> block_voice;     // [ceil(rows / 4)] voice of the block's rows, -1: none yet
    std::vector<char> placed;         // [n_items] the item has (had) a row
    int n_blocks() const { return (rows + BLOCK - 1) / BLOCK; }
};

// waiting items -> rows.  Appends (item, row) pairs in array order; *revoiced counts blocks that changed from one voice to another.
inline int place(const int32_t* voice, int n_items, State& s, std::vector<int>* items, std::vector<int>* rows, int* revoiced = nullptr) {
    int n_placed = 0;
    std::vector<int32_t> stuck;       // voices with an item that found no row in this pass
    for (int it = 0; it < n_items; ++it) {
        if (s.placed[it]) continue;
        const int32_t v = voice[it];
        if (std::find(stuck.begin(), stuck.end(), v) != stuck.end()) continue;
        int row = -1;
        for (int r = 0; r < s.rows && row < 0; ++r)
            if (s.row_item[r] < 0 && s.block_voice[r / BLOCK] == v) row = r;
        for (int b = 0; b < s.n_blocks() && row < 0; ++b) {
            bool all_free = true;
            for (int r = b * BLOCK; r < std::min(s.rows, (b + 1) * BLOCK); ++r) all_free = all_free && s.row_item[r] < 0;
            if (!all_free) continue;
            if (revoiced && s.block_voice[b] >= 0 && s.block_voice[b] != v) ++*revoiced;
            s.block_voice[b] = v;
            row = b * BLOCK;
        }
        if (row < 0) { stuck.push_back(v); continue; }
        s.row_item[row] = it;
        s.placed[it] = 1;
        if (items) items->push_back(it);
        if (rows) rows->push_back(row);
        ++n_placed;
    }
    return n_placed;
}

// the first wave on at most max_rows rows; sets s.rows: every row up to max_rows while items wait (a later hand-over may need
// them), else up to the last row that got an item
inline int start(const int32_t* voice, int n_items, int max_rows, State& s, std::vector<int>* items, std::vector<int>* rows) {
    s.rows = max_rows;
    s.row_item.assign(max_rows, -1);
    s.block_voice.assign(s.n_blocks(), -1);
    s.placed.assign(n_items, 0);
    const int n_placed = place(voice, n_items, s, items, rows);
    if (n_placed == n_items) {
        int last = 0;
        for (int r = 0; r < max_rows; ++r) if (s.row_item[r] >= 0) last = r;
        s.rows = last + 1;
        s.row_item.resize(s.rows);
        s.block_voice.resize(s.n_blocks());
    }
    return n_placed;
}

}  // namespace voice_plan
