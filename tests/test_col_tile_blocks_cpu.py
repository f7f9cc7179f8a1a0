"""The tile-block rule of the column-owner decode GEMM's launcher (gemm_col.hip col_tile_blocks) as host arithmetic:
rt_debug_col_tile_blocks touches no GPU.  Checked at n_cu = 256 (MI355X) on the decode projections of the 1.7B preset.  STORE
launches take the form as RESID launches do (the predictor's head gained per launch: profiles/r25_tile_blocks.txt)."""
import os
import re

import pytest

from rho_tts_amd import _native

STORE, RESID, SILU = 0, 1, 2
N_CU = 256
# (N, epi, name): 128 tiles x split 2 = 256 half-tile workgroups
WINDOW = [(2048, RESID, "talker o"), (2048, RESID, "talker down"), (2048, STORE, "pred head")]
OUTSIDE = [(1024, RESID, "pred o / down: the row-block rule's"), (1024, STORE, "mtp projection: the row-block rule's"), (4096, STORE, "qkv: split 1"),
           (3072, STORE, "talker head: split 1"), (12288, SILU, "talker gate/up"), (6144, SILU, "pred gate/up")]


def shipped(base, name):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rho_tts_amd", "csrc", "knobs.h")).read()
    return base + int(re.search(r"X\(%d, %s, (\d+)," % (base, name), src).group(1))


@pytest.fixture()
def lib():
    lib = _native.load_library()
    yield lib
    for code in (shipped(3600, "g_col_row_blocks"), shipped(3700, "g_col_tile_blocks"), 500):        # later tests see the shipped plan
        assert lib.rt_debug_tune(code, 0) == 0


def rows(lib, M, N, epi, split=0, n_cu=N_CU):
    return lib.rt_debug_col_tile_blocks(n_cu, M, N, epi, split)


def test_the_window_gets_whole_tiles_and_two_row_blocks(lib):
    assert lib.rt_debug_tune(3702, 0) == 0
    for N, epi, name in WINDOW:
        assert rows(lib, 17, N, epi) == 16 and rows(lib, 32, N, epi) == 16, name
        assert rows(lib, 33, N, epi) == 32 and rows(lib, 64, N, epi) == 32, name
    for N in (1040, 1552, 2047):                                                    # 65, 97 and 128 tiles
        assert rows(lib, 32, N, RESID) == 16 and rows(lib, 64, N, STORE) == 32, N


def test_launches_outside_the_window_get_none(lib):
    assert lib.rt_debug_tune(3702, 0) == 0
    for N, epi, name in OUTSIDE:
        for M in (17, 32, 33, 64):
            assert rows(lib, M, N, epi) == 0, (name, M)
    assert rows(lib, 32, 1024, RESID) == 0 and rows(lib, 32, 2064, RESID) == 0       # 64 tiles: round 24's; 129 tiles: split 1


def test_sixteen_rows_and_fewer_and_sixty_five_and_more_get_none(lib):
    assert lib.rt_debug_tune(3702, 0) == 0
    for N, epi, name in WINDOW + OUTSIDE:
        for M in (1, 16, 65, 128):
            assert rows(lib, M, N, epi) == 0, (name, M)


def test_the_switch_changes_the_answers_as_documented(lib):
    want = {0: {17: 0, 32: 0, 33: 0, 64: 0}, 1: {17: 0, 32: 0, 33: 32, 64: 32}, 2: {17: 16, 32: 16, 33: 32, 64: 32}}
    for N, epi, name in WINDOW:
        for value in (0, 1, 2):
            assert lib.rt_debug_tune(3700 + value, 0) == 0
            for M, r in want[value].items():
                assert rows(lib, M, N, epi) == r, (name, value, M)


def test_only_split_two_takes_the_form(lib):
    """Forced splits 1 and 4 (as the argument, or process-wide through 501 / 504) get none; a forced 2 is what N = 2048 resolves to."""
    assert lib.rt_debug_tune(3702, 0) == 0
    for M, r in ((32, 16), (64, 32)):
        assert rows(lib, M, 2048, RESID, 1) == 0 and rows(lib, M, 2048, RESID, 4) == 0 and rows(lib, M, 2048, RESID, 2) == r
    for code, r in ((501, 0), (504, 0), (502, 16), (500, 16)):
        assert lib.rt_debug_tune(code, 0) == 0
        assert rows(lib, 32, 2048, STORE) == r, code


def test_the_window_follows_the_cu_count(lib):
    """tiles x 2 <= n_cu < tiles x 4: N in 528..1024 on 128 CUs, 1040..2048 on 256, 1232..2432 on 304."""
    assert lib.rt_debug_tune(3702, 0) == 0
    assert rows(lib, 32, 2048, RESID, n_cu=128) == 0 and rows(lib, 32, 1024, RESID, n_cu=128) == 16 and rows(lib, 64, 528, STORE, n_cu=128) == 32
    assert rows(lib, 32, 512, RESID, n_cu=128) == 0
    assert rows(lib, 32, 1040, RESID, n_cu=304) == 0 and rows(lib, 32, 1216, RESID, n_cu=304) == 0       # (the row-block rule's on 304 CUs)
    assert rows(lib, 32, 1232, RESID, n_cu=304) == 16 and rows(lib, 64, 2432, RESID, n_cu=304) == 32 and rows(lib, 32, 2448, RESID, n_cu=304) == 0


def test_the_row_block_query_answers_by_its_own_rule_alone(lib):
    """rt_debug_col_row_blocks as tests/test_col_row_blocks_cpu.py pins it, under every value of the new switch; and where the row-block
    rule holds the tile-block rule does not."""
    assert lib.rt_debug_tune(3602, 0) == 0
    q = lib.rt_debug_col_row_blocks
    for value in (0, 1, 2):
        assert lib.rt_debug_tune(3700 + value, 0) == 0
        for N, epi in ((1024, RESID), (1024, STORE)):
            assert q(N_CU, 64, N, epi, 0) == 32 and q(N_CU, 33, N, epi, 0) == 32 and q(N_CU, 32, N, epi, 0) == 16 and q(N_CU, 17, N, epi, 0) == 16
            assert rows(lib, 64, N, epi) == 0 and rows(lib, 32, N, epi) == 0
        for N, epi in ((4096, STORE), (2048, STORE), (6144, SILU), (2048, RESID), (12288, SILU), (3072, STORE)):
            for M in (1, 16, 17, 32, 33, 64, 65, 128):
                assert q(N_CU, M, N, epi, 0) == 0, (N, epi, M)
        assert q(N_CU, 64, 1024, RESID, 1) == 32 and q(N_CU, 64, 1024, RESID, 2) == 32 and q(N_CU, 64, 1024, RESID, 4) == 0
        assert q(N_CU, 64, 2048, RESID, 1) == 32 and q(N_CU, 64, 2048, RESID, 0) == 0
        assert q(N_CU, 64, 192, SILU, 0) == 32 and q(N_CU, 20, 192, SILU, 0) == 16
        assert q(128, 64, 1024, RESID, 2) == 0 and q(304, 64, 1024, RESID, 2) == 32
    # with the row-block rule switched off its launches stay half-tile launches: the window is arithmetic, not "whatever is left"
    assert lib.rt_debug_tune(3600, 0) == 0 and lib.rt_debug_tune(3702, 0) == 0
    assert q(N_CU, 32, 1024, RESID, 0) == 0 and rows(lib, 32, 1024, RESID) == 0


def test_bad_arguments_are_refused(lib):
    for args in ((0, 32, 2048, RESID, 0), (256, 0, 2048, RESID, 0), (256, 129, 2048, RESID, 0), (256, 32, 0, RESID, 0), (256, 32, 2048, 3, 0),
                 (256, 32, 1000, SILU, 0), (256, 32, 2048, RESID, 3), (256, 32, 2048, RESID, 8)):
        assert lib.rt_debug_col_tile_blocks(*args) == -1, args
