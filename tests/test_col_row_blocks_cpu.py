"""The row-block rule of the column-owner decode GEMM's launcher (gemm_col.hip col_workgroups + col_row_blocks) as host arithmetic:
rt_debug_col_row_blocks touches no GPU.  Checked at n_cu = 256 (MI355X) on the decode projections of the 1.7B preset."""
import pytest

from rho_tts_amd import _native

STORE, RESID, SILU = 0, 1, 2
N_CU = 256
# (N, epi, name): predictor H 1024 / I 3072, talker H 2048 / I 6144 (N of a gate/up launch is gate + up)
PRED_NARROW = [(1024, RESID, "pred o"), (1024, RESID, "pred down"), (1024, STORE, "mtp projection")]          # 64 tiles x split 2 = 128 workgroups
PRED_FULL = [(4096, STORE, "pred qkv"), (2048, STORE, "pred head"), (6144, SILU, "pred gate/up")]              # 256, 256, 192 workgroups
TALKER = [(4096, STORE, "talker qkv"), (2048, RESID, "talker o"), (12288, SILU, "talker gate/up"), (2048, RESID, "talker down"), (3072, STORE, "talker head")]


@pytest.fixture()
def lib():
    lib = _native.load_library()
    yield lib
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rho_tts_amd", "csrc", "knobs.h")).read()
    shipped = 3600 + int(re.search(r"X\(3600, g_col_row_blocks, (\d+),", src).group(1))        # later tests see the shipped plan
    assert lib.rt_debug_tune(shipped, 0) == 0


def rows(lib, M, N, epi, split=0, n_cu=N_CU):
    return lib.rt_debug_col_row_blocks(n_cu, M, N, epi, split)


def test_narrow_predictor_launches_get_blocks(lib):
    assert lib.rt_debug_tune(3602, 0) == 0
    for N, epi, name in PRED_NARROW:
        assert rows(lib, 64, N, epi) == 32 and rows(lib, 33, N, epi) == 32, name
        assert rows(lib, 32, N, epi) == 16 and rows(lib, 17, N, epi) == 16, name


def test_launches_that_fill_the_chip_get_none(lib):
    assert lib.rt_debug_tune(3602, 0) == 0
    for N, epi, name in PRED_FULL + TALKER:
        for M in (17, 32, 33, 64):
            assert rows(lib, M, N, epi) == 0, (name, M)


def test_sixteen_rows_and_fewer_and_sixty_five_and_more_get_none(lib):
    assert lib.rt_debug_tune(3602, 0) == 0
    for N, epi, name in PRED_NARROW + PRED_FULL + TALKER:
        for M in (1, 8, 16, 65, 96, 128):
            assert rows(lib, M, N, epi) == 0, (name, M)


def test_the_switch_changes_the_answers_as_documented(lib):
    N, epi, _ = PRED_NARROW[0]
    want = {0: {17: 0, 32: 0, 33: 0, 64: 0}, 1: {17: 0, 32: 0, 33: 32, 64: 32}, 2: {17: 16, 32: 16, 33: 32, 64: 32}}
    for value in (0, 1, 2):
        assert lib.rt_debug_tune(3600 + value, 0) == 0
        for M, r in want[value].items():
            assert rows(lib, M, N, epi) == r, (value, M)


def test_the_rule_counts_workgroups_after_the_split(lib):
    """Half of the CUs is the limit, counted in workgroups (tiles x sub-tile split), and a forced split moves it."""
    assert lib.rt_debug_tune(3602, 0) == 0
    assert rows(lib, 64, 1024, RESID, 1) == 32 and rows(lib, 64, 1024, RESID, 2) == 32 and rows(lib, 64, 1024, RESID, 4) == 0
    assert rows(lib, 64, 2048, RESID, 1) == 32 and rows(lib, 64, 2048, RESID, 0) == 0       # (automatic: 128 tiles x 2)
    assert rows(lib, 64, 192, SILU) == 32 and rows(lib, 20, 192, SILU) == 16                 # 6 pairs: the form the GPU test runs
    assert rows(lib, 64, 1024, RESID, 2, n_cu=128) == 0 and rows(lib, 64, 1024, RESID, 2, n_cu=304) == 32


def test_bad_arguments_are_refused(lib):
    for args in ((0, 32, 1024, RESID, 0), (256, 0, 1024, RESID, 0), (256, 129, 1024, RESID, 0), (256, 32, 0, RESID, 0), (256, 32, 1024, 3, 0),
                 (256, 32, 1000, SILU, 0), (256, 32, 1024, RESID, 3), (256, 32, 1024, RESID, 8)):
        assert lib.rt_debug_col_row_blocks(*args) == -1, args
