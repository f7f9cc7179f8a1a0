"""CPU checks of the launch-plan switches: rho_tts_amd/csrc/knobs.h is the one table of them, and rt_debug_tune accepts exactly the
codes its rows describe.  rt_debug_tune touches a mutex and atomics only, so it is called here without a GPU."""
import os
import re

from rho_tts_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = re.compile(r"\bX\(\s*(\d+)\s*,\s*(g_\w+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(0x[0-9a-fA-F]+|\d+)\s*,\s*\"")


def table():
    """(coded rows, argument rows) of knobs.h as (base, name, default, lo, hi).  The argument row (RT_KNOB_ARG: the one switch set
    by rt_debug_tune's second argument) has a range of ARGUMENT values, not of codes."""
    src = open(os.path.join(ROOT, "rho_tts_amd", "csrc", "knobs.h")).read()
    at = src.index("#define RT_KNOB_ARG(")
    parse = lambda text: [(int(b), n, int(d), int(lo), int(hi, 0)) for b, n, d, lo, hi in ROW.findall(text)]
    return parse(src[:at]), parse(src[at:])


def tune_comment():
    src = open(os.path.join(ROOT, "include", "rho_tts_amd_debug.h")).read()
    return [c for c in re.findall(r"/\*.*?\*/", src, flags=re.S) if "A/B switches for measurements" in c][0]


# `BASE + name` calls whose values no loop or single-name parametrize line of the file spells out
OFFSETS = {("tests/test_long_context_gpu.py", "route"): (0, 1, 2)}          # second column of DECODE_CASES


def tune_calls():
    """(file, code) of every rt_debug_tune( call under tests/ and tools/ whose code the source spells out: integer literals as they
    stand; the names in `BASE + name` and bare names through the literal tuples that the file's `for name in (...)` loops,
    `name = (...)[i]` lines and `parametrize("name", [...])` marks give them (every `BASE + name` must resolve; a bare name that does
    not - a function parameter, a command-line argument - is left to the callers' literals)."""
    found = []
    for sub in ("tests", "tools"):
        for fn in sorted(os.listdir(os.path.join(ROOT, sub))):
            if not fn.endswith(".py") or fn == os.path.basename(__file__):
                continue
            src, where, values = open(os.path.join(ROOT, sub, fn)).read(), f"{sub}/{fn}", {}
            for name, tup in (re.findall(r"\bfor (\w+) in (\([^\n]*?\)):", src) + re.findall(r"\b(\w+) = (\([\d, ]+\))\[", src) +
                              re.findall(r"parametrize\(\"(\w+)\", (\[[\d, ]+\])", src)):
                values.setdefault(name, set()).update(int(v) for v in re.findall(r"\d+", tup))
            for name, alias in re.findall(r"\bfor (\w+) in (\w+):", src):
                values.setdefault(name, set()).update(values.get(alias, ()))
            for (f, name), offs in OFFSETS.items():
                if f == where:
                    values.setdefault(name, set()).update(offs)
            for arg in re.findall(r"rt_debug_tune\(\s*(.+?)\s*,\s*\w+\)", src):
                m = re.fullmatch(r"(?:(\d+) \+ )?(?:int\()?(\w+)\)?", arg)
                assert m, f"{where}: rt_debug_tune({arg}, ...) is not understood by this test"
                if m.group(2).isdigit():
                    found.append((where, int(m.group(1) or 0) + int(m.group(2))))
                    continue
                assert m.group(1) is None or values.get(m.group(2)), f"{where}: the values of {arg} are not spelled out in the file"
                found += [(where, int(m.group(1) or 0) + v) for v in sorted(values.get(m.group(2), ()))]
    return found


def test_table_is_ordered_disjoint_and_documented():
    rows, arg_rows = table()
    assert len(rows) + len(arg_rows) >= 31 and len(arg_rows) == 1
    assert len({r[1] for r in rows + arg_rows}) == len(rows) + len(arg_rows)
    for base, name, default, lo, hi in rows + arg_rows:
        assert lo <= default <= hi, name
    spans = [(base + lo, base + hi, name) for base, name, _, lo, hi in rows]
    assert spans == sorted(spans), "rows in ascending code order"
    for (_, hi_a, a), (lo_b, _, b) in zip(spans, spans[1:]):
        assert hi_a < lo_b, f"{a} and {b} overlap"
    comment = tune_comment()
    for base, name, *_ in rows + arg_rows:
        assert re.search(rf"(?<![\d.])\b{base}\b", comment), f"{name}: code {base} is missing from rho_tts_amd_debug.h"
    assert "RT_ERR_INVALID" in comment and "1100/1101" in comment and "1200/1201" in comment


def test_tune_accepts_the_table_and_nothing_else():
    lib = _native.load_library()
    rows, ((abase, _, adefault, alo, _),) = table()
    try:
        for base, name, default, lo, hi in rows:
            for v in (lo, hi, default):
                assert lib.rt_debug_tune(base + v, 0) == 0, (name, base + v)
        assert lib.rt_debug_tune(abase, alo) == 0 and lib.rt_debug_tune(abase, adefault) == 0
        spans = [(base + lo, base + hi) for base, _, _, lo, hi in rows]
        gaps = [(a_hi + 1, b_lo - 1) for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]) if b_lo - a_hi > 1]
        assert gaps
        bad = {c for g in gaps for c in (g[0], (g[0] + g[1]) // 2, g[1])} | {2550, 3150, 99, -1, -2301, spans[-1][1] + 1, 1 << 30}
        for code in sorted(bad):
            assert not any(lo <= code <= hi for lo, hi in spans), code
            before = max((s for s in spans if s[1] < code), default=spans[0])[1]
            after = min((s for s in spans if s[0] > code), default=spans[-1])[0]
            assert lib.rt_debug_tune(before, 0) == 0
            assert lib.rt_debug_tune(code, 0) == _native.RT_ERR_INVALID, code
            assert lib.rt_debug_tune(code, 8) == _native.RT_ERR_INVALID, code
            assert lib.rt_debug_tune(before, 0) == 0 and lib.rt_debug_tune(after, 0) == 0, code
    finally:
        restore_defaults(lib)


def test_every_code_used_by_tests_and_tools_is_accepted():
    lib = _native.load_library()
    calls = tune_calls()
    files = {f for f, _ in calls}
    assert len(calls) >= 60 and "tests/test_model_gpu.py" in files and "tools/bench_gemm.py" in files, sorted(files)
    for expected in (("tests/test_model_gpu.py", 2032), ("tests/test_model_gpu.py", 1707), ("tests/test_provider_gpu.py", 1401),
                     ("tests/test_kernels_gpu.py", 1903), ("tests/test_gemm_col_gpu.py", 2301), ("tools/bench_gemm.py", 2)):
        assert expected in calls, expected
    try:
        for where, code in calls:
            assert lib.rt_debug_tune(code, 0) == 0, (where, code)
    finally:
        restore_defaults(lib)


def restore_defaults(lib):
    """Later tests in this process see the shipped plan."""
    rows, ((abase, _, adefault, _, _),) = table()
    for base, name, default, _, _ in rows:
        assert lib.rt_debug_tune(base + default, adefault if base == abase else 0) == 0, name
