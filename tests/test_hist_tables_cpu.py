"""What the three tables folded from the level-2 history ring share, without a GPU: the cursor's rule
(bourse_amd/csrc/hist_cursor.hpp, compiled with g++ into a program of its own, plain and under the sanitizers), and the shape
of the one host path in bourse_amd.hip - an env without a table launches nothing for it, every kernel has one launch site,
and the resets check every table for lost steps before they launch for any."""
import os
import re
import subprocess

from test_bins_cpu import ROOT, _cxx

CSRC = os.path.join(ROOT, "bourse_amd", "csrc")
TABLES = ("series", "lags", "bins")
LAUNCHERS = [f"launch_{t}_{k}" for t in TABLES for k in ("fold", "clear")]


def _cursor_exe(tmp_path, extra=()):
    exe = str(tmp_path / "hist_cursor_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "hist_cursor_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_hist_cursor_hpp_by_hand_and_against_a_ring_that_is_really_written(tmp_path):
    run = subprocess.run([_cursor_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and re.search(r"hist_cursor ok \d{4} cases", run.stdout), run.stdout + run.stderr


def test_hist_cursor_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own"""
    exe = _cursor_exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "hist_cursor ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_the_cursor_header_is_plain_and_the_kernels_share_one_ring_header():
    cur = open(os.path.join(CSRC, "hist_cursor.hpp")).read()
    assert "hip_runtime" not in cur and "asm" not in re.sub(r"//.*", "", cur)
    ring = re.sub(r"//.*", "", open(os.path.join(CSRC, "hist_ring.hpp")).read())
    assert re.search(r"namespace bkd \{\s*namespace ring \{", ring) and "__global__" not in ring and "asm" not in ring
    assert "series::" not in ring and "lags::" not in ring and "bins::" not in ring
    for t in TABLES:
        src = open(os.path.join(CSRC, t + ".hpp")).read()
        assert '#include "hist_ring.hpp"' in src, t
        code = re.sub(r"//.*", "", src)
        # none of them keeps a copy of its own: no definition of the shared helpers, no record address spelled out
        assert not re.search(r"\b(wave_sync|vec_of|vec_lo|vec_hi|slot_of)\([^;{]*\)\s*\{", code), t
        assert "__builtin_amdgcn_fence" not in code and "n_books + b" not in code and "g.mask" not in code, t
        assert len(re.findall(r"ring::record\(", code)) >= 1 and len(re.findall(r"ring::masked_book\(", code)) == 1, t


def _functions(hip):
    return {m.group(1): fn for fn in re.split(r"\n(?=(?:static )?[\w:]+ \w+\([^;]*\) \{)", hip)
            for m in [re.match(r"(?:static )?[\w:]+ (\w+)\(", fn)] if m}


def test_every_launch_of_the_three_tables_sits_behind_the_on_flag_and_the_resets_check_all_before_launching_any():
    hip = open(os.path.join(CSRC, "bourse_amd.hip")).read()
    code = re.sub(r"//.*", "", hip)
    fns = _functions(code)
    # each of the six kernels is named at one launch site, inside its own launcher
    for t in TABLES:
        for k in ("fold", "clear"):
            sites = [name for name, fn in fns.items() if f"{t}::k_{k}," in fn]
            assert sites == [f"launch_{t}_{k}"] and code.count(f"{t}::k_{k},") == 1, (t, k, sites)
    # the launchers are named where they are declared and defined, and where the three descriptors are filled - nowhere else
    filled = re.search(r"HistTable tables\[N_HIST_TABLES\] = \{(.*?)\};", code, flags=re.S)
    assert filled and [x for x in re.findall(r"launch_\w+", filled.group(1))] == LAUNCHERS
    for name in LAUNCHERS:
        uses = [m.start() for m in re.finditer(r"\b" + name + r"\b", code)]
        decl = [m.start() for m in re.finditer(r"static void " + name + r"\(", code)]
        assert len(decl) == 2 and len(uses) == 3, (name, len(uses))
        assert [u for u in uses if not filled.start() <= u < filled.end()] == [d + len("static void ") for d in decl], name
    # so a table's kernels run only through its descriptor: .fold( in one function, .clear( in four
    through = {name: re.findall(r"\bt\.(fold|clear)\(env", fn) for name, fn in fns.items()}
    through = {name: calls for name, calls in through.items() if calls}
    assert through == {"table_fold_outstanding": ["fold"], "table_start_again": ["clear"], "table_clear_device": ["clear"],
                       "reset_books_from": ["clear"], "bk_checkpoint_load": ["clear"]}, through
    assert not re.search(r"\.(fold|clear)\(env", re.sub(r"\bt\.(fold|clear)\(env", "", code))
    # ... and every one of those tests `on` first, itself or through the guard
    load = fns["bk_checkpoint_load"]
    assert "t.on = true;" in fns["table_commit_enable"][:fns["table_commit_enable"].index("table_start_again(env")]
    assert "if (!t.on) continue;" in load[load.index("for (HistTable& t : env->tables)"):load.index("t.clear(env")]
    assert "if (!t.on) return fail(" in fns["table_ok"]
    for name in ("table_fold", "table_clear_device", "table_clear"):
        body = fns[name][fns[name].index("{"):]
        assert body.lstrip("{\n ").startswith("if (int rc = table_ok(env, which)) return rc;"), name
    callers = {name for name, fn in fns.items() if re.search(r"\btable_fold_outstanding\(env", fn[fn.index("{"):])}
    assert callers == {"table_fold", "table_clear_device", "reset_books_from"}, callers
    callers = {name for name, fn in fns.items() if re.search(r"\btable_start_again\(env", fn[fn.index("{"):])}
    assert callers == {"table_commit_enable", "table_clear_device"}, callers
    for t in TABLES:  # the entries are wrappers: they name no launcher and no kernel, only the shared functions
        for e, shared in (("fold", "table_fold"), ("clear_device", "table_clear_device"), ("clear", "table_clear")):
            assert re.search(r"\{ return " + shared + r"\(env, T_" + t.upper() + r"\b", fns[f"bk_{t}_{e}"]), (t, e)
        assert f"table_commit_enable(env, env->tables[T_{t.upper()}])" in fns[f"bk_{t}_enable"], t
    # the resets' opening: the loop of lost checks, then the loop that folds and cuts, then the reset itself
    reset = fns["reset_books_from"]
    loops = [m.start() for m in re.finditer(r"\bfor \(", reset)]
    assert len(loops) == 2
    check, fold, cut, go = (reset.index(x) for x in ("table_lost_check(env", "table_fold_outstanding(env", "t.clear(env, mask_dev, env->M, true)",
                                                     "launch_reset_books("))
    assert loops[0] < check < loops[1] < fold < cut < go, (loops, check, fold, cut, go)
    assert "if (env->tables[i].on)" in reset[loops[0]:check] and "if (!t.on) continue;" in reset[loops[1]:fold]
    # the checks run bins, lags, series; the launches series, lags, bins (the descriptors' order)
    assert "for (int i = N_HIST_TABLES - 1; i >= 0; --i)" in reset[loops[0]:check] and "for (HistTable& t : env->tables)" in reset[loops[1]:fold]
    assert re.search(r"enum \{ T_SERIES, T_LAGS, T_BINS, N_HIST_TABLES \};", code)
