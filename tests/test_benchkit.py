"""tools/benchkit.py, the part that needs no GPU and no library: the step limit, the row format of each reader bench tool,
the writer -- and that no tools/*_bench.py carries a copy of a shared helper again."""
import ast
import glob
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import benchkit as kit  # noqa: E402


def test_limit_that_expires_ends_the_process_with_124():
    code = ("import sys, time; sys.path.insert(0, sys.argv[1]); import benchkit\n"
            "with benchkit.limit(1, 'nap', 'toy'):\n    time.sleep(30)\nprint('went on')\n")
    r = subprocess.run([sys.executable, "-c", code, TOOLS], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=20)
    assert r.returncode == 124
    assert r.stderr == "toy: step 'nap' passed its limit of 1 s; ending\n"
    assert r.stdout == ""


def test_limit_that_does_not_expire_puts_the_handler_back():
    def mine(*_):
        pass
    before = signal.signal(signal.SIGALRM, mine)
    try:
        with kit.limit(30, "nothing", "toy"):
            assert signal.getsignal(signal.SIGALRM) is not mine
        assert signal.getsignal(signal.SIGALRM) is mine
        assert signal.alarm(0) == 0
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, before)


def test_med():
    assert kit.med([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert kit.med([4.0, 1.0, 2.0, 3.0]) == (2.5, 1.0, 4.0)


# each expected string is the tool's own format expression before the kit, evaluated on these inputs
TS, EXTRA, NAME = [0.0123, 1.5, 0.25, 12.3456], "  ratio 1.50", "  1024 names, a wave per row"
ROWS = {
    (58, 10): "  1024 names, a wave per row                               us      875.0 (12.3 .. 12345.6)  ratio 1.50",    # count_le_bench.py
    (72, 10): "  1024 names, a wave per row                                             us      875.0 (12.3 .. 12345.6)  ratio 1.50",    # top_bench.py
    (78, 10): "  1024 names, a wave per row                                                   us      875.0 (12.3 .. 12345.6)  ratio 1.50",    # across_bench.py
    (96, 11): "  1024 names, a wave per row                                                                     us       875.0 (12.3 .. 12345.6)  ratio 1.50",    # kept_bench.py
}


@pytest.mark.parametrize("width,digits", sorted(ROWS))
def test_row(width, digits, capsys):
    for rep, kw in ((kit.Report(width, digits), {}), (kit.Report(1, 1), dict(width=width, digits=digits))):
        assert rep.row(NAME, TS, EXTRA, **kw) == 0.875
        assert rep.lines == [ROWS[width, digits]]
        assert capsys.readouterr().out == ROWS[width, digits] + "\n"
        assert rep.row("x", [2.0]) == 2.0 and rep.lines[-1] == f"{'x':<{rep.width}} us {2000.0:{rep.digits}.1f} (2000.0 .. 2000.0)"
        capsys.readouterr()


def test_note(capsys):
    rep = kit.Report(10)
    rep.note("# quiet")
    assert capsys.readouterr().out == ""
    rep.note("# loud", echo=True)
    assert capsys.readouterr().out == "# loud\n" and rep.lines == ["# quiet", "# loud"]


def test_write(tmp_path):
    rep = kit.Report(10)
    rep.note("# MARK here")
    rep.note("row 1")
    out = tmp_path / "made" / "deeper" / "o.txt"                       # the directory is created
    rep.write(str(out))
    assert out.read_text() == "# MARK here\nrow 1\n"
    rep.write(str(out), mark="# MARK")                                 # with a mark and no head: just the lines
    assert out.read_text() == "# MARK here\nrow 1\n"
    fresh = tmp_path / "other" / "o.txt"                               # with a mark and no file: just the lines
    rep.write(str(fresh), mark="# MARK")
    assert fresh.read_text() == "# MARK here\nrow 1\n"
    out.write_text("table 1\ntable 2\n\n# MARK of an older run\nold row\n# MARK again\nold row 2\n")
    rep.write(str(out), mark="# MARK")                                 # three lines above the first mark survive
    assert out.read_text() == "table 1\ntable 2\n\n# MARK here\nrow 1\n"
    rep.write(str(out))                                                # without a mark nothing survives
    assert out.read_text() == "# MARK here\nrow 1\n"


SHARED = {"limit", "med", "timed_events", "timed_device", "timed_wall"}
ALLOWED = set()      # (tool, function) pairs that may stay, each with its reason as a comment; never a shared helper itself: none today


def test_no_tool_defines_a_shared_helper():
    tools = sorted(glob.glob(os.path.join(TOOLS, "*_bench.py")))
    assert len(tools) >= 11
    found = set()
    for path in tools:
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):                                    # every nesting depth
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name in SHARED:
                found.add((os.path.basename(path), node.name))
    assert found == ALLOWED, found ^ ALLOWED
