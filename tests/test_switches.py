"""The fit's environment switches: the stream creation order they must not move, and the README's
switch table against the code."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "machine-learning-replications_amd")

# runtime.py builds FIT_STREAMS at import from os.environ alone, so the child loads that one file
# with a placeholder for torch (its import would take seconds) instead of importing the package
_CHILD = """
import importlib.util, sys, types
class Placeholder(types.ModuleType):
    def __getattr__(self, name):     # (torch.float32 as a default argument, nothing more)
        return None
sys.modules["torch"] = Placeholder("torch")
spec = importlib.util.spec_from_file_location("hfens_runtime", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
print(repr(mod.FIT_STREAMS))
"""


def test_fit_streams_default_creation_order():
    """HIP maps streams to hardware queues in creation order, and the fit's speed depends on that
    mapping (runtime.py): with no HFENS_* variable set the fit creates exactly these six streams,
    in this order, at these priorities."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HFENS_")}
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(PKG, "runtime.py")], env=env,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert eval(r.stdout) == (("aux", 0), ("lasso_refit", 0), ("svc", -1), ("bases", 0), ("svc_ws_0", -1),
                              ("svc_ws_1", 0))


def _sources():
    paths = [os.path.join(ROOT, "bench.py")]
    for d, _, files in os.walk(PKG):
        paths += [os.path.join(d, f) for f in files if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp"))]
    return paths


def test_readme_switch_table_has_no_stale_rows():
    """Every HFENS_* name in the README's switch table is read (os.environ / getenv) somewhere in the
    package or in bench.py.  One direction only: a switch need not be documented."""
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        rows = [ln for ln in f if ln.startswith("| `HFENS_")]
    names = sorted({n for ln in rows for n in re.findall(r"HFENS_[A-Z0-9]+(?:_[A-Z0-9]+)*", ln)})
    assert len(rows) > 40 and names, "the switch table was not found"
    read = set()
    for p in _sources():
        with open(p, encoding="utf-8", errors="replace") as f:
            read.update(re.findall(r"(?:environ|getenv)[^\n]*?[\"'](HFENS_[A-Z0-9_]+)[\"']", f.read()))
    stale = [n for n in names if n not in read]
    assert not stale, f"README documents switches nothing reads: {stale}"
