"""include/pcgrl_hip.h promises that every developer switch of pcgrl_tuning gives the same results as the default ("the tests run
the alternatives against the same fixtures").  This keeps the promise checked: every field must be set by some GPU test
(tests/test_gpu_*.py) -- through _tune(), a tuning dict or TUNING_OVERRIDES.  No GPU needed: it reads source files only."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# deliberately gives wrong results (timing experiments: the MiniDungeons planner runs one agent only)
EXEMPT = {"md_only_agent"}


def tuning_fields():
    src = open(os.path.join(ROOT, "include", "pcgrl_hip.h")).read()
    body = re.search(r"typedef struct pcgrl_tuning \{(.*?)\} pcgrl_tuning;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip() for decl in re.findall(r"int32_t([^;]*);", body) for n in decl.split(",")]


def names_set(path):
    """String keys a test file hands to the library as switches: _tune(mp, "x", v), setitem(TUNING_OVERRIDES, "x", v),
    {"x": v}, t["x"] = v, dict(x=v), and ("x", ...) parameter tuples handed to _tune(mp, switch, ...).  Docstrings and comments
    do not count."""
    out = set()
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Call):
            fn = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", "")
            if fn in ("_tune", "setitem"):
                out.update(a.value for a in node.args if isinstance(a, ast.Constant) and isinstance(a.value, str))
            if fn == "dict":
                out.update(k.arg for k in node.keywords if k.arg)
        elif isinstance(node, ast.Tuple) and node.elts and isinstance(node.elts[0], ast.Constant) and isinstance(node.elts[0].value, str):
            out.add(node.elts[0].value)
        elif isinstance(node, ast.Dict):
            out.update(k.value for k in node.keys if isinstance(k, ast.Constant) and isinstance(k.value, str))
        elif isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Subscript) and isinstance(t.slice, ast.Constant) and isinstance(t.slice.value, str):
                    out.add(t.slice.value)
    return out


def test_header_lists_the_switches():
    f = tuning_fields()
    assert len(f) == len(set(f)) and {"no_fused", "inline_reset", "no_wide", "sok_spawn", "md_only_agent"} <= set(f), f


def test_every_switch_is_set_by_a_gpu_test():
    used = set()
    for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")):
        used |= names_set(p)
    missing = [f for f in tuning_fields() if f not in EXEMPT and f not in used]
    assert not missing, "pcgrl_tuning switches no GPU test sets: %s" % missing
