"""What the tests that need no GPU share (test_*_host.py, test_*_resources.py): the configuration the library is handed, the header
and what it declares, the kernels' resource directives in the compiler's assembly, the sanitized stand-alone simulators."""
import functools
import os
import re
import subprocess
import tempfile

from hostsim_build import build_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(prob, h, w, power=None, num_envs=1, rep="wide"):
    """The configuration BatchedPcgrlEnv hands the library for `prob` on maps of h rows x w columns, solver_power `power` where one is
    given (smb's is an attribute, not an adjust_param key: readout_harness.make_env).  No GPU: nothing is allocated."""
    from readout_harness import make_env
    return make_env(prob, h, w, power, rep=rep, seed=0, num_envs=num_envs)._config()


def forms(h, w):
    """The (lane group, mask width) forms that hold a map of h rows and w columns; the first is the one the library takes."""
    return [(g, b) for g in (16, 64) if h <= g for b in (32, 64) if w <= b]


def run_sanitized(src, define, timeout):
    """tests/hostsim/<src> with its own main() (-D<define>), built with the address and undefined-behaviour sanitizers and run as a
    program: it must end with status 0 and the line `ok`, with no report in between.  Returns what it printed."""
    r = subprocess.run([build_sanitized(src, define)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stdout, r.stdout[-2000:]
    return r.stdout


@functools.lru_cache(None)
def header():
    return open(os.path.join(ROOT, "include", "pcgrl_hip.h")).read()


@functools.lru_cache(None)
def plain_header():
    """include/pcgrl_hip.h with its comments dropped."""
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def _spaced(ctype):
    """A C type as a regular expression: any white space between its words and around a `*`."""
    words = ctype.replace("*", " * ").split()
    return "".join((r"\s*\*" if w == "*" else (r"\s+" if i and words[i - 1] != "*" else "") + re.escape(w)) for i, w in enumerate(words))


def prototype(ret, name, params):
    """The regular expression of `ret name(params...);` for parameter types like "const uint8_t*" or "int32_t": any parameter names,
    any white space."""
    args = [_spaced(p) + (r"\s*\w+" if p.endswith("*") else r"\s+\w+") for p in params]
    return r"\b" + _spaced(ret) + r"\s+" + name + r"\s*\(\s*" + r"\s*,\s*".join(args) + r"\s*\)\s*;"


# the parameters pcgrl_get_solution, pcgrl_get_playthrough and pcgrl_get_smb_play share
MOVES_PARAMS = ["pcgrl_env*", "const uint8_t*", "int32_t", "int32_t", "int8_t*", "int32_t*", "int8_t*", "int32_t*", "void*", "size_t", "void*"]


def struct_fields(name, ctype_map):
    """[(field, ctypes type)] of `typedef struct name {...} name;` in the header, in order: one declarator list per statement
    (`int32_t *a, *b;` declares two pointers), `ctype_map` from the C type as written ("const uint8_t*", "int32_t") to ctypes."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), plain_header(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        m = re.match(r"\s*((?:const\s+)?\w+)(.*)$", decl, re.S)
        base = " ".join(m.group(1).split())
        for part in m.group(2).split(","):
            fields.append((part.replace("*", "").strip(), ctype_map[base + ("*" if "*" in part else "")]))
    return fields


@functools.lru_cache(None)
def kernel_resources(part):
    """{demangled kernel name without its parameters: (vector registers, scalar registers, scratch bytes)} of part `part` of
    csrc/pcgrl_abi.hip, read from the `.amdhsa_` directives of the compiler's gfx950 assembly.  Compiled once per process and part."""
    from gym_pcgrl_amd import _lib
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "part%d.s" % part)
        subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + [f for f in _lib.HIPCC_FLAGS if f != "-shared"] +
                              ["-DPCGRL_PART=%d" % part, "--cuda-device-only", "-S", _lib.SOURCES[0], "-o", out], stderr=subprocess.DEVNULL)
        kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S)
    names = subprocess.run(["c++filt"] + [k for k, _ in kernels], stdin=subprocess.DEVNULL, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(names) == len(kernels)
    return {n.split("(")[0]: tuple(int(re.search(k + r"\s+(\d+)", body).group(1)) for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size"))
            for n, (_, body) in zip(names, kernels)}
