"""The compiler's own report on the kernels of one csrc/*.hip, for the resource tests: the source is compiled to device assembly
with the library's flags (no GPU needed: hipcc cross-compiles), once per process, and read into

    report("logodds_map.hip")[("k_ms_score", (4,))].resources["NumVgprs"]

A kernel is a symbol named by an .amdhsa_kernel directive; its key is the identifier and the template arguments decoded from the
Itanium-mangled symbol, e.g. ("k_resp_rows", (3, 11, True, False, False, False)) or ("k_gm_fold", ())."""
import collections
import functools
import pathlib
import re
import shutil
import subprocess
import tempfile

import pytest

from lslam_amd import build

# what the library is built with, less the link-only options: the budgets hold for the code objects that ship
FLAGS = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] + ["-S", "--cuda-device-only"]

Kernel = collections.namedtuple("Kernel", "resources ops")  # {"NumVgprs": 54, ...}, Counter({"v_readlane_b32": 2, ...})

_LENGTH = re.compile(r"\d+")
_SUBSTITUTION = re.compile(r"S[0-9A-Z]*_")
_LITERAL = re.compile(r"L([ijb])(n?)(\d+)E")
_BUILTIN = "vwbcahstijlmxynofdegz"


def _name_part(s, i):
    """The index behind the part of a name at s[i]: a substitution, a <length><identifier>, or template arguments."""
    m = _SUBSTITUTION.match(s, i)
    if m:
        return m.end()
    m = _LENGTH.match(s, i)
    if m:
        return m.end() + int(m.group())
    if s[i] != "I":
        raise ValueError(s[i:])
    i += 1
    while s[i] != "E":
        i = _argument(s, i)[1]
    return i + 1


def _type(s, i):
    """The index behind the type at s[i]."""
    while s[i] in "PKRO":
        i += 1
    if s[i] in _BUILTIN:
        return i + 1
    if s[i] == "N":
        i += 1
        while s[i] != "E":
            i = _name_part(s, i)
        return i + 1
    i = _name_part(s, i)
    return _name_part(s, i) if s[i:i + 1] == "I" else i  # a template-id, e.g. HIP_vector_type<double, 2>


def _argument(s, i):
    """(value, index behind it) of the template argument at s[i]: an int, a bool, or a type as its mangled text."""
    if s[i] == "L":
        m = _LITERAL.match(s, i)
        if not m:
            raise ValueError(s[i:])
        v = int(m.group(3))
        return (bool(v) if m.group(1) == "b" else -v if m.group(2) else v), m.end()
    j = _type(s, i)
    return s[i:j], j


def decode(symbol):
    """_ZN12_GLOBAL__N_112k_resp_tile3ILi3ELb1EEEvPK... -> ("k_resp_tile3", (3, True)).  Raises ValueError, naming the symbol, where
    the identifier or its template arguments cannot be delimited."""
    try:
        if not symbol.startswith("_Z"):
            raise ValueError(symbol)
        nested = symbol[2] == "N"
        i, name, args = 2 + nested, None, []
        m = _LENGTH.match(symbol, i)
        while m:  # the namespaces, then the identifier
            i = m.end() + int(m.group())
            name = symbol[m.end():i]
            m = _LENGTH.match(symbol, i)
        if name is None or len(symbol) < i:
            raise ValueError(symbol)
        if symbol[i:i + 1] == "I":
            i += 1
            while symbol[i] != "E":
                v, i = _argument(symbol, i)
                args.append(v)
            i += 1
        if nested and symbol[i] != "E":
            raise ValueError(symbol)
        return name, tuple(args)
    except (ValueError, IndexError):
        raise ValueError("cannot decode the kernel symbol %r" % symbol) from None


def parse(text):
    """(identifier, template arguments) -> Kernel, for every kernel of a device assembly text."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    seen, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"(_Z\S+):", line)  # a function label: a kernel's, or a device function's, which belongs to no kernel
        if m:
            cur = None
            if m.group(1) in kernels:
                kernels.remove(m.group(1))
                key = decode(m.group(1))
                if key in seen:
                    raise ValueError("two kernels decode to %r" % (key,))
                cur = seen[key] = Kernel({}, collections.Counter())
            continue
        if cur is None:
            continue
        m = re.match(r"; (\w+): (\d+)", line)  # the report block: "; NumVgprs: 54", "; LDSByteSize: 0 bytes/workgroup ..."
        if m:
            cur.resources[m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"\s+([a-z]\w*)", line)  # an instruction; directives begin with a dot, comments with a semicolon
        if m:
            cur.ops[re.sub(r"_e(32|64)$", "", m.group(1))] += 1
    if kernels:  # e.g. an extern "C" kernel, whose label is no _Z...
        raise ValueError("kernels without a decodable label: %s" % sorted(kernels))
    return seen


@functools.lru_cache(maxsize=None)
def report(source_name):
    """parse() of csrc/<source_name>, compiled once per process; skips the calling test where there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not pathlib.Path(hipcc).exists():
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        out = pathlib.Path(tmp) / (source_name + ".s")
        subprocess.run([hipcc, *FLAGS, "-o", str(out), str(build.CSRC / source_name)], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return parse(out.read_text())
