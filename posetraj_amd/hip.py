"""ctypes binding of ``libposetraj_hip.so`` (C ABI declared in ``include/posetraj_hip.h`` and the extension headers beside it: ``ABIS``).

There is no fallback: if the library is missing or a call fails, a ``RuntimeError`` is raised.  ``build()``
compiles the HIP sources for gfx950 in-tree (``posetraj_amd/libposetraj_hip.so``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.abspath(os.environ["PT_LIB"]) if os.environ.get("PT_LIB") else os.path.join(HERE, "libposetraj_hip.so")   # PT_LIB: A/B against another build on one box
SOURCES = ["api.hip", "igemm.hip", "ffn.hip", "lnlin.hip", "norm.hip", "attn.hip", "attn_general.hip", "elementwise.hip", "vae.hip", "vae_f32.hip", "clip.hip", "raster.hip", "train.hip", "gemm.hip", "norm_bwd.hip", "pointwise_bwd.hip", "optim.hip", "attn_bwd.hip", "batch.hip", "control.hip", "sampler.hip"]
HEADERS = ["pt_common.h", "igemm_tail.h", "pt_fold.h", "pt_launch.h"]
INCLUDE = os.path.join(HERE, "..", "include")


class Abi(typing.NamedTuple):
    """One header of the C ABI: what is written in _ROWS below, then what the import reads from the header itself."""
    name: str
    header: str                      # file name under include/
    prefix: str                      # of every entry point the header declares; `<prefix>abi_version()` returns the library's version
    macro: str                       # the version macro
    struct_classes: dict             # {struct tag: Python class name}
    version: int = None              # the macro's value
    structs: dict = None             # {struct tag: ctypes.Structure class}, the header's own
    prototypes: dict = None          # the C spelling, name -> (return type, [parameter types])
    signatures: dict = None          # name -> (restype, argtypes)


# Every header of the library, the frozen core first; each extension has a prefix and a version of its own.  This is the only list:
# the parser's prefixes, the bindings, the version check at load, the rebuild check and the source digest all follow it
# (a new family of entry points is a new header and one row here).  A later header may use the structs of an earlier one.
_ROWS = (
    Abi("core", "posetraj_hip.h", "pt_", "PT_ABI_VERSION", {"pt_igemm_params": "IgemmParams", "pt_ffn_params": "FfnParams", "pt_lnlin_params": "LnLinParams",
                                                            "pt_conv_f32_params": "ConvF32Params", "pt_gemm_params": "GemmParams"}),
    Abi("optim", "posetraj_optim.h", "pto_", "PT_OPTIM_ABI_VERSION", {"pt_adam8_segment": "Adam8Segment"}),     # 8-bit AdamW
    Abi("det", "posetraj_det.h", "ptd_", "PT_DET_ABI_VERSION", {}),                  # deterministic reductions (reuses pt_gemm_params)
    Abi("temporal", "posetraj_temporal.h", "ptt_", "PT_TEMPORAL_ABI_VERSION", {}),   # temporal attention backward of 33 - 128 frames
    Abi("batch", "posetraj_batch.h", "ptb_", "PT_BATCH_ABI_VERSION", {}),            # the temporal blocks' cross-attention rows of a batch of clips
    Abi("control", "posetraj_control.h", "ptc_", "PT_CONTROL_ABI_VERSION", {}),      # per-row weighted accumulation of the ControlNet residuals
    Abi("sampler", "posetraj_sampler.h", "pts_", "PT_SAMPLER_ABI_VERSION", {}),      # the linear multistep (DPM-Solver++(2M)) step
)

# The windowed denoise loop's two passes are an add-on library of their own (posetraj_amd/windows.py binds it): libposetraj_window.so
# from csrc/window.hip, declared in include/posetraj_window.h.  Not a row of the table above, not in SOURCES or header_paths(): the main
# library, its digest and its rebuild inputs do not know it.  The same reader reads its header; build() makes it after the main link.
_WINDOW_ROW = Abi("window", "posetraj_window.h", "ptw_", "PT_WINDOW_ABI_VERSION", {})
WINDOW_SOURCE, WINDOW_LIB_PATH = "window.hip", os.path.join(HERE, "libposetraj_window.so")

_lib = _checked = _window = None

# The headers are the only description of the ABI: the parameter structs, the signature tables and the versions below are
# read from them at import (the C subset they use, nothing more; tests/test_abi_cpu.py has a C++ compiler confirm the reading).
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_TYPE = r"(?:const\s+)?\w+\s*\*?"
_ENTRY = r"(?:%s)[a-z0-9_]+" % "|".join(re.escape(a.prefix) for a in _ROWS + (_WINDOW_ROW,))
_DECL = re.compile(r"""\s*(?: typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P=tag)\s*;
                            | (?P<ret>%s)\s*\b(?P<fn>%s)\s*\((?P<params>[^()]*)\)\s*;
                            | extern\s+"C"\s*\{ | \} )""" % (_TYPE, _ENTRY), re.X)
_FIELD = re.compile(r"(%s)\s*\b(\w+(?:\s*,\s*\w+)*)" % _TYPE)         # `int32_t C0, C1`, `const void* x0`; a parameter is the one-name case


def _ctype(spelling: str, structs: dict, returned: bool = False, header: str = "posetraj_hip.h"):
    """ctypes type of a C type as ``header`` spells it: scalars by name, `const pt_X_params*` a pointer to that struct,
    a returned `const char*` a string, every other pointer c_void_p."""
    m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*)?", spelling)
    const, base, ptr = m.groups() if m else (None, None, None)
    if not ptr and not const and base in _SCALARS:
        return _SCALARS[base]
    if ptr and const and base in structs:
        return C.POINTER(structs[base])
    if ptr and const and base == "char" and returned:
        return C.c_char_p
    if ptr and (base == "void" or base in _SCALARS):
        return C.c_void_p
    raise ValueError(f"{header}: type {spelling!r} is outside the C subset posetraj_amd.hip reads")


def _declarators(text: str, sep: str, header: str):
    """[(C type, name)] of a struct body (sep ';', several names per type allowed) or a parameter list (sep ',')."""
    out = []
    for decl in filter(None, (d.strip() for d in text.split(sep))):
        m = _FIELD.fullmatch(decl)
        if not m or (sep == "," and "," in m.group(2)):
            raise ValueError(f"{header}: cannot read the declaration {decl!r}")
        out += [(" ".join(m.group(1).split()), n.strip()) for n in m.group(2).split(",")]
    return out


def _parse_header(text: str, abi: Abi, known_structs: dict):
    """``abi`` with its version, structs, prototypes and signatures read from the text of its header.  Raises on anything it does
    not understand, naming the header; no declaration is skipped.  ``known_structs``: those of the headers before this one (they
    may appear in its prototypes; only its own are kept in the row)."""
    version = re.search(r"^#define\s+%s\s+(\d+)\s*$" % abi.macro, text, flags=re.M)
    if not version:
        raise ValueError(f"{abi.header}: no `#define {abi.macro} n`")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs, protos, pos = dict(known_structs), {}, 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if not m:
            raise ValueError(f"{abi.header}: cannot read the declaration {text[pos:].strip().split(';')[0][:200]!r}")
        if m.group("tag"):
            tag = m.group("tag")
            if tag not in abi.struct_classes:
                raise ValueError(f"{abi.header}: struct {tag!r} has no class name in the {abi.name!r} row of posetraj_amd.hip's table")
            fields = [(n, _ctype(t, structs, header=abi.header)) for t, n in _declarators(m.group("body"), ";", abi.header)]
            structs[tag] = type(abi.struct_classes[tag], (C.Structure,), {"_fields_": fields, "__doc__": f"``{tag}`` of include/{abi.header}."})
        elif m.group("fn"):
            params = m.group("params").strip()
            protos[m.group("fn")] = (" ".join(m.group("ret").split()), [] if params == "void" else [t for t, _ in _declarators(params, ",", abi.header)])
        pos = m.end()
    named = re.findall(_ENTRY + r"\s*\(", text)
    if len(named) != len(protos):
        raise ValueError(f"{abi.header}: {len(named)} names are followed by '(' but {len(protos)} prototypes were read")
    sigs = {name: (_ctype(ret, structs, True, abi.header), [_ctype(t, structs, header=abi.header) for t in params]) for name, (ret, params) in protos.items()}
    return abi._replace(version=int(version.group(1)), structs={k: v for k, v in structs.items() if k not in known_structs}, prototypes=protos, signatures=sigs)


ABIS = {}                            # name -> row, read; in _ROWS' order
for _abi in _ROWS:
    with open(os.path.join(INCLUDE, _abi.header)) as _f:
        ABIS[_abi.name] = _parse_header(_f.read(), _abi, {tag: cls for row in ABIS.values() for tag, cls in row.structs.items()})
    globals().update({cls.__name__: cls for cls in ABIS[_abi.name].structs.values()})       # IgemmParams ... GemmParams, Adam8Segment
with open(os.path.join(INCLUDE, _WINDOW_ROW.header)) as _f:
    WINDOW_ABI = _parse_header(_f.read(), _WINDOW_ROW, {})                                   # the add-on library's row, read the same way
# the core header's values under the names they have always had
_abi = ABIS["core"]
HEADER, STRUCT_CLASSES, ABI_VERSION, PROTOTYPES, SIGNATURES = os.path.join(INCLUDE, _abi.header), _abi.struct_classes, _abi.version, _abi.prototypes, _abi.signatures


def header_paths() -> list:
    """Every header the library is built from: a change of one rebuilds every object, and source_digest() covers them all."""
    return [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(INCLUDE, a.header) for a in ABIS.values()]


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> posetraj_amd/libposetraj_hip.so (cross-compiles without a GPU).  One object per
    source under ``csrc/_obj`` (re-compiled only when the source or a header is newer; up to 8 compiles in parallel, largest file first), then
    one link; then the add-on library ``libposetraj_window.so`` from ``csrc/window.hip`` by the same rule.  Refuses to run while ``PT_LIB`` points the loader at another library (an A/B build must not be overwritten
    by a build of the current tree)."""
    if os.environ.get("PT_LIB"):
        raise RuntimeError("posetraj_amd.hip.build: PT_LIB is set (A/B against another library); unset it to build the tree's own")
    from concurrent.futures import ThreadPoolExecutor
    hdr_time = max(os.path.getmtime(h) for h in header_paths())
    objdir = os.path.join(CSRC, "_obj")
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = []
    for name in SOURCES:
        src, obj = os.path.join(CSRC, name), os.path.join(objdir, name + ".o")
        rem = obj + ".remarks"
        if force or not (os.path.exists(obj) and os.path.exists(rem)) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            jobs.append((src, obj, rem))

    def compile_one(job):
        src, obj, rem = job
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed ({r.returncode}) on {os.path.basename(src)}:\n{r.stderr[-4000:]}")
        keep, on = [], False                                 # warnings are not remarks: show them (with their source excerpt)
        for ln in r.stderr.splitlines():
            if "warning:" in ln or "error:" in ln:
                on = True
            elif "remark:" in ln:
                on = False
            if on:
                keep.append(ln)
        if keep:
            print("\n".join(keep))
        with open(rem, "w") as f:
            f.write(r.stderr)

    if jobs:
        jobs.sort(key=lambda j: -os.path.getsize(j[0]))       # the long pole (igemm.hip: ~70 s of the build) starts first
        with ThreadPoolExecutor(max_workers=min(os.cpu_count() or 4, 8, len(jobs))) as ex:
            list(ex.map(compile_one, jobs))
    objs = [os.path.join(objdir, name + ".o") for name in SOURCES]
    if jobs or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc link failed ({r.returncode}):\n{r.stderr[-4000:]}")
        _write_resource_report("\n".join(open(o + ".remarks").read() for o in objs))
    # the add-on library of the windowed loop: same flags, same object directory, its source and its header its own rebuild inputs
    src, obj = os.path.join(CSRC, WINDOW_SOURCE), os.path.join(objdir, WINDOW_SOURCE + ".o")
    inputs = [src, os.path.join(INCLUDE, _WINDOW_ROW.header), os.path.join(CSRC, "pt_common.h"), os.path.join(INCLUDE, ABIS["core"].header)]
    if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(i) for i in inputs):
        compile_one((src, obj, obj + ".remarks"))
    if not os.path.exists(WINDOW_LIB_PATH) or os.path.getmtime(WINDOW_LIB_PATH) < os.path.getmtime(obj):
        cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", WINDOW_LIB_PATH, obj]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc link failed ({r.returncode}):\n{r.stderr[-4000:]}")
    return LIB_PATH


RESOURCES_PATH = os.path.join(HERE, "build_resources.json")


def _write_resource_report(remarks: str) -> None:
    """Register / spill counts per kernel from hipcc's kernel-resource-usage remarks -> posetraj_amd/build_resources.json.
    The pipelined igemm kernels live at the 256-register limit: a spill inside their K loop is a reload behind the LDS-DMA
    queue (tests/test_host_cpu.py asserts they have none)."""
    import json
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?:\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    if out:
        with open(RESOURCES_PATH, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)


def source_digest() -> str:
    """sha256 over the HIP sources + headers of the library (SOURCES and header_paths() in the order of their paths, each as file
    name, NUL, bytes): identifies a BUILD independently of where it was compiled.  Measurement files under profiles/ that only
    hold for one build (PMC traffic summaries) record it, and bench.py refuses to replay them for another."""
    import hashlib
    h = hashlib.sha256()
    for path in sorted([os.path.join(CSRC, s) for s in SOURCES] + header_paths()):
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    return h.hexdigest()


def _load(errcheck=None):
    """A handle of the library with every entry point of every row of ABIS typed from its signatures; raises if it has not been
    built (no CPU fallback exists).  With ``errcheck``, ctypes calls it on the result of every entry point that returns a status: return
    type ``int`` in the header, the row's version function excepted."""
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(posetraj_amd has no CPU or PyTorch fallback path)")
    L = C.CDLL(LIB_PATH)
    stale = []
    for abi in ABIS.values():
        for name, (res, args) in abi.signatures.items():
            fn = getattr(L, name)            # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
            if errcheck is not None and abi.prototypes[name][0] == "int" and name != abi.prefix + "abi_version":
                fn.errcheck = errcheck
        built = getattr(L, abi.prefix + "abi_version")()
        if built != abi.version:
            stale.append(f"{abi.name} {built} (header {abi.version})")
    if stale:
        raise RuntimeError(f"libposetraj_hip.so ABI versions differ from the headers': {', '.join(stale)}; rebuild")
    return L


def lib():
    """The loaded library, raw: every call returns what the C function returned."""
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def checked():
    """The same library through a second handle whose status-returning entry points raise like ``check`` on a non-zero
    status (ctypes' own ``errcheck``: no Python wrapper around the call).  What the product calls."""
    global _checked
    if _checked is None:
        _checked = _load(_raise_on_status)
    return _checked


def window():
    """The add-on library of the windowed denoise loop (include/posetraj_window.h), checked: a status-returning entry point raises
    ``RuntimeError`` with the library's own message on a non-zero status.  Raises if it has not been built or is of another version."""
    global _window
    if _window is None:
        if not os.path.exists(WINDOW_LIB_PATH):
            raise RuntimeError(f"{WINDOW_LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(posetraj_amd has no CPU or PyTorch fallback path)")
        L, abi = C.CDLL(WINDOW_LIB_PATH), WINDOW_ABI

        def raise_on_status(rc, fn, args):
            if rc != 0:
                raise RuntimeError(f"libposetraj_window: {fn.__name__} failed ({rc}): {L.ptw_last_error().decode()}")
            return rc

        for name, (res, args) in abi.signatures.items():
            fn = getattr(L, name)            # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
            if abi.prototypes[name][0] == "int" and name != abi.prefix + "abi_version":
                fn.errcheck = raise_on_status
        if L.ptw_abi_version() != abi.version:
            raise RuntimeError(f"libposetraj_window.so ABI version {L.ptw_abi_version()} differs from the header's {abi.version}; rebuild")
        _window = L
    return _window


def _raise_on_status(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__)
    return rc


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError(f"libposetraj_hip: {what} failed ({rc}): {lib().pt_last_error().decode()}")
