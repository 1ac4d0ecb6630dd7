"""ctypes binding of ``libposetraj_hip.so`` (C ABI declared in ``include/posetraj_hip.h``).

There is no fallback: if the library is missing or a call fails, a ``RuntimeError`` is raised.  ``build()``
compiles the HIP sources for gfx950 in-tree (``posetraj_amd/libposetraj_hip.so``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.abspath(os.environ["PT_LIB"]) if os.environ.get("PT_LIB") else os.path.join(HERE, "libposetraj_hip.so")   # PT_LIB: A/B against another build on one box
SOURCES = ["api.hip", "igemm.hip", "ffn.hip", "lnlin.hip", "norm.hip", "attn.hip", "attn_general.hip", "elementwise.hip", "vae.hip", "vae_f32.hip", "clip.hip", "raster.hip", "train.hip", "gemm.hip", "backward.hip", "attn_bwd.hip", "batch.hip", "control.hip", "sampler.hip"]
HEADERS = ["pt_common.h", "igemm_tail.h", "pt_fold.h"]
HEADER = os.path.join(HERE, "..", "include", "posetraj_hip.h")
STRUCT_CLASSES = {"pt_igemm_params": "IgemmParams", "pt_ffn_params": "FfnParams", "pt_lnlin_params": "LnLinParams",
                  "pt_conv_f32_params": "ConvF32Params", "pt_gemm_params": "GemmParams"}
# the optimizer extension (include/posetraj_optim.h: entry points `pto_*` of the same library, a version of its own)
OPTIM_HEADER = os.path.join(HERE, "..", "include", "posetraj_optim.h")
OPTIM_STRUCT_CLASSES = {"pt_adam8_segment": "Adam8Segment"}
# the deterministic-reduction extension (include/posetraj_det.h: entry points `ptd_*`, a version of its own; it reuses pt_gemm_params)
DET_HEADER = os.path.join(HERE, "..", "include", "posetraj_det.h")
# the long-clip extension (include/posetraj_temporal.h: entry points `ptt_*`, a version of its own): temporal attention backward of 33 - 128 frames
TEMPORAL_HEADER = os.path.join(HERE, "..", "include", "posetraj_temporal.h")
# the clip-batch extension (include/posetraj_batch.h: entry points `ptb_*`, a version of its own): the temporal blocks' cross-attention rows of a batch
BATCH_HEADER = os.path.join(HERE, "..", "include", "posetraj_batch.h")
# the control-weight extension (include/posetraj_control.h: entry points `ptc_*`, a version of its own): per-row weighted accumulation of the ControlNet residuals
CONTROL_HEADER = os.path.join(HERE, "..", "include", "posetraj_control.h")
# the sampler extension (include/posetraj_sampler.h: entry points `pts_*`, a version of its own): the linear multistep (DPM-Solver++(2M)) step
SAMPLER_HEADER = os.path.join(HERE, "..", "include", "posetraj_sampler.h")

_lib = _checked = None

# ---------------------------------------------------------------------------------------------------------------------
# The header is the only description of the ABI: the parameter structs, the signature table and the version below are
# read from it at import (the C subset it uses, nothing more; tests/test_host_cpu.py has a C++ compiler confirm the reading).
# ---------------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_TYPE = r"(?:const\s+)?\w+\s*\*?"
_DECL = re.compile(r"""\s*(?: typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P=tag)\s*;
                            | (?P<ret>%s)\s*\b(?P<fn>pt[odtbcs]?_[a-z0-9_]+)\s*\((?P<params>[^()]*)\)\s*;
                            | extern\s+"C"\s*\{ | \} )""" % _TYPE, re.X)
_FIELD = re.compile(r"(%s)\s*\b(\w+(?:\s*,\s*\w+)*)" % _TYPE)         # `int32_t C0, C1`, `const void* x0`; a parameter is the one-name case


def _ctype(spelling: str, structs: dict, returned: bool = False):
    """ctypes type of a C type as the header spells it: scalars by name, `const pt_X_params*` a pointer to that struct,
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
    raise ValueError(f"posetraj_hip.h: type {spelling!r} is outside the C subset posetraj_amd.hip reads")


def _declarators(text: str, sep: str):
    """[(C type, name)] of a struct body (sep ';', several names per type allowed) or a parameter list (sep ',')."""
    out = []
    for decl in filter(None, (d.strip() for d in text.split(sep))):
        m = _FIELD.fullmatch(decl)
        if not m or (sep == "," and "," in m.group(2)):
            raise ValueError(f"posetraj_hip.h: cannot read the declaration {decl!r}")
        out += [(" ".join(m.group(1).split()), n.strip()) for n in m.group(2).split(",")]
    return out


def _parse_header(text: str, struct_classes: dict = STRUCT_CLASSES, version_macro: str = "PT_ABI_VERSION", known_structs: dict = None):
    """(PT_ABI_VERSION, {struct tag: Structure class}, {entry point: (C return type, [C parameter types])}).  Raises on
    anything it does not understand; no declaration is skipped.  (The messages say posetraj_hip.h for every header.)  ``known_structs``:
    those of a header this one includes (they may appear in its prototypes; only its own are returned)."""
    version = re.search(r"^#define\s+%s\s+(\d+)\s*$" % version_macro, text, flags=re.M)
    if not version:
        raise ValueError(f"posetraj_hip.h: no `#define {version_macro} n`")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs, protos, pos = dict(known_structs or {}), {}, 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if not m:
            raise ValueError(f"posetraj_hip.h: cannot read the declaration {text[pos:].strip().split(';')[0][:200]!r}")
        if m.group("tag"):
            tag = m.group("tag")
            if tag not in struct_classes:
                raise ValueError(f"posetraj_hip.h: struct {tag!r} has no class name in posetraj_amd.hip.STRUCT_CLASSES")
            fields = [(n, _ctype(t, structs)) for t, n in _declarators(m.group("body"), ";")]
            structs[tag] = type(struct_classes[tag], (C.Structure,), {"_fields_": fields, "__doc__": f"``{tag}`` of include/posetraj_hip.h."})
        elif m.group("fn"):
            params = m.group("params").strip()
            protos[m.group("fn")] = (" ".join(m.group("ret").split()), [] if params == "void" else [t for t, _ in _declarators(params, ",")])
        pos = m.end()
    named = re.findall(r"pt[odtbcs]?_[a-z0-9_]+\s*\(", text)
    if len(named) != len(protos):
        raise ValueError(f"posetraj_hip.h: {len(named)} names are followed by '(' but {len(protos)} prototypes were read")
    return int(version.group(1)), {k: v for k, v in structs.items() if k not in (known_structs or {})}, protos


with open(HEADER) as _f:
    ABI_VERSION, _STRUCTS, PROTOTYPES = _parse_header(_f.read())       # PROTOTYPES: the C spelling, name -> (return type, [parameter types])
IgemmParams, FfnParams, LnLinParams, ConvF32Params, GemmParams = (_STRUCTS[tag] for tag in STRUCT_CLASSES)         # in STRUCT_CLASSES' order
# name -> (restype, argtypes); every symbol include/posetraj_hip.h declares
SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in PROTOTYPES.items()}
with open(OPTIM_HEADER) as _f:
    OPTIM_ABI_VERSION, _OPTIM_STRUCTS, OPTIM_PROTOTYPES = _parse_header(_f.read(), OPTIM_STRUCT_CLASSES, "PT_OPTIM_ABI_VERSION")
Adam8Segment = _OPTIM_STRUCTS["pt_adam8_segment"]
OPTIM_SIGNATURES = {name: (_ctype(ret, _OPTIM_STRUCTS, returned=True), [_ctype(t, _OPTIM_STRUCTS) for t in params])
                    for name, (ret, params) in OPTIM_PROTOTYPES.items()}
with open(DET_HEADER) as _f:
    DET_ABI_VERSION, _, DET_PROTOTYPES = _parse_header(_f.read(), {}, "PT_DET_ABI_VERSION", _STRUCTS)
DET_SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in DET_PROTOTYPES.items()}
with open(TEMPORAL_HEADER) as _f:
    TEMPORAL_ABI_VERSION, _, TEMPORAL_PROTOTYPES = _parse_header(_f.read(), {}, "PT_TEMPORAL_ABI_VERSION", _STRUCTS)
TEMPORAL_SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in TEMPORAL_PROTOTYPES.items()}
with open(BATCH_HEADER) as _f:
    BATCH_ABI_VERSION, _, BATCH_PROTOTYPES = _parse_header(_f.read(), {}, "PT_BATCH_ABI_VERSION", _STRUCTS)
BATCH_SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in BATCH_PROTOTYPES.items()}
with open(CONTROL_HEADER) as _f:
    CONTROL_ABI_VERSION, _, CONTROL_PROTOTYPES = _parse_header(_f.read(), {}, "PT_CONTROL_ABI_VERSION", _STRUCTS)
CONTROL_SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in CONTROL_PROTOTYPES.items()}
with open(SAMPLER_HEADER) as _f:
    SAMPLER_ABI_VERSION, _, SAMPLER_PROTOTYPES = _parse_header(_f.read(), {}, "PT_SAMPLER_ABI_VERSION", _STRUCTS)
SAMPLER_SIGNATURES = {name: (_ctype(ret, _STRUCTS, returned=True), [_ctype(t, _STRUCTS) for t in params]) for name, (ret, params) in SAMPLER_PROTOTYPES.items()}


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> posetraj_amd/libposetraj_hip.so (cross-compiles without a GPU).  One object per
    source under ``csrc/_obj`` (re-compiled only when the source or a header is newer; up to 8 compiles in parallel, largest file first), then
    one link.  Refuses to run while ``PT_LIB`` points the loader at another library (an A/B build must not be overwritten
    by a build of the current tree)."""
    if os.environ.get("PT_LIB"):
        raise RuntimeError("posetraj_amd.hip.build: PT_LIB is set (A/B against another library); unset it to build the tree's own")
    from concurrent.futures import ThreadPoolExecutor
    headers = [os.path.join(CSRC, h) for h in HEADERS] + [HEADER, OPTIM_HEADER, DET_HEADER, TEMPORAL_HEADER, BATCH_HEADER, CONTROL_HEADER, SAMPLER_HEADER]
    hdr_time = max(os.path.getmtime(h) for h in headers)
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
    """sha256 over the HIP sources + headers of the library: identifies a BUILD independently of where it was compiled.
    Measurement files under profiles/ that only hold for one build (PMC traffic summaries) record it, and bench.py refuses
    to replay them for another."""
    import hashlib
    h = hashlib.sha256()
    for path in sorted([os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [HEADER, OPTIM_HEADER, DET_HEADER, TEMPORAL_HEADER, BATCH_HEADER, CONTROL_HEADER, SAMPLER_HEADER]):
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    return h.hexdigest()


def _load(errcheck=None):
    """A handle of the library with every entry point typed from SIGNATURES; raises if it has not been built (no CPU
    fallback exists).  With ``errcheck``, ctypes calls it on the result of every entry point that returns a status: return
    type ``int`` in the header, pt_abi_version excepted."""
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(posetraj_amd has no CPU or PyTorch fallback path)")
    L = C.CDLL(LIB_PATH)
    for sigs, protos in ((SIGNATURES, PROTOTYPES), (OPTIM_SIGNATURES, OPTIM_PROTOTYPES), (DET_SIGNATURES, DET_PROTOTYPES),
                         (TEMPORAL_SIGNATURES, TEMPORAL_PROTOTYPES), (BATCH_SIGNATURES, BATCH_PROTOTYPES), (CONTROL_SIGNATURES, CONTROL_PROTOTYPES),
                         (SAMPLER_SIGNATURES, SAMPLER_PROTOTYPES)):
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)            # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
            if errcheck is not None and protos[name][0] == "int" and name not in ("pt_abi_version", "pto_abi_version", "ptd_abi_version", "ptt_abi_version", "ptb_abi_version", "ptc_abi_version", "pts_abi_version"):
                fn.errcheck = errcheck
    if (L.pt_abi_version() != ABI_VERSION or L.pto_abi_version() != OPTIM_ABI_VERSION or L.ptd_abi_version() != DET_ABI_VERSION
            or L.ptt_abi_version() != TEMPORAL_ABI_VERSION or L.ptb_abi_version() != BATCH_ABI_VERSION or L.ptc_abi_version() != CONTROL_ABI_VERSION
            or L.pts_abi_version() != SAMPLER_ABI_VERSION):
        raise RuntimeError(f"libposetraj_hip.so ABI {L.pt_abi_version()} / optimizer extension {L.pto_abi_version()} / deterministic extension "
                           f"{L.ptd_abi_version()} / long-clip extension {L.ptt_abi_version()} / clip-batch extension {L.ptb_abi_version()} / control-weight extension "
                           f"{L.ptc_abi_version()} / sampler extension {L.pts_abi_version()} != expected {ABI_VERSION} / {OPTIM_ABI_VERSION} / {DET_ABI_VERSION} / "
                           f"{TEMPORAL_ABI_VERSION} / {BATCH_ABI_VERSION} / {CONTROL_ABI_VERSION} / {SAMPLER_ABI_VERSION}; rebuild")
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


def _raise_on_status(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__)
    return rc


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError(f"libposetraj_hip: {what} failed ({rc}): {lib().pt_last_error().decode()}")
