"""The C ABI contract, once for every header: ``posetraj_amd.hip``'s table against the literal rows below, the header text, a C++
compiler, the symbols the built library exports, the two ctypes handles, the product's call sites and the build's inputs.  A new
header is one row of ``EXPECT`` here and one row of ``hip``'s table; nothing below names a header.  No kernel runs here."""
import ast
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import pytest

# (name, file under include/, prefix, version macro, version, entry points, call sites in posetraj_amd/*.py, of which keyword or starred)
EXPECT = [
    ("core", "posetraj_hip.h", "pt_", "PT_ABI_VERSION", 10, 76, 73, 2),
    ("optim", "posetraj_optim.h", "pto_", "PT_OPTIM_ABI_VERSION", 1, {"pto_abi_version", "pto_adamw8_f32", "pto_adam8_dequant_f32"}, 2, 0),
    ("det", "posetraj_det.h", "ptd_", "PT_DET_ABI_VERSION", 1,
     {"ptd_abi_version", "ptd_groupnorm_bwd_ws_floats", "ptd_groupnorm_bwd", "ptd_layernorm_bwd_ws_floats", "ptd_layernorm_bwd",
      "ptd_colsum_ws_floats", "ptd_colsum_f16", "ptd_dot_diff_ws_floats", "ptd_dot_diff", "ptd_dot_diff_dev", "ptd_sumsq_ws_floats",
      "ptd_sumsq_f32", "ptd_gemm_ws_floats", "ptd_gemm_f16"}, 13, 0),
    ("temporal", "posetraj_temporal.h", "ptt_", "PT_TEMPORAL_ABI_VERSION", 1, {"ptt_abi_version", "ptt_attn_temporal_bwd_long_f16"}, 1, 0),
    ("batch", "posetraj_batch.h", "ptb_", "PT_BATCH_ABI_VERSION", 1,
     {"ptb_abi_version", "ptb_add_rowvec_interleaved_f16", "ptb_colsum_interleaved_f16", "ptb_colsum_interleaved_ws_floats",
      "ptb_colsum_interleaved_det_f16"}, 4, 0),
    ("control", "posetraj_control.h", "ptc_", "PT_CONTROL_ABI_VERSION", 1, {"ptc_abi_version", "ptc_weighted_residual_add_f16"}, 1, 0),
    ("sampler", "posetraj_sampler.h", "pts_", "PT_SAMPLER_ABI_VERSION", 1, {"pts_abi_version", "pts_cfg_multistep_step", "pts_multistep_step"}, 2, 0),
]
# {struct tag: Python class name} of the rows that declare structs
STRUCTS = {"core": {"pt_igemm_params": "IgemmParams", "pt_ffn_params": "FfnParams", "pt_lnlin_params": "LnLinParams",
                    "pt_conv_f32_params": "ConvF32Params", "pt_gemm_params": "GemmParams"},
           "optim": {"pt_adam8_segment": "Adam8Segment"}}
# the core entry points that return something other than a status (test_checked_handle_raises_where_the_raw_one_returns calls some)
CORE_PLAIN = {"pt_abi_version", "pt_last_error", "pt_igemm_splitk_ws_bytes", "pt_groupnorm_scratch_floats", "pt_prof_collect_list"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
each_row = pytest.mark.parametrize("row", EXPECT, ids=[r[0] for r in EXPECT])


@pytest.fixture(scope="module")
def hip():
    from posetraj_amd import hip
    hip.build()
    return hip


@pytest.fixture(scope="module")
def exported(hip):
    """Every unmangled symbol the library defines that looks like an entry point."""
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and re.match(r"^pt[a-z]?_", ln.split()[-1])}


def header_text(row):
    return open(os.path.join(ROOT, "include", row[1])).read()


def test_the_table_has_exactly_these_rows_in_this_order(hip):
    assert [(a.name, a.header, a.prefix, a.macro, a.version) for a in hip.ABIS.values()] == [r[:5] for r in EXPECT]
    assert list(hip.ABIS) == [r[0] for r in EXPECT] and {a.name: a.struct_classes for a in hip.ABIS.values() if a.struct_classes} == STRUCTS
    core = hip.ABIS["core"]
    assert (hip.ABI_VERSION, hip.SIGNATURES, hip.PROTOTYPES, hip.STRUCT_CLASSES) == (10, core.signatures, core.prototypes, core.struct_classes)
    assert len(hip.SIGNATURES) == 76 and os.path.samefile(hip.HEADER, os.path.join(ROOT, "include", "posetraj_hip.h"))
    sets = [set(a.signatures) for a in hip.ABIS.values()]
    assert sum(len(s) for s in sets) == len(set().union(*sets))                   # pairwise disjoint


@each_row
def test_versions_agree_in_the_header_the_table_and_both_handles(hip, row):
    name, _, prefix, macro, version = row[:5]
    assert re.search(r"^#define\s+%s\s+%d\s*$" % (macro, version), header_text(row), flags=re.M)
    assert hip.ABIS[name].version == version
    assert getattr(hip.lib(), prefix + "abi_version")() == getattr(hip.checked(), prefix + "abi_version")() == version


@each_row
def test_the_header_declares_exactly_the_bound_names(hip, row):
    name, prefix, entries = row[0], row[2], row[5]
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text(row), flags=re.S)
    declared = set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % re.escape(prefix), code))
    abi = hip.ABIS[name]
    assert declared == set(abi.signatures) == set(abi.prototypes), declared ^ set(abi.signatures)
    assert declared == entries if isinstance(entries, set) else len(declared) == entries
    assert all(n.startswith(prefix) and not n.startswith(tuple(r[2] for r in EXPECT if r[2] != prefix)) for n in declared)


@each_row
def test_a_compiler_confirms_the_bindings_read_from_the_header(hip, row, tmp_path):
    """posetraj_amd.hip reads the structs and prototypes of a header with a small parser of its own; a C++ compiler is the independent
    judge of that reading.  One translation unit includes the real header and asserts, from the ctypes tables, the size of every
    struct, the offset and size of every field and the exact type of every entry point (the C spelling the parser kept beside the
    ctypes type: `const float*` and `void*` differ here).  A wrong regex, type map, field order or padding does not compile."""
    abi = hip.ABIS[row[0]]
    spelled = {}                                                                 # ctypes.c_int IS ctypes.c_int32 where int has 32 bits
    for c_type, ct in (("int", ctypes.c_int), ("int32_t", ctypes.c_int32), ("int64_t", ctypes.c_int64), ("float", ctypes.c_float), ("double", ctypes.c_double)):
        spelled.setdefault(ct, set()).add(c_type)
    tu = ["#include <cstddef>", "#include <type_traits>", '#include "posetraj_hip.h"', f'#include "{row[1]}"']
    assert set(abi.structs) == set(abi.struct_classes)
    for tag, name in abi.struct_classes.items():
        cls = getattr(hip, name)
        assert cls is abi.structs[tag]
        tu.append(f"static_assert(sizeof({tag}) == {ctypes.sizeof(cls)}, \"sizeof {tag}\");")
        for field, typ in cls._fields_:
            tu.append(f"static_assert(offsetof({tag}, {field}) == {getattr(cls, field).offset} && sizeof({tag}::{field}) == {ctypes.sizeof(typ)}, \"{tag}.{field}\");")
    for fn, (ret, params) in abi.prototypes.items():
        res, args = abi.signatures[fn]
        assert len(args) == len(params), fn
        for c_type, ct in zip([ret] + params, [res] + args):                    # the ctypes side agrees with the spelling the compiler judges
            assert c_type in spelled[ct] if ct in spelled else c_type.endswith("*"), (fn, c_type, ct)
        tu.append(f"static_assert(std::is_same_v<decltype(&{fn}), {ret} (*)({', '.join(params) or 'void'})>, \"{fn}\");")
    tu.append(f"static_assert({row[3]} == {row[4]} && PT_ABI_VERSION == 10, \"versions\");")
    src = tmp_path / "abi_probe.cpp"
    src.write_text("\n".join(tu) + "\n")
    cxx = shutil.which("c++") or shutil.which("clang++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@each_row
def test_the_library_exports_the_rows_names_and_no_other_with_its_prefix(hip, exported, row):
    defined = {n for n in exported if n.startswith(row[2])}
    assert defined == set(hip.ABIS[row[0]].signatures), defined ^ set(hip.ABIS[row[0]].signatures)
    assert all(hasattr(hip.lib(), n) for n in defined)


def test_the_library_exports_no_entry_point_outside_the_table(hip, exported):
    """A prefix nobody registered: every defined unmangled ``pt_`` / ``pt<letter>_`` symbol belongs to some row."""
    assert exported == {n for a in hip.ABIS.values() for n in a.signatures}


@each_row
def test_errcheck_is_set_on_status_returns_of_the_checked_handle_only(hip, row):
    abi, L, C = hip.ABIS[row[0]], hip.lib(), hip.checked()
    status = {n for n, (ret, _) in abi.prototypes.items() if ret == "int" and n != row[2] + "abi_version"}
    if row[0] == "core":
        assert status == set(abi.prototypes) - CORE_PLAIN
    for n in abi.signatures:
        assert (getattr(C, n).errcheck is hip._raise_on_status) == (n in status), n
        assert not getattr(L, n).errcheck, n


@each_row
def test_product_calls_pass_as_many_arguments_as_the_header_declares(hip, row):
    """Every call of an entry point in posetraj_amd/*.py, by its attribute name: positional arguments == parameters of the prototype.
    (ctypes reports a wrong count only when the call runs - on the GPU.)  Keyword and starred calls cannot be counted: the core
    has two (optim.py's pt_adamw_fused_f32 and pt_adamw_ema_f32), the extensions none.  The site counts are the census of the
    tree; every entry point of an extension but its version function is called."""
    abi, pkg = hip.ABIS[row[0]], os.path.join(ROOT, "posetraj_amd")
    names = set(abi.signatures) - {row[2] + "abi_version"}
    sites, skipped = [], []
    for f in sorted(f for f in os.listdir(pkg) if f.endswith(".py")):
        for node in ast.walk(ast.parse(open(os.path.join(pkg, f)).read())):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names:
                sites.append(node.func.attr)
                if node.keywords or any(isinstance(a, ast.Starred) for a in node.args):
                    skipped.append((f, node.lineno))
                    continue
                assert len(node.args) == len(abi.signatures[node.func.attr][1]), (f, node.lineno, node.func.attr)
    assert len(sites) == row[6] and len(skipped) <= row[7], (len(sites), skipped)
    assert row[0] == "core" or set(sites) == names, names - set(sites)


def test_one_list_of_headers_feeds_the_rebuild_check_and_the_digest(hip, monkeypatch, tmp_path):
    """hip.header_paths() holds every row's header and every csrc/ header; source_digest() is the documented hash over the sources
    and exactly those paths; build() asks the same function: a path that does not exist stops it before any compiler runs."""
    paths = hip.header_paths()
    csrc = os.path.join(ROOT, "posetraj_amd", "csrc")
    want = [os.path.join(csrc, h) for h in hip.HEADERS] + [os.path.join(ROOT, "include", r[1]) for r in EXPECT]
    assert len(paths) == len(want) and all(os.path.samefile(p, w) for p, w in zip(paths, want))
    assert "pt_fold.h" in hip.HEADERS and all(s.endswith(".hip") and os.path.exists(os.path.join(csrc, s)) for s in hip.SOURCES)
    h = hashlib.sha256()
    for path in sorted([os.path.join(hip.CSRC, s) for s in hip.SOURCES] + paths):
        h.update(os.path.basename(path).encode() + b"\0" + open(path, "rb").read())
    assert h.hexdigest() == hip.source_digest()
    missing = str(tmp_path / "not_a_header.h")
    monkeypatch.setattr(hip, "header_paths", lambda: paths + [missing])
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: pytest.fail("build() reached a compiler"))
    monkeypatch.delenv("PT_LIB", raising=False)
    with pytest.raises(FileNotFoundError, match="not_a_header.h"):
        hip.build()
    with pytest.raises(FileNotFoundError, match="not_a_header.h"):
        hip.source_digest()
