"""The C-ABI library: loads on a CPU-only box, exports exactly what include/rsm.h declares, and refuses to
run without a GPU (no CPU fallback anywhere in the product path)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsm.h")


def declared():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rsm_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_what_the_binding_lists():
    from reconstruction_amd import _lib
    assert declared() == sorted(_lib.EXPORTS)


def test_library_loads_and_exports_every_declared_symbol():
    from reconstruction_amd import _lib
    lib = _lib.load()
    for name in declared():
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rsm_[a-z0-9_]+)", out))
    assert exported == set(declared()), exported ^ set(declared())
    assert lib.rsm_version().startswith(b"rsm-mi355")
    assert lib.rsm_profile_stage_count() >= 10


def test_struct_layouts_match_the_header():
    from reconstruction_amd import _lib
    # rsm_boundary = 6 ints; rsm_pair_in: 4 ptr + 4 int + (pad) double + 2 int + 28 double + int
    assert C.sizeof(_lib.Boundary) == 24
    assert C.sizeof(_lib.PairIn) == 4 * 8 + 4 * 4 + 8 + 2 * 4 + 28 * 8 + 8
    assert C.sizeof(_lib.PairOut) == 2 * 8 + 2 * 24 + 8 + 8 + 8 + 8 + 8 + 8


MIRRORS = {"rsm_boundary": "Boundary", "rsm_pair_in": "PairIn", "rsm_pair_out": "PairOut", "rsm_filter_params": "FilterParams", "rsm_mls_params": "MlsParams",
           "rsm_poisson_params": "PoissonParams", "rsm_mesh_clean_params": "MeshCleanParams", "rsm_mesh_color_params": "MeshColorParams",
           "rsm_dedup_view": "DedupView", "rsm_rectify_in": "RectifyIn", "rsm_rectify_out": "RectifyOut"}


def test_struct_layouts_as_the_c_compiler_sees_them(tmp_path):
    """sizeof / offsetof of every struct the binding mirrors, from gcc itself, against the ctypes classes; the member names come from each
    class's _fields_, so a member the header does not have fails to compile."""
    from reconstruction_amd import _lib
    src = tmp_path / "layout.c"
    mirror = {t: getattr(_lib, c) for t, c in MIRRORS.items()}
    body = "".join('printf("%s %%zu\\n", sizeof(%s));\n' % (t, t) + "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (t, f, t, f) for f, _ in c._fields_)
                   for t, c in mirror.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n%sprintf("rsm_point16 %%zu\\n", sizeof(rsm_point16));\nreturn 0; }\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for t, c in mirror.items():
        assert int(got[t]) == C.sizeof(c), t
        for f, _ in c._fields_:
            assert int(got["%s.%s" % (t, f)]) == getattr(c, f).offset, (t, f)
    assert int(got["rsm_point16"]) == 16


# the header's scalar vocabulary -> (bytes, signed, floating); a type that is not listed fails the prototype test
SCALARS = {"int": (4, True, False), "int64_t": (8, True, False), "long long": (8, True, False), "uint32_t": (4, False, False),
           "size_t": (8, False, False), "double": (8, True, True)}


def header_prototypes():
    """{name: (return kind, [parameter kind])} of every function include/rsm.h declares; a kind is "void", "ptr" or a key of SCALARS."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    txt = re.sub(r"typedef\s+(struct|enum)\s+\w+\s*\{.*?\}\s*\w+\s*;", "", txt, flags=re.S)

    def kind(decl, named):
        decl = decl.strip()
        if "*" in decl or "[" in decl:
            return "ptr"
        words = [w for w in decl.split() if w != "const"]
        return " ".join(words[:-1] if named else words)

    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?[\s*]+)(rsm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        params = [] if params.strip() == "void" else [kind(q, True) for q in params.split(",")]
        protos[name] = (kind(ret, False), params)
    return protos


def shape(t):
    """A ctypes type of the binding's table as "void", "ptr" or a value of SCALARS."""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    return (C.sizeof(t), t(-1).value < 0, t is C.c_double)


def test_every_prototype_of_the_binding_matches_the_header():
    """Return kind, parameter count and, per parameter, pointer or scalar -- and a scalar's width, signedness and integer / double --
    of every row of _lib.PROTOTYPES against include/rsm.h."""
    from reconstruction_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == declared() == sorted(_lib.PROTOTYPES) and len(protos) >= 94
    want = dict(SCALARS, ptr="ptr", void="void")
    for name, (ret, params) in protos.items():
        assert ret in want and set(params) <= set(want) - {"void"}, (name, ret, params)   # a type the header grew and this test does not know
        restype, argtypes = _lib.PROTOTYPES[name]
        assert shape(restype) == want[ret], (name, "returns", ret)
        assert len(argtypes) == len(params), (name, len(params))
        for i, (t, k) in enumerate(zip(argtypes, params)):
            assert shape(t) == want[k], (name, i, k, t)


def test_no_function_is_left_without_a_prototype():
    from reconstruction_amd import _lib
    lib = _lib.load()
    assert _lib.EXPORTS == list(_lib.PROTOTYPES)
    for name in _lib.EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(_lib.PROTOTYPES[name][1]), name
        assert fn.restype == _lib.PROTOTYPES[name][0], name


def test_abi_constant_is_the_headers():
    from reconstruction_amd import _lib
    m = re.search(r"^#define\s+RSM_ABI_VERSION\s+(\d+)\s*$", open(HEADER).read(), flags=re.M)
    assert m and _lib.RSM_ABI_VERSION == int(m.group(1)) == _lib.load().rsm_abi_version()


def test_no_gpu_means_error_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from reconstruction_amd import Context, RsmError
    with pytest.raises(RsmError):
        Context(0)


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "reconstruction_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                # comments may mention the oracle; nothing may import, include, link or load it
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
                assert not re.search(r"#\s*include\s*[<\"][^>\"]*oracle", txt), f
                assert "liborc" not in txt and "orc_match_pair" not in txt, f


def test_header_is_plain_c():
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mock_adapter_program_builds_and_links(tmp_path):
    """tests/cpp/mock_adapter.cpp (the traits-based adapter with mock types) compiles with plain g++ and links against
    the C-ABI library; it is executed on the GPU box."""
    from reconstruction_amd import _lib
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "mock_adapter.cpp"), "-o", str(tmp_path / "mock_adapter"),
                        "-L" + os.path.dirname(_lib.LIB_PATH), "-lrsm_mi355", "-Wl,-rpath-link,/opt/rocm/lib",
                        "-Wl,--allow-shlib-undefined", "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# Every name rsm_set_option took while it was a chain of `!strcmp(name, "...")` (commit 4f0d0b9): the 34 which that pattern with
# the class [a-z_0-9] finds there, and the two with a capital letter which it could not see.  The table takes these and no others.
OPTION_NAMES = ["cu_share", "filter_ladder_h", "filter_list", "filter_low_priority", "filter_normals_window", "filter_wg_max",
                "filter_window", "heavy_exclusive", "heavy_from_sweep", "heavy_lanes", "heavy_min_px", "meshcolor_big_box", "ncc_bytes",
                "ncc_mid", "ncc_slide_max", "no_exact", "no_rowgemm", "refine_prefill", "refine_rekey_side", "refine_rekey_until",
                "refine_skew_from", "refine_skew_min_px", "refine_skew_prio", "refine_skew_rows", "refine_skew_uw", "refine_skew_waves",
                "refine_skew_waves_alone", "refine_skew_waves_low", "refine_split", "refine_tile_from", "refine_tile_min_px",
                "refine_upd_cap", "shared_gpu", "wide_rows"] + ["refine_skew_T", "refine_tile_T"]


def test_every_option_of_rsm_set_option_is_documented_in_the_header():
    """include/rsm.h lists the tuning knobs; a name rsm_set_option accepts and the header does not mention is a knob nobody
    can find."""
    src = open(os.path.join(ROOT, "reconstruction_amd", "csrc", "rsm_api.hip")).read()
    # the rows of kOptions (name, member, ...) and of kSpecialOptions (name, handler)
    names = sorted(set(re.findall(r'^\s*\{"([A-Za-z_0-9]+)", (?:&rsm_ctx::\w+, OPT_|set_\w+\})', src, flags=re.M)))
    assert names == sorted(OPTION_NAMES), set(names) ^ set(OPTION_NAMES)
    hdr = open(os.path.join(ROOT, "include", "rsm.h")).read()
    missing = [n for n in names if '"%s"' % n not in hdr]
    assert not missing, missing
